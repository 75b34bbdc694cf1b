#!/usr/bin/env python3
"""resolve_cost.py -- what the Query step (lexemes or keys -> ascending term ids) costs on the host and on the device.  One job on one
MI355X:
  (a) keys entry.  Batches of 1024 x 5 keys (C3's shape) and 1024 x 2..8 mixed, over vocabularies of 30 k (C3's size), 1 M and 8 M terms
      (indexes of one posting a term: only the vocabulary matters).  Host: ONE vbm25_lookup_terms call over the batch's keys, then
      std::sort + unique + drop per query.  Device: Resolver.submit_keys + collect one batch at a time, and the same at depth 3
      sustained.
  (b) lexeme entry.  The same shapes with 0 %, 5 % and 100 % of the lexemes on the hash path (24-byte lexemes; the others are decimal
      strings).  Host: vbm25_intern a lexeme + the steps of (a).  Device: Resolver.submit (prepacked arrays) + collect, likewise.
      The host side of (a) and (b) is timed inside a small C++ program (tools/resolve_host_cost.cpp, built here), so no ctypes call
      overhead is charged to it; the device side is timed from Python around the two ctypes calls, which it therefore includes.
  (c) end to end on C3's index: lexemes -> Resolver ring (depth 2) -> Stream ring (depth 3) in queries/s, beside term ids -> Stream
      ring from the same process.
  (d) kernel time alone for (a) and (b): the resolver's HIP events around a batch's kernels (upload and the host's copies excluded).
Every device result is checked against the host program's checksum of (q_off, term_ids).  Host clock around synchronous calls,
WARMUP untimed and REPS timed repetitions, median / min / max.  Prints one JSON object (and writes it to the path given first).

  python tools/resolve_cost.py profiles/resolve_cost.json [--vocab 30000,1000000,8000000] [--skip-c3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, REPS, RING_STEPS = 5, 30, 60
SEED = bytes(range(32))
NQ = 1024


def ms(ts):
    return {"median": round(statistics.median(ts) * 1e3, 4), "min": round(min(ts) * 1e3, 4), "max": round(max(ts) * 1e3, 4)}


def fnv(q_off, term_ids):
    h = 1469598103934665603
    for v in list(q_off) + list(term_ids):
        h = ((h ^ int(v)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def lexeme_of(i):
    """the vocabulary: even numbers are decimal strings (the padded path), odd ones 24-byte lexemes (the hash)"""
    return b"%d" % i if i % 2 == 0 else b"hashed-lexeme-%010d" % i


def vocabulary(vb, n_terms):
    """keys of lexeme_of(0 .. n_terms) in key order (interned on the device: tests/test_gpu_resolve.py holds that equal to vbm25_intern)"""
    lex = [lexeme_of(i) for i in range(n_terms)]
    data = b"".join(lex)
    lens = np.fromiter(map(len, lex), dtype=np.uint64, count=n_terms)
    del lex
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    keys = vb.intern_batch((np.frombuffer(data, dtype=np.uint8), off), SEED)
    order = np.lexsort((keys[:, 8:].copy().view(">u8").ravel(), keys[:, :8].copy().view(">u8").ravel()))
    return np.ascontiguousarray(keys[order])


def make_case(vb, n_terms, rng, lens, hashed):
    """nq queries of the given lengths over the vocabulary, `hashed` of the lexemes from its odd (hashed) half"""
    n = int(lens.sum())
    pick = rng.integers(0, n_terms // 2, n) * 2
    pick[rng.random(n) < hashed] += 1
    lex = [lexeme_of(int(i)) for i in pick]
    data = np.frombuffer(b"".join(lex), dtype=np.uint8)
    lex_off = np.concatenate([[0], np.cumsum([len(t) for t in lex])]).astype(np.uint64)
    q_lex = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    keys = vb.intern_batch((data, lex_off), SEED)
    return dict(data=data, lex_off=lex_off, q_lex=q_lex, keys=keys)


def kernel_ms(vb, r):
    f = vb.lib().vbm25_debug_resolver_kernel_ms
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    out = C.c_double()
    vb.api.check(f(r.h, C.byref(out)))
    return out.value


def device_side(vb, gix, case, entry):
    n_lex, n_bytes = len(case["lex_off"]) - 1, int(case["lex_off"][-1])
    if entry == "keys":
        def submit(r):
            r.submit_keys(case["keys"], case["q_lex"])
    else:
        packed = (case["data"], case["lex_off"], case["q_lex"])

        def submit(r):
            r.submit(packed)
    r = vb.Resolver(gix, 3, NQ, n_lex, n_bytes, seed=SEED)
    one, kern = [], []
    for i in range(WARMUP + REPS):
        t = time.perf_counter()
        submit(r)
        ids, off = r.collect()
        t = time.perf_counter() - t
        if i >= WARMUP:
            one.append(t)
            kern.append(kernel_ms(vb, r) * 1e-3)

    def ring(n):
        for _ in range(3):
            submit(r)
        for _ in range(n - 3):
            r.collect()
            submit(r)
        for _ in range(3):
            r.collect()
    ring(WARMUP + 3)
    t = time.perf_counter()
    ring(RING_STEPS)
    t = time.perf_counter() - t
    return dict(one_batch_ms=ms(one), kernels_ms=ms(kern), depth3_step_ms=round(t / RING_STEPS * 1e3, 4),
                depth3_queries_per_s=round(NQ * RING_STEPS / t), checksum=fnv(off, ids), n_ids=int(off[-1]))


def vocab_child(n_terms, host_exe):
    import vectorchord_bm25_amd as vb
    t0 = time.perf_counter()
    keys = vocabulary(vb, n_terms)
    n_docs = 1000
    post_doc = (np.arange(n_terms) % n_docs).astype(np.uint32)
    dseg = vb.DeviceSegment.build(1.2, 0.75, np.bincount(post_doc, minlength=n_docs).astype(np.uint32), np.zeros((n_docs, 3), np.uint16),
                                  keys.reshape(-1), np.arange(n_terms + 1, dtype=np.uint64), post_doc, np.ones(n_terms, np.uint32))
    gix = vb.GpuIndex(dseg)
    rng = np.random.default_rng(n_terms)
    shapes = {"1024x5": np.full(NQ, 5), "1024x2..8": rng.integers(2, 9, NQ)}
    cases = [(f"{sname}_hashed{int(h * 100)}", make_case(vb, n_terms, rng, lens, h)) for sname, lens in shapes.items() for h in (0.0, 0.05, 1.0)]
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as fh:
        fh.write(np.uint32(n_terms).tobytes() + keys.tobytes() + SEED + np.uint32(len(cases)).tobytes())
        for _, c in cases:
            fh.write(np.uint32(NQ).tobytes() + np.uint32(len(c["lex_off"]) - 1).tobytes() + np.uint64(c["lex_off"][-1]).tobytes())
            fh.write(c["q_lex"].tobytes() + c["lex_off"].tobytes() + c["data"].tobytes() + c["keys"].tobytes())
        path = fh.name
    setup_s = time.perf_counter() - t0
    try:
        host = [json.loads(l) for l in subprocess.run([host_exe, path], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout.splitlines()]
    finally:
        os.unlink(path)
    rows = {}
    for (name, c), h in zip(cases, host):
        row = {"lexemes": len(c["lex_off"]) - 1, "lexeme_bytes": int(c["lex_off"][-1]), "term_ids": h["n_ids"],
               "host_keys_ms": h["keys_ms"], "host_lexemes_ms": h["lexemes_ms"], "host_intern_only_ms": h["intern_only_ms"]}
        for entry in ("keys", "lexemes"):
            d = device_side(vb, gix, c, entry)
            assert d.pop("checksum") == h["checksum"] and d.pop("n_ids") == h["n_ids"], f"{name} {entry}: the device's ids differ from the host's"
            row["device_" + entry] = d
        rows[name] = row
    r = vb.Resolver(gix, 3, NQ, 8 * NQ, 64 * NQ, seed=SEED)
    print("RESULT " + json.dumps({"n_terms": n_terms, "setup_s": round(setup_s, 1), "resolver_device_bytes": r.device_bytes, "cases": rows}))


def c3_child():
    import vectorchord_bm25_amd as vb
    from bench import WORKLOADS
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C3"]
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    rng = np.random.default_rng(1)
    toks = np.stack([rng.choice(vocab, nterms, replace=False) for _ in range(nq)]).astype(np.uint32)
    terms = np.sort(dseg.token_terms(toks.reshape(-1)).reshape(nq, nterms), axis=1).reshape(-1)
    assert (terms != 0xFFFFFFFF).all()
    off = (np.arange(nq + 1) * nterms).astype(np.uint32)
    packed = vb.pack_lexemes([[b"%d" % t for t in row] for row in toks])  # (the synthetic vocabulary's lexemes: decimal strings)
    res = vb.Resolver(gix, 2, nq, nq * nterms, int(packed[1][-1]))
    res.submit(packed)
    ids, q_off = res.collect()
    assert np.array_equal(ids, terms) and np.array_equal(q_off, off)
    st = vb.Stream(gix, 3, nq, nq * nterms, k)
    out = (np.zeros((nq, k), dtype=vb.HIT_DTYPE), np.zeros(nq, dtype=np.uint32))

    def ids_ring(n):
        for _ in range(3):
            st.submit(terms, off)
        for _ in range(n - 3):
            st.collect(out)
            st.submit(terms, off)
        for _ in range(3):
            st.collect(out)

    def lexeme_ring(n):  # batch i + 1 (and i + 2) resolve while batch i scans
        res.submit(packed)
        res.submit(packed)
        for i in range(n):
            a, b = res.collect()
            if i + 2 < n:
                res.submit(packed)
            if st.in_flight == 3:
                st.collect(out)
            st.submit(a, b)
        while st.in_flight:
            st.collect(out)
    row = {}
    for name, fn in (("ids_to_stream", ids_ring), ("lexemes_to_resolver_to_stream", lexeme_ring)):
        fn(WARMUP + 3)
        ref = (out[0].copy(), out[1].copy())
        qps = []
        for _ in range(5):
            t = time.perf_counter()
            fn(RING_STEPS)
            qps.append(nq * RING_STEPS / (time.perf_counter() - t))
        row[name] = {"queries_per_s": {"median": round(statistics.median(qps)), "min": round(min(qps)), "max": round(max(qps))},
                     "step_ms": round(nq / statistics.median(qps) * 1e3, 4)}
        row.setdefault("_ref", ref)
        assert np.array_equal(out[1], row["_ref"][1]) and np.array_equal(out[0]["doc_id"], row["_ref"][0]["doc_id"])
    row.pop("_ref")
    row["lexemes_over_ids"] = round(row["lexemes_to_resolver_to_stream"]["queries_per_s"]["median"] / row["ids_to_stream"]["queries_per_s"]["median"], 3)
    print("RESULT " + json.dumps(dict(row, workload="C3", nq=nq, terms_per_query=nterms, k=k, steps=RING_STEPS)))


def run_child(args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), *args], check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--vocab", default="30000,1000000,8000000")
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--vocab-child", type=int)
    ap.add_argument("--host-exe")
    ap.add_argument("--c3-child", action="store_true")
    a = ap.parse_args()
    if a.vocab_child:
        return vocab_child(a.vocab_child, a.host_exe)
    if a.c3_child:
        return c3_child()
    csrc = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
    exe = os.path.join(tempfile.mkdtemp(), "resolve_host_cost")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "resolve_host_cost.cpp"), "-L" + csrc, "-lvbm25",
                           "-Wl,-rpath," + csrc, "-o", exe])
    res = {"warmup": WARMUP, "reps": REPS, "ring_steps": RING_STEPS, "queries_per_batch": NQ, "unit": "ms unless named",
           "prefix_directory": "not built, not measured: lookup_lane is the plain bisection", "vocabularies": [], "c3_end_to_end": None}

    def save():  # (after every step: a job that is cut short keeps what it has)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")
    for v in a.vocab.split(","):
        res["vocabularies"].append(run_child(["--vocab-child", v, "--host-exe", exe]))
        save()
    if not a.skip_c3:
        res["c3_end_to_end"] = run_child(["--c3-child"])
        save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
