#!/usr/bin/env python3
"""caster_cost.py -- what the Document step costs through a caster (vbm25_caster, the ring that keeps its staging and scratch) beside
the unchanged one-shot vbm25_documents_cast and beside the host program (tools/cast_host_cost.cpp) in the same run.  One job on one
MI355X:
  small   1 024 documents of 5 lexemes, 0 % and 100 % of them on the hash path: the step time through a depth-3 ring (submit i + 2,
          collect i), a depth-1 submit + collect, the one-shot call, each as the host clock around calls that end in a wait for the
          device; the kernels alone (the slot's HIP events: everything behind the upload) under cast_pack 0 / 1 / 2; the host program on
          one thread.
  bulk    --docs documents (default 1 000 000) of log-normal length 100 at 0 %, 5 % and 100 % hashed: chunks of 65 536 through a
          depth-3 ring, every chunk appended with vbm25_documents_extend, then vbm25_device_segment_build_documents; beside the one-shot
          cast + the same build; and the sum of the chunks' kernel times under cast_pack 0 / 1 / 2 beside the one-shot cast's kernels.
  stream  the largest and the median step of a vbm25_stream loop on C3's index (10 M documents generated on the device, 1 024 five-term
          queries, k = 10), 200 steps, three runs: alone, with the one-shot cast of the small batch repeated on a second thread, with a
          depth-3 caster doing the same.
Every device result is checked against the host program's checksum of (start, key, tf, length) before its time is reported: of a
timed loop the last repetition's result, of the small shape's kernel times under a cast_pack setting every repetition's, of the bulk
shapes' the setting's first and last.  --warmup untimed and --reps timed repetitions (5 and 30 by default) for every figure, median /
min / max.  A difference counts as one where it exceeds three times the comparison's own max - min;
`verdicts` says so for the three questions.  Writes one JSON object to the path given first.

  python tools/caster_cost.py profiles/caster_cost.json [--docs 1000000] [--reps 30] [--warmup 5] [--skip-stream]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cast_cost as cc  # noqa: E402  (the corpus, the checksum and the timing helpers of the one-shot tool)

SEED = cc.SEED
CHUNK = 65_536
RING_STEPS = 50  # steps of the ring in one timed repetition of the small shape


def host_program(exe, corpus, threads, warmup, reps):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "corpus.bin")
        cc.write_corpus(path, corpus)
        line = subprocess.run([exe, path, str(threads), str(warmup), str(reps), "0"], check=True, stdout=subprocess.PIPE, text=True, timeout=3000).stdout
    return json.loads(line)


def packed_of(c):
    return (c["data"], c["lex_off"], c["lex_count"], c["doc_lex"])


def kernel_ms(L, caster):
    k = C.c_double()
    L.vbm25_debug_caster_kernel_ms.argtypes = [C.c_void_p, C.c_void_p]
    rc = L.vbm25_debug_caster_kernel_ms(caster.h, C.byref(k))
    if rc:
        raise SystemExit("vbm25_debug_caster_kernel_ms failed")
    return k.value / 1e3


def spread(m):
    return m["max"] - m["min"]


def differs(a, b):
    """a against the comparison b: the medians are further apart than three times b's own max - min"""
    return abs(a["median"] - b["median"]) > 3 * spread(b)


def small_shape(vb, exe, hashed, a):
    corpus = cc.make_corpus(1024, np.full(1024, 5), hashed, seed=2)
    packed, pay = packed_of(corpus), corpus["payload"]
    name = f"1024 x 5, {hashed:.0%} hashed"
    host = host_program(exe, corpus, 1, a.warmup, a.reps)
    want = host["checksum"]
    L = vb.lib()
    L.vbm25_debug_cast_kernel_ms.argtypes = [C.c_void_p]
    res = {"shape": name, "n_docs": 1024, "n_lexemes": len(corpus["lex_count"]), "lexeme_bytes": len(corpus["data"]), "host_1_thread": host}

    def must(h, what):
        got = cc.checksum(h.download())
        if got != want:
            raise SystemExit(f"{name}: {what}: checksum {got} differs from the host's {want}")

    one_kernel = []

    def one_shot():
        h = vb.Documents.cast(packed, pay, seed=SEED)
        k = C.c_double()
        vb._lib.check(L.vbm25_debug_cast_kernel_ms(C.byref(k)))
        one_kernel.append(k.value / 1e3)
        return h

    t, h = cc.timed(one_shot, a.warmup, a.reps)
    must(h, "one-shot")
    res["one_shot_ms"], res["one_shot_kernels_ms"] = t, cc.ms(one_kernel[a.warmup:])
    n_lex, n_bytes = len(corpus["lex_count"]), len(corpus["data"])
    with vb.Caster(0, 1, 1024, n_lex, n_bytes, seed=SEED) as c1:
        def round_trip():
            c1.submit(packed, pay)
            return c1.collect()
        t, h = cc.timed(round_trip, a.warmup, a.reps)
        must(h, "depth 1")
        res["depth_1_submit_collect_ms"] = t
        res["kernels_ms"] = {}
        for pack in (0, 1, 2):
            vb.set_tuning("cast_pack", pack)
            ks = []
            for r in range(a.warmup + a.reps):
                must(round_trip(), f"cast_pack {pack}")
                ks.append(kernel_ms(L, c1))
            res["kernels_ms"][f"cast_pack_{pack}"] = cc.ms(ks[a.warmup:])
        vb.reset_tuning()
        res["caster_device_bytes_depth_1"] = c1.device_bytes()
    with vb.Caster(0, 3, 1024, n_lex, n_bytes, seed=SEED) as c3:
        def ring():
            c3.submit(packed, pay)
            c3.submit(packed, pay)
            for _ in range(RING_STEPS):
                c3.submit(packed, pay)
                h = c3.collect()
            c3.collect()
            last = c3.collect()
            return h, last
        t, (h, last) = cc.timed(ring, a.warmup, a.reps)
        must(h, "depth 3")
        must(last, "depth 3, the last batch")
        # (RING_STEPS + 2 batches a repetition, the two at the ends not overlapped: charged to the steps, so the figure is an upper bound)
        res["depth_3_step_ms"] = {k: round(v / RING_STEPS, 4) for k, v in t.items()}
        res["depth_3_steps_per_repetition"] = RING_STEPS
    return res


def bulk_shape(vb, exe, n_docs, lens, hashed, a):
    corpus = cc.make_corpus(n_docs, lens, hashed, seed=3)
    name = f"{n_docs} x log-normal(100), {hashed:.0%} hashed"
    host = host_program(exe, corpus, 16, 0, 1)  # (for its checksum; the host's times on this shape are profiles/cast_cost.json's)
    want = host["checksum"]
    packed, pay = packed_of(corpus), corpus["payload"]
    doc_lex, lex_off = corpus["doc_lex"], corpus["lex_off"]
    cuts = list(range(0, n_docs, CHUNK)) + [n_docs]
    chunks = []
    for lo, hi in zip(cuts, cuts[1:]):
        e0, e1 = int(doc_lex[lo]), int(doc_lex[hi])
        b0, b1 = int(lex_off[e0]), int(lex_off[e1])
        chunks.append(((corpus["data"][b0:b1], lex_off[e0:e1 + 1] - lex_off[e0], corpus["lex_count"][e0:e1], doc_lex[lo:hi + 1] - doc_lex[lo]), pay[lo:hi]))
    max_lex = max(len(c[0][2]) for c in chunks)
    max_bytes = max(len(c[0][0]) for c in chunks)
    L = vb.lib()
    L.vbm25_debug_cast_kernel_ms.argtypes = [C.c_void_p]
    res = {"shape": name, "n_docs": n_docs, "n_lexemes": len(corpus["lex_count"]), "lexeme_bytes": len(corpus["data"]), "chunk_docs": CHUNK,
           "chunks": len(chunks), "host_16_threads_one_run": host}

    def must(h, what):
        got = cc.checksum(h.download())
        if got != want:
            raise SystemExit(f"{name}: {what}: checksum {got} differs from the host's {want}")

    one_kernel = []

    def one_shot():
        h = vb.Documents.cast(packed, pay, seed=SEED)
        k = C.c_double()
        vb._lib.check(L.vbm25_debug_cast_kernel_ms(C.byref(k)))
        one_kernel.append(k.value / 1e3)
        return h

    def one_shot_build():
        h = one_shot()
        return h, vb.DeviceSegment.from_documents(h, 1.2, 0.75)

    t_cast, h = cc.timed(one_shot, a.warmup, a.reps)
    must(h, "one-shot")
    res["one_shot_cast_ms"], res["one_shot_kernels_ms"] = t_cast, cc.ms(one_kernel[a.warmup:])
    del h
    t, (h, dseg) = cc.timed(one_shot_build, a.warmup, a.reps)
    res["one_shot_cast_and_build_ms"] = t
    n_terms, n_post = dseg.n_terms, dseg.n_postings
    del h, dseg
    print(f"{name}: one-shot done", file=sys.stderr, flush=True)
    with vb.Caster(0, 3, CHUNK, max_lex, max_bytes, seed=SEED) as c:
        kernels = []

        def ring_cast():
            whole = vb.Documents.empty(payload=True)
            pending = 0
            ks = 0.0
            for docs, p in chunks:
                if pending == 3:
                    whole.extend(c.collect())
                    ks += kernel_ms(L, c)
                    pending -= 1
                c.submit(docs, p)
                pending += 1
            while pending:
                whole.extend(c.collect())
                ks += kernel_ms(L, c)
                pending -= 1
            kernels.append(ks)
            return whole

        def ring_build():
            whole = ring_cast()
            return whole, vb.DeviceSegment.from_documents(whole, 1.2, 0.75)

        t_cast, whole = cc.timed(ring_cast, a.warmup, a.reps)
        must(whole, "ring + extend")
        res["ring_cast_extend_ms"] = t_cast
        res["extended_handle_bytes"] = whole.device_bytes()
        del whole
        t, (whole, dseg) = cc.timed(ring_build, a.warmup, a.reps)
        if (dseg.n_terms, dseg.n_postings) != (n_terms, n_post):
            raise SystemExit(f"{name}: the build of the extended handle has {dseg.n_terms} terms, {dseg.n_postings} postings")
        res["ring_cast_extend_and_build_ms"] = t
        del whole, dseg
        res["kernels_sum_ms"] = {}
        for pack in (0, 1, 2):
            vb.set_tuning("cast_pack", pack)
            del kernels[:]
            for r in range(a.warmup + a.reps):
                whole = ring_cast()
                if r in (0, a.warmup + a.reps - 1):  # (the first and the last, as cc.timed's callers check the last: the download and
                    must(whole, f"cast_pack {pack}")  # the checksum of 96 M elements take many times the cast itself)
                del whole
            res["kernels_sum_ms"][f"cast_pack_{pack}"] = cc.ms(kernels[a.warmup:])
        vb.reset_tuning()
        res["caster_device_bytes_depth_3"] = c.device_bytes()
    return res


def stream_beside(vb, a):
    """the largest step of a serving stream: alone, beside the one-shot cast, beside the caster"""
    import bench
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = bench.WORKLOADS["C3"]
    seg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(seg)
    terms, off = bench.make_queries(seg, vocab, nq, nterms, 7, zipf_s)
    corpus = cc.make_corpus(1024, np.full(1024, 5), 0.05, seed=2)
    packed, pay = packed_of(corpus), corpus["payload"]
    st = vb.Stream(gix, 3, nq, len(terms), k)
    steps = 200

    def loop():
        st.submit(terms, off)
        st.submit(terms, off)
        ts = []
        for _ in range(20 + steps):
            t0 = time.perf_counter()
            st.submit(terms, off)
            st.collect()
            ts.append(time.perf_counter() - t0)
        st.collect()
        st.collect()
        return cc.ms(ts[20:])

    def beside(work):
        stop, count, errors = threading.Event(), [0], []

        def run():
            try:
                work(stop, count)
            except BaseException as e:  # noqa: BLE001
                errors.append(repr(e))
        th = threading.Thread(target=run)
        th.start()
        time.sleep(0.2)  # (the neighbour is warm before the timed loop starts)
        out = loop()
        stop.set()
        th.join()
        if errors:
            raise SystemExit(f"the neighbour failed: {errors}")
        out["neighbour_casts"] = count[0]
        return out

    def one_shot(stop, count):
        while not stop.is_set():
            vb.Documents.cast(packed, pay, seed=SEED)
            count[0] += 1

    def ring(stop, count):
        with vb.Caster(0, 3, 1024, len(corpus["lex_count"]), len(corpus["data"]), seed=SEED) as c:
            c.submit(packed, pay)
            c.submit(packed, pay)
            while not stop.is_set():
                c.submit(packed, pay)
                c.collect()
                count[0] += 1

    res = {"index": "C3", "steps": steps, "warmup_steps": 20, "stream_depth": 3}
    res["alone"] = loop()
    res["beside_one_shot_cast"] = beside(one_shot)
    res["beside_caster_ring"] = beside(ring)
    res["alone_again"] = loop()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out", nargs="?")
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--skip-stream", action="store_true")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here is measured anywhere else")
    import vectorchord_bm25_amd as vb
    csrc = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
    exe = os.path.join(tempfile.mkdtemp(), "cast_host_cost")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "cast_host_cost.cpp"), "-L" + csrc, "-lvbm25",
                           "-Wl,-rpath," + csrc, "-o", exe])
    cc.make_corpus.vocab = cc.vocabulary()
    res = {"warmup": a.warmup, "reps": a.reps, "unit": "ms", "vocabulary": cc.VOCAB, "small": [], "bulk": []}

    def save():  # (after every part: a job that is cut short keeps what it has)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    for hashed in (0.0, 1.0):
        res["small"].append(small_shape(vb, exe, hashed, a))
        save()
        print(f"small {hashed} done", file=sys.stderr, flush=True)
    if not a.skip_stream:
        res["stream"] = stream_beside(vb, a)
        save()
        print("stream done", file=sys.stderr, flush=True)
    rng = np.random.default_rng(1)
    lens = np.clip(np.rint(rng.lognormal(np.log(0.8 * 100), 0.6, a.docs)), 8, 2000).astype(np.int64)
    for hashed in (0.0, 0.05, 1.0):
        res["bulk"].append(bulk_shape(vb, exe, a.docs, lens, hashed, a))
        save()
        print(f"bulk {hashed} done", file=sys.stderr, flush=True)
    # the three questions
    v = res["verdicts"] = {"rule": "a difference counts where the medians are further apart than 3 x the comparison's max - min"}
    v["small"] = [{"shape": s["shape"],
                   "depth_3_step_vs_host_1_thread": {"caster": s["depth_3_step_ms"], "host": s["host_1_thread"]["cast_ms"],
                                                     "ratio_host_over_caster": round(s["host_1_thread"]["cast_ms"]["median"] / s["depth_3_step_ms"]["median"], 3),
                                                     "counts": differs(s["depth_3_step_ms"], s["host_1_thread"]["cast_ms"])},
                   "depth_1_vs_one_shot": {"ratio_one_shot_over_caster": round(s["one_shot_ms"]["median"] / s["depth_1_submit_collect_ms"]["median"], 3),
                                           "counts": differs(s["depth_1_submit_collect_ms"], s["one_shot_ms"])}} for s in res["small"]]
    v["bulk"] = [{"shape": b["shape"],
                  "ratio_one_shot_over_ring": round(b["one_shot_cast_and_build_ms"]["median"] / b["ring_cast_extend_and_build_ms"]["median"], 3),
                  "counts": differs(b["ring_cast_extend_and_build_ms"], b["one_shot_cast_and_build_ms"])} for b in res["bulk"]]
    # cast_pack: the fastest on the small shapes, unless slower than 0 on a bulk shape by more than that shape's spread
    def small_total(pack):
        return sum(s["kernels_ms"][f"cast_pack_{pack}"]["median"] for s in res["small"])

    def bulk_ok(pack):
        return all(b["kernels_sum_ms"][f"cast_pack_{pack}"]["median"] - b["kernels_sum_ms"]["cast_pack_0"]["median"] <= spread(b["kernels_sum_ms"]["cast_pack_0"])
                   for b in res["bulk"])
    order = sorted((0, 1, 2), key=small_total)
    v["cast_pack"] = {"small_kernels_median_sum_ms": {str(p): round(small_total(p), 4) for p in (0, 1, 2)}, "bulk_condition_met": {str(p): bulk_ok(p) for p in (0, 1, 2)},
                      "choice": next(p for p in order if bulk_ok(p))}
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
