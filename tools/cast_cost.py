#!/usr/bin/env python3
"""cast_cost.py -- what the Document step (tsvector lexemes -> cast documents) and its two consumers cost on the host and on the
device.  One job on one MI355X:
  host      the path without the device cast: per document a vbm25_intern loop, std::sort by key and a saturating merge, on 1 and on 16
            threads, timed inside a small C++ program (tools/cast_host_cost.cpp, built here), so no ctypes overhead is charged to it.
            For the build: that cast + a host vocabulary (sort and unique of all keys, ranks by bisection) +
            vbm25_segment_build_device_unsorted.
  device    vbm25_documents_cast end to end (staging and upload included, prepacked arrays, timed from Python around the ctypes call),
            its kernels alone (HIP events), vbm25_device_segment_build_documents on the cast handle, and
            vbm25_device_growing_append_documents for deltas of 1, 1 000 and 100 000 documents beside vbm25_device_growing_append on
            the downloaded arrays (each repetition on a fresh empty growing segment).
  shapes    --docs documents (default 1 000 000) with log-normal lengths of mean 100 (len_mode 1's law) over 30 000 lexemes, 0 %, 5 %
            and 100 % of them on the hash path; and 1 024 documents of 5 lexemes, the small-batch latency.
Every device result is checked against the host program's checksum of (start, key, tf, length) before its time is reported.  Host
clock around synchronous calls, --warmup untimed and --reps timed repetitions (5 and 30 by default; --host-reps and --host-reps-1t for
the host program on 16 threads and on one, whose single-thread runs of the large shape take 6 to 15 seconds each), median / min / max.  Writes one JSON object to the path given first.

  python tools/cast_cost.py profiles/cast_cost.json [--docs 1000000] [--reps 30] [--warmup 5] [--host-reps 30] [--host-reps-1t 30]"""
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

SEED = bytes(range(32))
VOCAB = 30_000
WIDTH = 24


def ms(ts):
    return {"median": round(statistics.median(ts) * 1e3, 4), "min": round(min(ts) * 1e3, 4), "max": round(max(ts) * 1e3, 4)}


def vocabulary():
    """lexeme i of the padded kind (a decimal string) and of the hashed kind (24 bytes), as rows of WIDTH bytes and their lengths"""
    short = np.zeros((VOCAB, WIDTH), dtype=np.uint8)
    long_ = np.zeros((VOCAB, WIDTH), dtype=np.uint8)
    s_len = np.zeros(VOCAB, dtype=np.int64)
    for i in range(VOCAB):
        a, b = b"%d" % i, b"hashed-lexeme-%010d" % i
        short[i, :len(a)] = np.frombuffer(a, dtype=np.uint8)
        long_[i] = np.frombuffer(b, dtype=np.uint8)
        s_len[i] = len(a)
    return short, s_len, long_


def make_corpus(n_docs, lens, hashed, seed):
    """prepacked documents: lens lexemes a document drawn uniformly from the vocabulary, `hashed` of them from its hashed kind"""
    rng = np.random.default_rng(seed)
    short, s_len, long_ = make_corpus.vocab
    doc_lex = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    n_lex = int(doc_lex[-1])
    parts, lex_len = [], np.zeros(n_lex, dtype=np.int64)
    col = np.arange(WIDTH)
    for a in range(0, n_lex, 4_000_000):  # (in pieces: the padded rows are 24 bytes a lexeme)
        b = min(n_lex, a + 4_000_000)
        pick = rng.integers(0, VOCAB, b - a)
        is_long = rng.random(b - a) < hashed
        ln = np.where(is_long, WIDTH, s_len[pick])
        rows = np.where(is_long[:, None], long_[pick], short[pick])
        parts.append(rows[col[None, :] < ln[:, None]])
        lex_len[a:b] = ln
    data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    lex_off = np.concatenate([[0], np.cumsum(lex_len)]).astype(np.uint64)
    lex_count = rng.integers(1, 4, n_lex).astype(np.uint32)
    payload = rng.integers(0, 65535, (n_docs, 3)).astype(np.uint16)
    return dict(data=np.ascontiguousarray(data), lex_off=lex_off, lex_count=lex_count, doc_lex=doc_lex, payload=payload)


def write_corpus(path, c):
    with open(path, "wb") as f:
        np.array([len(c["doc_lex"]) - 1, len(c["lex_count"]), len(c["data"])], dtype=np.uint64).tofile(f)
        f.write(SEED)
        for name in ("doc_lex", "lex_off", "lex_count", "payload", "data"):
            c[name].tofile(f)


def checksum(d):
    """tools/cast_host_cost.cpp's checksum of a downloaded cast, in wrapping 64-bit arithmetic"""
    u = np.uint64
    with np.errstate(over="ignore"):
        start, tf, length = d["g_start"].astype(u), d["g_tf"].astype(u), d["length"].astype(u)
        key = np.ascontiguousarray(d["g_key"]).view("<u8").reshape(-1, 2)
        e = np.arange(len(tf), dtype=u)
        h = (start * (np.arange(len(start), dtype=u) + u(1))).sum(dtype=u)
        h += ((key[:, 0] ^ (key[:, 1] * u(3))) * (u(2) * e + u(1)) + tf * (e + u(5))).sum(dtype=u)
        h += (length * (np.arange(len(length), dtype=u) + u(7))).sum(dtype=u)
    return f"{int(h):016x}"


def timed(fn, warmup, reps):
    ts = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if r >= warmup:
            ts.append(t1 - t0)
    return ms(ts), out


def run_shape(vb, host_exe, name, corpus, a, with_build, deltas):
    res = {"shape": name, "n_docs": len(corpus["doc_lex"]) - 1, "n_lexemes": len(corpus["lex_count"]), "lexeme_bytes": len(corpus["data"])}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "corpus.bin")
        write_corpus(path, corpus)
        res["host"] = []
        for threads, reps in ((1, a.host_reps_1t), (16, a.host_reps)):
            warm = a.warmup if reps >= a.reps else 1  # (a shortened host run: one untimed repetition)
            line = subprocess.run([host_exe, path, str(threads), str(warm), str(reps), str(min(3, reps) if with_build else 0)],
                                  check=True, stdout=subprocess.PIPE, text=True, timeout=3000).stdout
            res["host"].append(dict(json.loads(line), warmup=warm))
            print(f"{name}: host, {threads} thread(s) done", file=sys.stderr, flush=True)
    packed = (corpus["data"], corpus["lex_off"], corpus["lex_count"], corpus["doc_lex"])
    L = vb.lib()
    L.vbm25_debug_cast_kernel_ms.argtypes = [C.c_void_p]
    kernel = []

    def cast():
        h = vb.Documents.cast(packed, corpus["payload"], seed=SEED)
        k = C.c_double()
        vb._lib.check(L.vbm25_debug_cast_kernel_ms(C.byref(k)))
        kernel.append(k.value / 1e3)
        return h

    t_cast, h = timed(cast, a.warmup, a.reps)
    print(f"{name}: device cast done", file=sys.stderr, flush=True)
    got = checksum(h.download())
    if got != res["host"][0]["checksum"] or got != res["host"][1]["checksum"]:
        raise SystemExit(f"{name}: the device cast's checksum {got} differs from the host's {res['host'][0]['checksum']}")
    upload_bytes = 4 * len(corpus["doc_lex"]) * 2 + 8 * len(corpus["lex_off"]) + 4 * len(corpus["lex_count"]) + len(corpus["data"]) + corpus["payload"].nbytes
    res["device"] = {"cast_end_to_end_ms": t_cast, "cast_kernels_ms": ms(kernel[a.warmup:]), "checksum": got, "n_elements": h.n_elements,
                     "upload_bytes": upload_bytes, "handle_bytes": h.device_bytes()}
    if with_build:
        t_build, dseg = timed(lambda: vb.DeviceSegment.from_documents(h, 1.2, 0.75), a.warmup, a.reps)
        if dseg.n_terms != res["host"][1]["n_terms"] or dseg.n_postings != h.n_elements:
            raise SystemExit(f"{name}: the device build has {dseg.n_terms} terms, {dseg.n_postings} postings")
        res["device"]["from_documents_ms"] = t_build
        res["device"]["n_terms"] = dseg.n_terms
        gix = vb.GpuIndex(dseg)
        empty = dict(g_start=np.zeros(1, np.uint64), g_key=np.zeros(0, np.uint8), g_tf=np.zeros(0, np.uint32), g_fieldnorm=np.zeros(0, np.uint8),
                     g_payload=np.zeros((0, 3), np.uint16))
        res["device"]["append"] = []
        for n in deltas:
            n = min(n, res["n_docs"])
            e = int(corpus["doc_lex"][n])
            sub = (corpus["data"][:int(corpus["lex_off"][e])], corpus["lex_off"][:e + 1], corpus["lex_count"][:e], corpus["doc_lex"][:n + 1])
            hd = vb.Documents.cast(sub, corpus["payload"][:n], seed=SEED)
            arr = hd.download()
            t_docs, t_host = [], []
            for r in range(a.warmup + a.reps):
                g1, g2 = vb.GrowingSegment(gix, **empty), vb.GrowingSegment(gix, **empty)
                t0 = time.perf_counter()
                g1.append_documents(hd)
                t1 = time.perf_counter()
                g2.append(arr["g_start"], arr["g_key"], arr["g_tf"], arr["g_fieldnorm"], arr["g_payload"])
                t2 = time.perf_counter()
                if g1.n_docs != n or g2.n_docs != n or g1.device_bytes != g2.device_bytes:
                    raise SystemExit(f"{name}: the two appends of {n} documents differ")
                if r >= a.warmup:
                    t_docs.append(t1 - t0)
                    t_host.append(t2 - t1)
            res["device"]["append"].append({"delta_docs": n, "delta_elements": hd.n_elements, "append_documents_ms": ms(t_docs),
                                            "append_host_arrays_ms": ms(t_host)})
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out", nargs="?")
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--host-reps", type=int, default=30)
    p.add_argument("--host-reps-1t", type=int, default=30)
    a = p.parse_args()
    import vectorchord_bm25_amd as vb
    csrc = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
    host_exe = os.path.join(tempfile.mkdtemp(), "cast_host_cost")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "cast_host_cost.cpp"), "-L" + csrc, "-lvbm25",
                           "-Wl,-rpath," + csrc, "-o", host_exe])
    make_corpus.vocab = vocabulary()
    res = {"warmup": a.warmup, "reps": a.reps, "host_reps": a.host_reps, "host_reps_1_thread": a.host_reps_1t, "unit": "ms", "vocabulary": VOCAB, "shapes": []}

    def save():  # (after every shape: a job that is cut short keeps what it has)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    rng = np.random.default_rng(1)
    small = make_corpus(1024, np.full(1024, 5), 0.05, seed=2)
    res["shapes"].append(run_shape(vb, host_exe, "1024 x 5, 5 % hashed", small, a, False, ()))
    save()
    lens = np.clip(np.rint(rng.lognormal(np.log(0.8 * 100), 0.6, a.docs)), 8, 2000).astype(np.int64)
    for hashed in (0.0, 0.05, 1.0):
        corpus = make_corpus(a.docs, lens, hashed, seed=3)
        res["shapes"].append(run_shape(vb, host_exe, f"{a.docs} x log-normal(100), {hashed:.0%} hashed", corpus, a, hashed == 0.05, (1, 1000, 100_000)))
        save()
        del corpus
    print(json.dumps(res))


if __name__ == "__main__":
    main()
