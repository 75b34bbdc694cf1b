#!/usr/bin/env python3
"""filter_cost.py -- what a document filter costs (vbm25_batch_set_filter): kernel_ms of C3's batch (10 M documents, 1024 x 5 terms,
top-10) unfiltered, with a filter that keeps every document, and with filters that keep 1/2, 1/10 and 1/300 of them; then C5's
index (50 M documents, Zipf(1), 10 terms, top-100) on a sample of its batch, unfiltered and keeping 1/10.  The filters keep the
documents d with d % m == 1.  A filtered query starts from threshold 0 (no theta0) and its threshold rises only from accepted
documents: the selective filters scan more blocks.  Prints one JSON object (and writes it to argv[1] when given)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vectorchord_bm25_amd as vb  # noqa: E402
from bench import WORKLOADS, make_queries  # noqa: E402

WARMUP, STEPS = 3, 20


def timed(b, runs=STEPS):
    for _ in range(WARMUP):
        b.run()
    b.fetch()
    b.set_timing(True)
    for _ in range(runs):
        b.run()
    ms, n = b.kernel_ms()
    b.set_timing(False)
    hits, n_hits = b.fetch()
    return ms, n, hits, n_hits


def measure(name, nq_sample, moduli):
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS[name]
    nq = min(nq, nq_sample) if nq_sample else nq
    t0 = time.perf_counter()
    seg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(seg)
    terms, off = make_queries(seg, vocab, nq, nterms, seed=1, zipf_s=zipf_s)
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_queries(terms, off)
    out = {"workload": f"{name}: {n_docs} docs / {vocab} vocab / {nq} x {nterms}-term / top-{k}", "route": b.debug_route(),
           "setup_s": round(time.perf_counter() - t0, 1), "kernel_ms": {}, "mean_hits": {}}
    ms, n, plain, n_plain = timed(b)
    out["kernel_ms"]["unfiltered"] = round(ms, 4)
    out["mean_hits"]["unfiltered"] = float(n_plain.mean())
    ids = np.arange(n_docs, dtype=np.int64)
    sel = np.zeros(nq, dtype=np.uint32)
    for m in moduli:
        label = "keep_all" if m == 1 else f"keep_1/{m}"
        keep = np.ones(n_docs, dtype=bool) if m == 1 else ids % m == 1
        f = vb.DocFilter(gix, keep)
        del keep
        b.set_filter(f, sel)
        ms, n, hits, n_hits = timed(b)
        if m == 1:  # (a filter that keeps everything: the unfiltered records, byte for byte)
            assert hits.tobytes() == plain.tobytes() and np.array_equal(n_hits, n_plain), "keep-all differs from unfiltered"
        else:
            assert all(np.all(hits[q, :n_hits[q]]["doc_id"] % m == 1) for q in range(nq)), f"{label}: a rejected document came back"
        out["kernel_ms"][label] = round(ms, 4)
        out["mean_hits"][label] = float(n_hits.mean())
        b.set_filter(None)
        del f
    return out


def main():
    import torch

    res = {"gpu": torch.cuda.get_device_name(0), "steps": STEPS, "warmup": WARMUP,
           "C3": measure("C3", 0, (1, 2, 10, 300)), "C5_sample": measure("C5", 128, (10,))}
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
