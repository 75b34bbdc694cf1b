#!/usr/bin/env python3
"""growing_filter_cost.py -- what a document filter on the growing segment costs on the device (vbm25_filter_set_growing with a batch
holding filter and segment): kernel_ms of C3's batch (10 M documents, 1024 x 5 terms) at top-10 and top-100 with 100 k and 1 M growing
documents of about 60 elements each (tests/growing_data.py), every query taking bitmap 0.  The sealed bitmap keeps every document, so
the sealed half does the same work in every filtered row and the growing bitmaps are what differ: keep all, a random half, a random
1/100, 1/100 clustered in one contiguous range (the tile skip of growing_scan_kernel), none.

Reported per size and k:
  unfiltered_ms          kernel_ms of the batch with the segment and no filter
  <bitmap>_kernel_ms     kernel_ms with the filter
  <bitmap>_growing_ms    <bitmap>_kernel_ms minus kernel_ms of the same filter without the segment (the sealed half alone)
  <bitmap>_host_ms_per_query  the host composition for the same filter (vbm25_growing_search with the rejected documents marked
                         deleted + vbm25_merge_hits, one thread), whose records are checked against the device's
and at the top kernel_ms of the batch with neither (k*_none) and with the sealed filter alone (k*_sealed_filter).  Prints one JSON
object (and writes it to argv[1] when given)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vectorchord_bm25_amd as vb  # noqa: E402
from bench import WORKLOADS, make_queries  # noqa: E402
from growing_data import make_growing  # noqa: E402

WARMUP, STEPS = 3, 20
SIZES = (100_000, 1_000_000)


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
    return ms, hits, n_hits


def bitmaps(n_grow, seed):
    rng = np.random.default_rng(seed)
    clustered = np.zeros(n_grow, bool)
    lo = n_grow // 3
    clustered[lo:lo + n_grow // 100] = True
    return {"all": np.ones(n_grow, bool), "half": rng.random(n_grow) < 0.5, "1_100_random": rng.random(n_grow) < 0.01,
            "1_100_clustered": clustered, "none": np.zeros(n_grow, bool)}


def main():
    import torch

    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, _ = WORKLOADS["C3"]
    t0 = time.perf_counter()
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    terms, off = make_queries(dseg, vocab, nq, nterms, seed=1, zipf_s=zipf_s)
    hseg = dseg.download()
    term_key = hseg.arrays()["term_key"]
    keys = term_key.reshape(-1, 16)
    sel = np.zeros(nq, np.uint32)
    res = {"gpu": torch.cuda.get_device_name(0), "steps": STEPS, "warmup": WARMUP,
           "workload": f"C3: {n_docs} docs / {vocab} vocab / {nq} x {nterms}-term", "sealed_bitmap": "keep all",
           "setup_s": round(time.perf_counter() - t0, 1), "kernel_ms": {}, "growing": {}}
    f = vb.DocFilter(gix, np.ones(hseg.n_docs, bool))
    batches, sealed = {}, {}
    for k in (10, 100):
        b = vb.Batch(gix, nq, len(terms), k)
        b.set_queries(terms, off)
        res["kernel_ms"][f"k{k}_none"] = round(timed(b)[0], 4)
        b.set_filter(f, sel)
        res["kernel_ms"][f"k{k}_sealed_filter"] = round(timed(b)[0], 4)
        b.set_filter(None)
        batches[k] = b
        sealed[k] = vb.search_batch(gix, terms, off, k)  # (the sealed half of every row: the sealed bitmap keeps all)
    for n_grow in SIZES:
        G, _ = make_growing(term_key, n_grow, seed=n_grow, mean_elems=60)
        gs = vb.GrowingSegment(gix, **G)
        deleted = G["g_deleted"].astype(bool)
        row = {"elements": int(len(G["g_tf"])), "device_bytes": gs.device_bytes}
        maps = bitmaps(n_grow, n_grow + 1)
        for k, b in batches.items():
            b.set_growing(gs)
            row[f"k{k}_unfiltered_ms"] = round(timed(b)[0], 4)
            b.set_growing(None)
            for name, keep in maps.items():
                f.set_growing(gs, keep)
                b.set_growing(gs)
                b.set_filter(f, sel)
                ms, hits, n_hits = timed(b)
                b.set_filter(None)
                b.set_growing(None)
                row[f"k{k}_{name}_kernel_ms"] = round(ms, 4)
                row[f"k{k}_{name}_growing_ms"] = round(ms - res["kernel_ms"][f"k{k}_sealed_filter"], 4)
                # the host composition for a few queries: time per query, records equal to the device's
                n_host = 8 if n_grow <= 100_000 else 2
                Gq = dict(G)
                Gq["g_deleted"] = (deleted | ~keep).astype(np.uint8)
                sh, snh = sealed[k]
                t2 = time.perf_counter()
                for q in range(n_host):
                    query = vb.Query([keys[r].tobytes() for r in terms[off[q]:off[q + 1]]])
                    want = vb.merge_hits(sh[q, :snh[q]], vb.growing_search(hseg, query, k, **Gq), k)
                    assert n_hits[q] == len(want) and hits[q, :n_hits[q]].tobytes() == want.tobytes(), f"{n_grow} k={k} {name} q{q}"
                row[f"k{k}_{name}_host_ms_per_query"] = round((time.perf_counter() - t2) * 1e3 / n_host, 2)
                row[f"k{k}_{name}_growing_hits"] = int(sum(int((hits[q, :n_hits[q]]["doc_id"] > 0xFFFFFFFF - n_grow).sum())
                                                           for q in range(nq)))
        f.set_growing(None)
        res["growing"][str(n_grow)] = row
        del gs
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
