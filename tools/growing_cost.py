#!/usr/bin/env python3
"""growing_cost.py -- what a growing (unsealed) segment costs on the device (vbm25_batch_set_growing): kernel_ms of C3's batch (10 M
documents, 1024 x 5 terms) at top-10 and top-100 with no growing segment and with 10 k, 100 k and 1 M growing documents of about 60
elements each (tests/growing_data.py: uniform over the sealed keys and 50 keys the sealed segment lacks, 10 % deleted); per size the
upload time and vbm25_device_growing_bytes, the growing part's time (kernel_ms with the segment minus kernel_ms without: the copy of
the sealed records, growing_scan_kernel and growing_merge_kernel) and its fraction of the HBM bound (12 B per growing posting of the
batch's terms over that time, against 8 TB/s); and the host composition's time per query for the same shapes (vbm25_growing_search +
vbm25_merge_hits, one thread: what the shim ran per query before), whose records are checked against the device's.  Prints one JSON
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
SIZES = (10_000, 100_000, 1_000_000)
HBM_BPS = 8e12


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


def main():
    import torch

    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, _ = WORKLOADS["C3"]
    t0 = time.perf_counter()
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    terms, off = make_queries(dseg, vocab, nq, nterms, seed=1, zipf_s=zipf_s)
    hseg = dseg.download()
    term_key = hseg.arrays()["term_key"]
    res = {"gpu": torch.cuda.get_device_name(0), "steps": STEPS, "warmup": WARMUP,
           "workload": f"C3: {n_docs} docs / {vocab} vocab / {nq} x {nterms}-term", "setup_s": round(time.perf_counter() - t0, 1),
           "kernel_ms": {}, "growing": {}}
    batches = {}
    for k in (10, 100):
        b = vb.Batch(gix, nq, len(terms), k)
        b.set_queries(terms, off)
        ms, hits, n_hits = timed(b)
        res["kernel_ms"][f"k{k}_none"] = round(ms, 4)
        batches[k] = b
    for n_grow in SIZES:
        G, g_term = make_growing(term_key, n_grow, seed=n_grow, mean_elems=60)
        t1 = time.perf_counter()
        gs = vb.GrowingSegment(gix, **G)
        up_s = time.perf_counter() - t1
        # growing postings of the batch's terms (live documents, keys the sealed segment holds)
        live = np.repeat(G["g_deleted"] == 0, np.diff(G["g_start"].astype(np.int64)))
        df = np.bincount(g_term[(g_term != 0xFFFFFFFF) & live], minlength=hseg.n_terms)
        postings = int(df[terms].sum())
        row = {"elements": int(len(G["g_tf"])), "upload_s": round(up_s, 3), "device_bytes": gs.device_bytes,
               "batch_postings": postings}
        for k, b in batches.items():
            b.set_growing(gs)
            ms, hits, n_hits = timed(b)
            b.set_growing(None)
            grow_ms = ms - res["kernel_ms"][f"k{k}_none"]
            row[f"k{k}_kernel_ms"] = round(ms, 4)
            row[f"k{k}_growing_ms"] = round(grow_ms, 4)
            row[f"k{k}_hbm_fraction"] = round(12.0 * postings / (grow_ms * 1e-3) / HBM_BPS, 4) if grow_ms > 0 else None
            # the host composition for a few queries of the batch: time per query, records equal to the device's
            n_host = 8 if n_grow <= 100_000 else 2
            sealed, snh = vb.search_batch(gix, terms[:off[n_host]], off[:n_host + 1], k)
            keys = term_key.reshape(-1, 16)
            t2 = time.perf_counter()
            for q in range(n_host):
                query = vb.Query([keys[r].tobytes() for r in terms[off[q]:off[q + 1]]])
                want = vb.merge_hits(sealed[q, :snh[q]], vb.growing_search(hseg, query, k, **G), k)
                assert n_hits[q] == len(want) and hits[q, :n_hits[q]].tobytes() == want.tobytes(), f"n_grow={n_grow} k={k} q{q}"
            row[f"k{k}_host_ms_per_query"] = round((time.perf_counter() - t2) * 1e3 / n_host, 2)
            row[f"k{k}_growing_hits"] = int(sum(int((hits[q, :n_hits[q]]["doc_id"] > 0xFFFFFFFF - n_grow).sum()) for q in range(nq)))
        res["growing"][str(n_grow)] = row
        del gs
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
