#!/usr/bin/env python3
"""maintain_cost.py -- what VACUUM's compaction on the device costs (vbm25_index_maintain) at C3 (10 M documents, 30 k vocabulary,
about 1 G postings): the time of {0, 1, 10} % deleted sealed documents x {0, 100 k, 1 M} growing documents (tests/growing_data.py, about
60 elements each, 10 % of them deleted), split into the five phases of csrc/maintain.hip (relabel, count, vocabulary, scatter,
encode; the library's per-call phase clock, vbm25_debug_maintain_phases); the bytes the scatter pass moves (the blob and the block
metadata read, 8 bytes per posting written) against 8 TB/s; for nothing deleted and no growing documents the two other routes to the
same segment -- the host route (download, CPU decode, vbm25_segment_build) and vbm25_device_segment_build from host mappings --, the
host route's segment checked byte for byte against the compaction's; and the payoff: kernel_ms of C3's batch with 1 M growing
documents and a filter that deletes 1 / 10 of the sealed documents attached, before and after the compaction (the same queries, looked up by key in the new vocabulary).  Prints one JSON object (and writes it to
argv[1] when given)."""
import ctypes as C
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
from maintain_model import decode_all_np  # noqa: E402

WARMUP, STEPS = 3, 20
HBM_BPS = 8e12
PHASES = ("relabel", "count", "vocabulary", "scatter", "encode")


def phases():
    f = vb.lib().vbm25_debug_maintain_phases
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    out = np.zeros(5, np.float64)
    f(out.ctypes.data_as(C.c_void_p))
    return out


def timed(b):
    for _ in range(WARMUP):
        b.run()
    b.fetch()
    b.set_timing(True)
    for _ in range(STEPS):
        b.run()
    ms, _ = b.kernel_ms()
    b.set_timing(False)
    return ms


def main():
    import torch

    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C3"]
    t0 = time.perf_counter()
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    terms, off = make_queries(dseg, vocab, nq, nterms, seed=1, zipf_s=zipf_s)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    hseg = dseg.download()
    download_s = time.perf_counter() - t1
    a = hseg.arrays()
    term_key = a["term_key"].copy()
    blob_bytes, n_blocks, n_post = int(hseg.desc.blob_bytes), hseg.n_blocks, dseg.n_postings
    res = {"gpu": torch.cuda.get_device_name(0), "workload": f"C3: {n_docs} docs / {vocab} vocab / {n_post} postings / {n_blocks} blocks",
           "setup_s": round(time.perf_counter() - t0, 1), "compaction": {}}
    # the other two routes to the same segment, for the case whose mappings the index itself holds (nothing deleted, no growing
    # documents): (a) the host route -- download, CPU decode (numpy, every block of a width at once), vbm25_segment_build on 16
    # threads; (b) vbm25_device_segment_build from those host mappings (8 B per posting over the host link, then the encode)
    t1 = time.perf_counter()
    docs, tfs, ts = decode_all_np(a, chunk=1 << 18)
    decode_s = time.perf_counter() - t1
    doc_len = np.bincount(docs, minlength=n_docs).astype(np.uint32)  # maintain.rs:344-362: a document's length = its postings
    t1 = time.perf_counter()
    hbuilt = vb.Segment.build(1.2, 0.75, doc_len, a["doc_payload"], term_key, ts, docs, tfs, threads=16)
    host_build_s = time.perf_counter() - t1
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    dbuilt = vb.DeviceSegment.build(1.2, 0.75, doc_len, a["doc_payload"], term_key, ts, docs, tfs)
    torch.cuda.synchronize()
    device_from_host_s = time.perf_counter() - t1
    del dbuilt, docs, tfs, doc_len
    vb.DeviceSegment.maintain(gix, None, None)  # (first call: the device code is loaded)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    compacted = vb.DeviceSegment.maintain(gix, None, None)
    torch.cuda.synchronize()
    compaction_s = time.perf_counter() - t1
    c_seg = compacted.download()  # (kept alive: arrays() are views into it)
    c_arr, h_arr = c_seg.arrays(), hbuilt.arrays()
    same = c_seg.meta() == hbuilt.meta() and all(np.array_equal(c_arr[name].reshape(-1), h_arr[name].reshape(-1)) for name in h_arr)
    res["routes_del0_grow0"] = {"compaction_s": round(compaction_s, 4), "host_route_download_s": round(download_s, 3),
                                "host_route_cpu_decode_s": round(decode_s, 2), "host_route_segment_build_s": round(host_build_s, 2),
                                "host_route_total_s": round(download_s + decode_s + host_build_s, 2),
                                "device_segment_build_from_host_mappings_s": round(device_from_host_s, 3),
                                "host_route_segment_equals_compaction": bool(same)}
    print(f"routes: {res['routes_del0_grow0']}", file=sys.stderr)
    del hseg, a, hbuilt, compacted, c_seg, c_arr, h_arr
    rng = np.random.default_rng(1)
    grow = {0: None}
    for n_grow in (100_000, 1_000_000):
        grow[n_grow], _ = make_growing(term_key, n_grow, seed=n_grow, mean_elems=60)
    dels = {p: (rng.random(n_docs) < p / 100.0) for p in (0, 1, 10)}
    for p, deleted in dels.items():
        for n_grow, G in grow.items():
            best = None
            for _ in range(2):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ds = vb.DeviceSegment.maintain(gix, deleted if p else None, G)
                ms = (time.perf_counter() - t) * 1e3
                ph = phases()
                if best is None or ms < best[0]:
                    best = (ms, ph, ds.n_docs, ds.n_postings)
                del ds
            ms, ph, nd, npost = best
            scatter_bytes = blob_bytes + 16 * n_blocks + 8 * npost
            row = {"total_ms": round(ms, 2), **{f"{n}_ms": round(float(x), 2) for n, x in zip(PHASES, ph)}, "n_docs": nd, "n_postings": npost,
                   "scatter_bytes": scatter_bytes, "scatter_hbm_fraction": round(scatter_bytes / (ph[3] * 1e-3) / HBM_BPS, 3)}
            res["compaction"][f"del{p}_grow{n_grow}"] = row
            print(f"del {p}% grow {n_grow}: {row}", file=sys.stderr)
    # payoff: 1 M growing documents and a filter deleting 1 / 10 of the sealed documents, before and after the compaction
    G = grow[1_000_000]
    deleted = dels[10]
    gs = vb.GrowingSegment(gix, **G)
    f = vb.DocFilter(gix, ~deleted)
    f.set_growing(gs, np.ones(len(G["g_start"]) - 1, bool))
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_queries(terms, off)
    res["payoff"] = {"k": k, "before_plain_kernel_ms": round(timed(b), 4)}
    b.set_growing(gs)
    b.set_filter(f, np.zeros(nq, np.uint32))
    res["payoff"]["before_kernel_ms"] = round(timed(b), 4)
    del b
    ds = vb.DeviceSegment.maintain(gix, deleted, G)
    cix = vb.GpuIndex(ds)
    new_ids = cix.lookup_terms([bytes(term_key[t]) for t in terms])
    q_new = []
    for q in range(nq):  # (a query's terms are ascending in key order in both vocabularies)
        q_new.append(new_ids[off[q]:off[q + 1]])
    b2 = vb.Batch(cix, nq, len(terms), k)
    b2.set_queries(np.concatenate(q_new).astype(np.uint32), off)
    res["payoff"]["after_kernel_ms"] = round(timed(b2), 4)
    res["payoff"]["after_n_docs"] = ds.n_docs
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
