#!/usr/bin/env python3
"""pages_device_cost.py -- what it costs to get a PostgreSQL bm25 index relation into HBM as a searchable index, by the two routes:
  host    vbm25_segment_from_pages (single-threaded walk, a host copy of the index) + vbm25_index_create (upload of that copy)
  device  vbm25_device_segment_from_pages (host follows the page chains, pinned staging, kernels flatten) + vbm25_index_create_from_device
at relations of 100 k and 1 M documents (30 k vocabulary, lognormal lengths, mean 100) written by the oracle's page writer
(tests/orc.py: Pages).  Both routes read the pages through the same C callback (the writer's page accessor: no Python in the loop).
Wall time per route ends in a device synchronise; the routes alternate in one process, one warm-up and five repetitions each; median
and spread (min, max).  Also: bytes over the host link, host memory the library allocates for the index, and the device reader's
kernel time from HIP events.  Prints one JSON object (and writes it to argv[1] when given; argv[2]: comma-separated document counts
instead of 100 k and 1 M -- a 10 M relation is 2 GB of pages and wants about 12 GB of host memory beside them)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orc  # noqa: E402
import vectorchord_bm25_amd as vb  # noqa: E402

REPS = 5
SIZES = (100_000, 1_000_000)


def stats():
    f = vb.lib().vbm25_debug_pages_device_stats
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    out = np.zeros(4, np.float64)
    f(out.ctypes.data_as(C.c_void_p))
    return out


def main():
    import torch

    L = vb.lib()
    read_page = C.cast(orc.lib().orc_pages_get, C.c_void_p)  # const uint8_t *(void *pages, uint32_t id): a vbm25_read_page_fn
    sizes = tuple(int(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else SIZES
    res = {"gpu": torch.cuda.get_device_name(0), "repetitions": REPS, "sizes": {}}
    if 10_000_000 not in sizes:
        res["10000000_docs"] = "not measured"
    for n_docs in sizes:
        print(f"{n_docs}: corpus", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        seg = vb.Segment.synth(n_docs, 30_000, mean_len=100, len_mode=1, seed=20260925, threads=16)
        print(f"{n_docs}: relation", file=sys.stderr, flush=True)
        oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
        pages = orc.Pages(oix, seed=bytes(range(32)))
        n_pages = len(pages)
        index_bytes = int(sum(a.nbytes for a in seg.arrays().values()))
        setup_s = time.perf_counter() - t0
        print(f"{n_docs}: {n_pages} pages, set up in {setup_s:.1f} s", file=sys.stderr, flush=True)

        def host_route():
            torch.cuda.synchronize()
            t = time.perf_counter()
            h = C.c_void_p()
            vb.api.check(L.vbm25_segment_from_pages(read_page, pages.h, C.byref(h)))
            t_read = time.perf_counter() - t
            s = vb.Segment(h)
            ix = vb.GpuIndex(s)
            torch.cuda.synchronize()
            return time.perf_counter() - t, t_read, ix

        def device_route():
            torch.cuda.synchronize()
            t = time.perf_counter()
            h = C.c_void_p()
            vb.api.check(L.vbm25_device_segment_from_pages(read_page, pages.h, 0, C.byref(h)))
            torch.cuda.synchronize()
            t_read = time.perf_counter() - t
            st = stats()
            ix = vb.GpuIndex(vb.DeviceSegment(h))
            torch.cuda.synchronize()
            return time.perf_counter() - t, t_read, ix, st

        host_s, host_read_s, dev_s, dev_read_s, st = [], [], [], [], None
        for rep in range(REPS + 1):
            print(f"{n_docs}: repetition {rep}", file=sys.stderr, flush=True)
            th, thr, ixh = host_route()
            del ixh
            td, tdr, ixd, st = device_route()
            del ixd
            if rep:  # (the first one loads the device code)
                host_s.append(th), host_read_s.append(thr), dev_s.append(td), dev_read_s.append(tdr)
        # the two routes' indexes answer alike (one small batch)
        _, _, ixh = host_route()
        _, _, ixd, _ = device_route()
        rng = np.random.default_rng(0)
        terms = np.sort(np.stack([rng.choice(seg.n_terms, 4, replace=False) for _ in range(32)]), axis=1).reshape(-1).astype(np.uint32)
        off = (np.arange(33) * 4).astype(np.uint32)
        h0, n0 = vb.search_batch(ixh, terms, off, 10)
        h1, n1 = vb.search_batch(ixd, terms, off, 10)
        del ixh, ixd

        def summary(x):
            return {"median_s": round(float(np.median(x)), 4), "min_s": round(float(min(x)), 4), "max_s": round(float(max(x)), 4)}
        res["sizes"][str(n_docs)] = {
            "pages": n_pages, "relation_bytes": 8192 * n_pages, "index_bytes": index_bytes, "setup_s": round(setup_s, 1),
            "host_route": {**summary(host_s), "reader_median_s": round(float(np.median(host_read_s)), 4),
                           "host_link_bytes": index_bytes,
                           "host_memory_for_the_index_bytes": index_bytes,
                           "note": "the flattened arrays (vectors grown by push_back hold up to twice that while they grow), uploaded from pageable memory"},
            "device_route": {**summary(dev_s), "reader_median_s": round(float(np.median(dev_read_s)), 4),
                             "kernels_ms": round(float(st[0]), 3), "host_link_bytes": int(st[1] + st[2]),
                             "host_memory_bytes": int(st[3]),
                             "note": "16 MiB of pinned staging, 8 bytes per page, and the segment's host members (keys, df, first blocks, bytes per token)"},
            "device_over_host": round(float(np.median(dev_s) / np.median(host_s)), 3),
            "records_equal": bool(np.array_equal(n0, n1) and h0.tobytes() == h1.tobytes()),
        }
        print(json.dumps(res["sizes"][str(n_docs)]), file=sys.stderr, flush=True)
        del pages, oix, seg
    print(json.dumps(res, indent=1), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
