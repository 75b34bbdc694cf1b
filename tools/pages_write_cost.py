#!/usr/bin/env python3
"""pages_write_cost.py -- what writing a device segment out as the reference's index pages costs (vbm25_device_segment_write_relation)
at C3 (10 M documents, 30 k vocabulary, about 1 G postings): the wall time of the whole call with a callback that does nothing and
with one that copies every image into host memory (both compiled C, so the time is the library's and not an interpreter's), split
by the library's HIP events into layout kernels, fill kernels and copies to the host (vbm25_debug_pages_write_stats); beside it
vbm25_device_segment_download of the same segment, the only other way out of HBM, which moves bytes of the same order.  The written
relation is read back by the device reader and compared with the segment's download.  Prints one JSON object (and writes it to
argv[1] when given)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vectorchord_bm25_amd as vb  # noqa: E402
from bench import WORKLOADS  # noqa: E402

CALLBACKS = r"""
#include <stdint.h>
#include <string.h>
struct dst { uint8_t *base; uint64_t n_pages; };
int noop_page(void *ctx, uint32_t id, const uint8_t *image) { (void)ctx; (void)id; (void)image; return 0; }
int copy_page(void *ctx, uint32_t id, const uint8_t *image) {
    struct dst *d = (struct dst *)ctx;
    if (id >= d->n_pages) return 1;
    memcpy(d->base + (uint64_t)id * 8192, image, 8192);
    return 0;
}
"""


class Dst(C.Structure):
    _fields_ = [("base", C.c_void_p), ("n_pages", C.c_uint64)]


def stats():
    f = vb.lib().vbm25_debug_pages_write_stats
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    out = np.zeros(6, np.float64)
    f(out.ctypes.data_as(C.c_void_p))
    return out


def main():
    import torch

    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C3"]
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "cb.c"), "w") as fh:
            fh.write(CALLBACKS)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(tmp, "cb.c"), "-o", os.path.join(tmp, "cb.so")])
        cb = C.CDLL(os.path.join(tmp, "cb.so"))
    L = vb.lib()
    torch.cuda.synchronize()
    t = time.perf_counter()
    flush_pages = dseg.page_count()
    page_count_ms = (time.perf_counter() - t) * 1e3
    n_pages = flush_pages + 4
    image = np.empty(n_pages * 8192, np.uint8)
    image.fill(0xa5)   # (touched: the copies below do not pay for page faults)
    dst = Dst(image.ctypes.data, n_pages)
    with open(vb.library_path(), "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"gpu": torch.cuda.get_device_name(0), "libvbm25_sha256_16": sha,
           "workload": f"C3: {n_docs} docs / {dseg.n_terms} terms / {dseg.n_postings} postings / {dseg.n_blocks} blocks",
           "pages": n_pages, "page_bytes": n_pages * 8192, "page_count_ms": round(page_count_ms, 2)}

    def write(fn, ctx):
        best = None
        for _ in range(3):   # (the first call loads the device code)
            n = C.c_uint32()
            torch.cuda.synchronize()
            t = time.perf_counter()
            vb.api.check(L.vbm25_device_segment_write_relation(dseg.h, None, C.cast(fn, C.c_void_p), ctx, C.byref(n)))
            ms = (time.perf_counter() - t) * 1e3
            assert n.value == n_pages
            if best is None or ms < best[0]:
                best = (ms, stats())
        ms, s = best
        return {"total_ms": round(ms, 2), "layout_kernels_ms": round(s[0], 3), "fill_kernels_ms": round(s[1], 3), "copies_ms": round(s[2], 2),
                "bytes_to_host": int(s[3]), "bytes_to_device": int(s[4]), "host_link_GBps": round(s[3] / (s[2] * 1e-3) / 1e9, 2),
                "fill_GBps": round(n_pages * 8192 / (s[1] * 1e-3) / 1e9, 1)}

    res["write_relation_noop_callback"] = write(cb.noop_page, None)
    res["write_relation_memcpy_callback"] = write(cb.copy_page, C.cast(C.pointer(dst), C.c_void_p))
    best = None
    for _ in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        hseg = dseg.download()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None else min(best, ms)
    nbytes = int(sum(a.nbytes for a in hseg.arrays().values()))
    res["download"] = {"total_ms": round(best, 2), "bytes": nbytes, "GBps": round(nbytes / (best * 1e-3) / 1e9, 2)}
    res["write_over_download"] = round(res["write_relation_memcpy_callback"]["total_ms"] / best, 2)
    # the copied relation, read back on the device, is the segment
    pages = image.reshape(n_pages, 8192)
    back = vb.DeviceSegment.from_pages(lambda i: pages[i].ctypes.data if i < n_pages else None).download()
    a, b = back.arrays(), hseg.arrays()
    res["read_back_equals_segment"] = bool(back.meta() == hseg.meta() and all(np.array_equal(a[n].reshape(-1), b[n].reshape(-1)) for n in b))
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
