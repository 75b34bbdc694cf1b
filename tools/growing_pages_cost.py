#!/usr/bin/env python3
"""growing_pages_cost.py -- what it costs to get a relation's growing segment (its vectors tape) into HBM as a device growing
segment of C3's index (10 M documents, 30 k vocabulary), by the two routes:
  host    vbm25_growing_from_pages (the host touches every tuple and element) + vbm25_growing_upload (key check on the host, the
          CSR over the link, the inverted form built on the device)
  device  vbm25_device_growing_from_pages (the host follows the page chain, pinned staging, kernels classify / scan / copy / check,
          the same device build behind them), without and with the CSR copied back
at 100 000 and 1 000 000 growing documents of 5 to 40 elements (keys of C3's vocabulary, ascending; a draw's duplicates dropped).
The tape is written here with numpy in the reference's page layout, one _2 and one _0 per document, behind a Meta and a Jump page;
every route reads it through the same C callback (compiled here with g++: no Python in the loop).  Wall time per route ends in a
device synchronise; the routes alternate in one process, one warm-up and five repetitions each; median and spread (min, max).
Also the device reader's kernel time between HIP events and its bytes over the host link in both directions.
Prints one JSON object (and writes it to argv[1] when given; argv[2]: comma-separated document counts instead)."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vectorchord_bm25_amd as vb  # noqa: E402
from bench import WORKLOADS  # noqa: E402

REPS = 5
SIZES = (100_000, 1_000_000)
NONE = 0xFFFFFFFF

READER_C = """
#include <stdint.h>
struct images { const uint8_t *base; uint32_t n; };
const uint8_t *image_page(void *ctx, uint32_t id) {
    const struct images *im = (const struct images *)ctx;
    return id < im->n ? im->base + (uint64_t)8192 * id : 0;
}
"""


class Images(C.Structure):
    _fields_ = [("base", C.c_void_p), ("n", C.c_uint32)]


def page_reader(tmp):
    src, so = os.path.join(tmp, "image_page.c"), os.path.join(tmp, "image_page.so")
    open(src, "w").write(READER_C)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", src, "-o", so])
    return C.cast(C.CDLL(so).image_page, C.c_void_p)


def stats():
    f = vb.lib().vbm25_debug_growing_pages_stats
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    out = np.zeros(4, np.float64)
    f(out.ctypes.data_as(C.c_void_p))
    return out


def make_documents(term_key, n_grow, seed):
    rng = np.random.default_rng(seed)
    n_terms = len(term_key)
    lens = rng.integers(5, 41, n_grow)
    doc = np.repeat(np.arange(n_grow, dtype=np.int64), lens)
    code = np.unique(doc * n_terms + rng.integers(0, n_terms, len(doc)))   # (term_key is in key order: ascending ids are ascending keys)
    d, t = code // n_terms, code % n_terms
    start = np.r_[0, np.cumsum(np.bincount(d, minlength=n_grow))].astype(np.int64)
    return dict(start=start, key=term_key[t], tf=rng.integers(1, 6, len(t)).astype(np.uint32), fieldnorm=rng.integers(0, 200, n_grow).astype(np.uint8),
                payload=rng.integers(0, 65535, (n_grow, 3)).astype(np.uint32), deleted=(rng.random(n_grow) < 0.1).astype(np.uint32))


def write_relation(g):
    """Meta (page 0), Jump (page 1) and the vectors tape from page 2: per document a _2 (16 bytes) and a _0 (24 + 20 n bytes), as many
    documents per page as fit; a page's tuples lie upwards from its line pointers in slot order.  Returns the images, [pages, 8192]."""
    start = g["start"]
    n, counts = len(start) - 1, np.diff(start)
    rec = 40 + 20 * counts                      # bytes of a document's two tuples
    rec_off = np.r_[0, np.cumsum(rec)]
    stream = np.zeros(rec_off[-1] // 4, np.uint32)
    hdr = np.zeros((n, 10), np.uint32)
    hdr[:, 0], hdr[:, 2] = 2, g["fieldnorm"]
    hdr[:, 6] = g["deleted"] | g["payload"][:, 0] << 16
    hdr[:, 7] = g["payload"][:, 1] | g["payload"][:, 2] << 16
    hdr[:, 8] = 24 | (24 + 20 * counts).astype(np.uint32) << 16
    stream[(rec_off[:-1] // 4)[:, None] + np.arange(10)] = hdr
    el = np.concatenate([np.ascontiguousarray(g["key"]).view(np.uint32).reshape(-1, 4), g["tf"][:, None]], axis=1)
    first = np.repeat(rec_off[:-1] // 4 + 10 - 5 * start[:-1], counts) + 5 * np.arange(len(el))
    for a in range(0, len(el), 1 << 22):
        stream[first[a:a + (1 << 22), None] + np.arange(5)] = el[a:a + (1 << 22)]
    stream = stream.view(np.uint8)
    # pages: 24 bytes of header, two line pointers per document, the tuples, 8 bytes of special area
    need = np.r_[0, np.cumsum(rec + 8)]
    bounds = [0]
    while bounds[-1] < n:
        bounds.append(int(np.searchsorted(need, need[bounds[-1]] + 8160, side="right")) - 1)
    images = np.zeros((len(bounds) + 1, 8192), np.uint8)
    meta = b"vchordbm" + struct.pack("<QddII", 1, 1.2, 0.75, NONE, 1) + bytes(range(32))
    jump = struct.pack("<IIQHHIIIIIIIIII", 2, 0, 0, 2036, 680, 0, NONE, NONE, 0, NONE, NONE, NONE, NONE, NONE, NONE) + bytes(4)
    for page, t in ((0, meta), (1, jump)):
        images[page, 8184 - len(t):8184] = np.frombuffer(t, np.uint8)
        images[page, 24:28] = np.frombuffer(struct.pack("<I", (8184 - len(t)) | 1 << 15 | len(t) << 17), np.uint8)
        images[page, 12:18] = np.frombuffer(struct.pack("<HHH", 28, 8184 - len(t), 8184), np.uint8)
        images[page, 8184:8188] = np.frombuffer(struct.pack("<I", NONE), np.uint8)
    for p in range(len(bounds) - 1):
        i, j = bounds[p], bounds[p + 1]
        at = 24 + 8 * (j - i)
        data = stream[rec_off[i]:rec_off[j]]
        img = images[p + 2]
        img[at:at + len(data)] = data
        off = (at + rec_off[i:j] - rec_off[i]).astype(np.uint32)
        lp = np.stack([off | 1 << 15 | 16 << 17, (off + 16) | 1 << 15 | (24 + 20 * counts[i:j]).astype(np.uint32) << 17], axis=1)
        img[24:at] = lp.astype(np.uint32).reshape(-1).view(np.uint8)
        img[12:18] = np.frombuffer(struct.pack("<HHH", at, at, 8184), np.uint8)
        img[8184:8188] = np.frombuffer(struct.pack("<I", p + 3 if p + 2 < len(bounds) else NONE), np.uint8)
    return images


def main():
    import torch

    L = vb.lib()
    sizes = tuple(int(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else SIZES
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C3"]
    t0 = time.perf_counter()
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    hseg = dseg.download()
    term_key = hseg.arrays()["term_key"].reshape(-1, 16).copy()
    del hseg
    res = {"gpu": torch.cuda.get_device_name(0), "index": f"C3: {n_docs} docs / {len(term_key)} terms", "repetitions": REPS,
           "setup_s": round(time.perf_counter() - t0, 1), "sizes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        read_page = page_reader(tmp)
        for n_grow in sizes:
            t0 = time.perf_counter()
            images = write_relation(make_documents(term_key, n_grow, seed=n_grow))
            ctx = Images(images.ctypes.data, len(images))
            print(f"{n_grow}: {len(images)} pages written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

            def host_route():
                torch.cuda.synchronize()
                t = time.perf_counter()
                h = C.c_void_p()
                vb.api.check(L.vbm25_growing_from_pages(read_page, C.byref(ctx), C.byref(h)))
                t_read = time.perf_counter() - t
                d, out = vb.api.GrowingDesc(), C.c_void_p()
                vb.api.check(L.vbm25_growing_get_desc(h, C.byref(d)))
                vb.api.check(L.vbm25_growing_upload(gix.h, C.byref(d), C.byref(out)))
                torch.cuda.synchronize()
                return time.perf_counter() - t, t_read, out, h

            def device_route(with_csr):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out, csr = C.c_void_p(), C.c_void_p()
                vb.api.check(L.vbm25_device_growing_from_pages(gix.h, read_page, C.byref(ctx), C.byref(out), C.byref(csr) if with_csr else None))
                torch.cuda.synchronize()
                return time.perf_counter() - t, out, csr, stats()

            host_s, host_read_s, dev_s, dev_csr_s, st, st_csr = [], [], [], [], None, None
            for rep in range(REPS + 1):
                th, thr, out, h = host_route()
                L.vbm25_device_growing_free(out)
                L.vbm25_growing_free(h)
                td, out, _, st = device_route(False)
                L.vbm25_device_growing_free(out)
                tc, out, csr, st_csr = device_route(True)
                L.vbm25_device_growing_free(out)
                L.vbm25_growing_free(csr)
                if rep:  # (the first one loads the device code)
                    host_s.append(th), host_read_s.append(thr), dev_s.append(td), dev_csr_s.append(tc)
            # the routes agree: the CSR byte for byte, one small batch record for record
            _, _, out_h, h = host_route()
            _, out_d, csr, _ = device_route(True)
            want, got = vb.api._growing_dict(h), vb.api._growing_dict(csr)
            csr_equal = all(want[name].tobytes() == got[name].tobytes() for name in want)
            gs_h, gs_d = vb.GrowingSegment.__new__(vb.GrowingSegment), vb.GrowingSegment.__new__(vb.GrowingSegment)
            gs_h.h, gs_d.h = out_h, out_d
            rng = np.random.default_rng(0)
            terms = np.sort(np.stack([rng.choice(len(term_key), 4, replace=False) for _ in range(32)]), axis=1).reshape(-1).astype(np.uint32)
            off = (np.arange(33) * 4).astype(np.uint32)
            h0, n0 = vb.search_batch_growing(gix, gs_h, terms, off, 10)
            h1, n1 = vb.search_batch_growing(gix, gs_d, terms, off, 10)
            n_el = int(st[3])
            del gs_h, gs_d
            L.vbm25_growing_free(h)
            L.vbm25_growing_free(csr)

            def summary(x):
                return {"median_s": round(float(np.median(x)), 4), "min_s": round(float(min(x)), 4), "max_s": round(float(max(x)), 4)}
            res["sizes"][str(n_grow)] = {
                "pages": len(images), "tape_bytes": 8192 * (len(images) - 2), "elements": n_el, "csr_bytes": 20 * n_el + 16 * n_grow + 8,
                "host_composition": {**summary(host_s), "reader_median_s": round(float(np.median(host_read_s)), 4),
                                     "host_link_bytes_up": 20 * n_el + 16 * n_grow + 8},
                "device_reader": {**summary(dev_s), "kernels_ms": round(float(st[0]), 3), "host_link_bytes_up": int(st[1]),
                                  "host_link_bytes_down": int(st[2]),
                                  "kernel_bytes": 2 * 20 * n_el, "note": "kernel_bytes: the elements read from the page images and written to the planes"},
                "device_reader_with_csr": {**summary(dev_csr_s), "kernels_ms": round(float(st_csr[0]), 3), "host_link_bytes_up": int(st_csr[1]),
                                           "host_link_bytes_down": int(st_csr[2])},
                "device_over_host": round(float(np.median(dev_s) / np.median(host_s)), 3),
                "device_with_csr_over_host": round(float(np.median(dev_csr_s) / np.median(host_s)), 3),
                "csr_equal": bool(csr_equal), "records_equal": bool(np.array_equal(n0, n1) and h0.tobytes() == h1.tobytes()),
            }
            print(json.dumps(res["sizes"][str(n_grow)]), file=sys.stderr, flush=True)
            del images
    print(json.dumps(res, indent=1), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
