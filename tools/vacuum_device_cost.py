#!/usr/bin/env python3
"""vacuum_device_cost.py -- what it costs to get from a relation's pages to VACUUM's compacted segment in HBM, by the two routes:
  old  vbm25_sealed_deleted_from_pages (the host walks every document tuple) + vbm25_device_growing_from_pages(..., csr) (the CSR comes
       down) + vbm25_index_maintain on those host arrays (validated on the host, and up again)
  new  vbm25_device_vacuum_from_pages + vbm25_index_maintain_device (the inputs stay in HBM)
at C3's shape built on the device (10 M documents, 30 k vocabulary): the relation is vbm25_device_segment_write_relation's, with 1 % of
the sealed documents' deleted flags set and a vectors tape of 100 000 inserted documents (tools/growing_pages_cost.py's writer, 10 % of
them deleted) linked in.  Both routes read the pages through the same C callback (no Python in the loop).  Per route: wall time from
the first call to the device synchronise after the compaction (one warm-up and REPS repetitions; median and spread), the bytes over
the host link in each direction (the library's counters), the readers' kernel time and the compaction's five phases.

One route per run (--route old | new | both), so that the old route can be timed on another build of the library (VBM25_LIBRARY: the
parent commit's): the runs share the JSON file argv[1], every route is stored with the hash of the library it ran on, and a run that
finds both compares them -- the two segments' checksums must be equal.  The compaction's bytes are every copy of the call, the
encode's included (vbm25_debug_maintain_link_bytes); the new route asserts from that counter that nothing O(elements) or O(documents)
crosses the link: the index's term keys and the new vocabulary's arrays, O(terms), in both directions."""
import argparse
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np
import torch  # (before the library is loaded: both bring a HIP runtime, and torch's has to be the process's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vectorchord_bm25_amd import _lib  # noqa: E402

NEW_ROUTE = ("vbm25_device_vacuum_from_pages", "vbm25_device_vacuum_info", "vbm25_device_vacuum_read", "vbm25_device_vacuum_free",
             "vbm25_index_maintain_device", "vbm25_filter_remap_device")
# an older build of the library (VBM25_LIBRARY) lacks the new route's entry points: they leave this process's binding table, and the
# run can take the old route only
_raw = C.CDLL(_lib.library_path())
HAS_NEW_ROUTE = all(hasattr(_raw, name) for name in NEW_ROUTE)
if not HAS_NEW_ROUTE:
    for name in NEW_ROUTE:
        _lib.ABI.pop(name, None)

import vectorchord_bm25_amd as vb  # noqa: E402
from bench import WORKLOADS  # noqa: E402
from growing_pages_cost import Images, make_documents, page_reader, write_relation  # noqa: E402
from pages_write_cost import CALLBACKS, Dst  # noqa: E402

REPS = 3
N_GROW = 100_000
SEALED_DELETED = 0.01
PHASES = ("relabel", "count", "vocabulary", "scatter", "encode")
NONE = 0xFFFFFFFF


def debug_doubles(name, n):
    """a vbm25_debug_* counter array of the loaded library; None when this build has no such counter"""
    f = getattr(vb.lib(), name, None)
    if f is None:
        return None
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    out = np.zeros(n, np.float64)
    f(out.ctypes.data_as(C.c_void_p))
    return out


def u32(images, page, at):
    return struct.unpack_from("<I", images[page], at)[0]


def first_tuple(images, page):
    return u32(images, page, 24) & 0x7fff


def build_relation(dseg, term_key, copy_page):
    """the segment's relation as one array [pages, 8192], the flags set, the vectors tape linked in; returns (images, flags)"""
    n_sealed_pages = dseg.page_count() + 4
    tape = write_relation(make_documents(term_key, N_GROW, seed=N_GROW))[2:]   # (without that writer's own Meta and Jump)
    images = np.zeros((n_sealed_pages + len(tape), 8192), np.uint8)
    dst = Dst(images.ctypes.data, n_sealed_pages)
    n = C.c_uint32()
    vb.api.check(vb.lib().vbm25_device_segment_write_relation(dseg.h, None, C.cast(copy_page, C.c_void_p), C.cast(C.pointer(dst), C.c_void_p), C.byref(n)))
    assert n.value == n_sealed_pages
    # the vectors tape behind the sealed relation: its links move with it, Jump.ptr_vectors names its first page
    nxt = tape[:, 8184:8188].view("<u4")
    nxt[nxt != NONE] += n_sealed_pages - 2
    images[n_sealed_pages:] = tape
    ptr_jump = u32(images, 0, first_tuple(images, 0) + 36)
    joff = first_tuple(images, ptr_jump)
    images[ptr_jump, joff:joff + 4] = np.frombuffer(struct.pack("<I", n_sealed_pages), np.uint8)
    # DocumentTuple.deleted of a random 1 %
    flags = np.random.default_rng(1).random(dseg.n_docs) < SEALED_DELETED
    p, d = u32(images, ptr_jump, joff + 44), 0
    while p != NONE:
        k = (struct.unpack_from("<H", images[p], 12)[0] - 24) // 4
        idx = np.flatnonzero(flags[d:d + k])
        if len(idx):
            images[p][(images[p][24:24 + 4 * k].view("<u4") & 0x7fff)[idx]] = 1
        d += k
        p = u32(images, p, 8184)
    assert d == dseg.n_docs
    return images, flags


def segment_crc(ds):
    """CRC-32 over the downloaded segment's arrays in name order"""
    seg = ds.download()
    arrays = seg.arrays()
    crc = zlib.crc32(repr(seg.meta()).encode())
    for name in sorted(arrays):
        crc = zlib.crc32(np.ascontiguousarray(arrays[name]).reshape(-1).view(np.uint8), crc)
    return crc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--route", default="both", choices=("old", "new", "both"))
    args = ap.parse_args()
    routes = ("old", "new") if args.route == "both" else (args.route,)
    if "new" in routes and not HAS_NEW_ROUTE:
        sys.exit("this build of the library has no vbm25_device_vacuum_from_pages: --route old")
    L = vb.lib()
    with open(vb.library_path(), "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()[:16]
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C3"]
    t0 = time.perf_counter()
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    hseg = dseg.download()
    term_key = hseg.arrays()["term_key"].reshape(-1, 16).copy()
    del hseg
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "cb.c"), "w") as fh:
            fh.write(CALLBACKS)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(tmp, "cb.c"), "-o", os.path.join(tmp, "cb.so")])
        copy_page = C.CDLL(os.path.join(tmp, "cb.so")).copy_page
        read_page = page_reader(tmp)
    images, flags = build_relation(dseg, term_key, copy_page)
    ctx = Images(images.ctypes.data, len(images))
    n_terms, n_words = dseg.n_terms, (n_docs + 63) // 64
    del dseg
    setup_s = time.perf_counter() - t0
    print(f"{len(images)} pages, set up in {setup_s:.1f} s", file=sys.stderr, flush=True)
    res = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as fh:
            res = json.load(fh)
    res.update({"gpu": torch.cuda.get_device_name(0), "repetitions": REPS,
                "workload": f"C3: {n_docs} sealed documents / {n_terms} terms, {int(flags.sum())} of them deleted; {N_GROW} inserted documents",
                "pages": len(images), "relation_bytes": int(images.nbytes)})

    def old_route():
        torch.cuda.synchronize()
        t = time.perf_counter()
        words = np.zeros(n_words, np.uint64)
        nd, ndel = C.c_uint32(), C.c_uint32()
        vb.api.check(L.vbm25_sealed_deleted_from_pages(read_page, C.byref(ctx), words.ctypes.data_as(C.c_void_p), n_words, C.byref(nd), C.byref(ndel)))
        t_flags = time.perf_counter() - t
        gs, csr = C.c_void_p(), C.c_void_p()
        vb.api.check(L.vbm25_device_growing_from_pages(gix.h, read_page, C.byref(ctx), C.byref(gs), C.byref(csr)))
        t_read = time.perf_counter() - t
        reader = debug_doubles("vbm25_debug_growing_pages_stats", 4)
        d, out = vb.api.GrowingDesc(), C.c_void_p()
        vb.api.check(L.vbm25_growing_get_desc(csr, C.byref(d)))
        vb.api.check(L.vbm25_index_maintain(gix.h, words.ctypes.data_as(C.c_void_p), C.byref(d), None, C.byref(out)))
        torch.cuda.synchronize()
        total = time.perf_counter() - t
        link = debug_doubles("vbm25_debug_maintain_link_bytes", 2)
        if link is None:   # a build without the counter: the copies csrc/maintain.hip makes of these arguments ...
            link = np.array([8 * n_words + 8 * (d.n_docs + 1) + 20 * d.n_elements + 7 * d.n_docs + 16 * n_terms, 28.0])
            counted = "computed from the arguments"
        else:
            counted = "the library's counter"
        L.vbm25_device_growing_free(gs)
        L.vbm25_growing_free(csr)
        return total, {"sealed_flags_host_walk_s": t_flags, "readers_s": t_read}, reader, link, counted, debug_doubles("vbm25_debug_maintain_phases", 5), \
            vb.DeviceSegment(out), (nd.value, ndel.value)

    def new_route():
        torch.cuda.synchronize()
        t = time.perf_counter()
        dv, out = C.c_void_p(), C.c_void_p()
        vb.api.check(L.vbm25_device_vacuum_from_pages(gix.h, read_page, C.byref(ctx), C.byref(dv)))
        t_read = time.perf_counter() - t
        reader = debug_doubles("vbm25_debug_vacuum_pages_stats", 4)
        vb.api.check(L.vbm25_index_maintain_device(gix.h, dv, None, C.byref(out)))
        torch.cuda.synchronize()
        total = time.perf_counter() - t
        link = debug_doubles("vbm25_debug_maintain_link_bytes", 2)
        nd, ndel = C.c_uint32(), C.c_uint32()
        vb.api.check(L.vbm25_device_vacuum_info(dv, C.byref(nd), C.byref(ndel), None, None, None))
        L.vbm25_device_vacuum_free(dv)
        return total, {"readers_s": t_read}, reader, link, "the library's counter", debug_doubles("vbm25_debug_maintain_phases", 5), vb.DeviceSegment(out), \
            (nd.value, ndel.value)

    for route in routes:
        fn = old_route if route == "old" else new_route
        walls, parts, last = [], [], None
        for rep in range(REPS + 1):
            print(f"{route}: repetition {rep}", file=sys.stderr, flush=True)
            last = fn()
            if rep:   # (the first one loads the device code)
                walls.append(last[0]), parts.append(last[1])
            if rep < REPS:
                del last
        total, _, reader, link, counted, phases, ds, counts = last
        assert counts == (n_docs, int(flags.sum())), counts
        # what every compaction copies for its NEW vocabulary of F tokens, whatever its inputs: the keys (16 F) and starts (8 (F + 1))
        # come down before the encode, which sends the starts and the first blocks up (12 (F + 1)) beside two tables of 256 entries
        # and fetches the block boundaries (4 (F + 1)) and 20 bytes of scalars
        F = ds.n_terms
        vocab_up, vocab_down = 12 * (F + 1) + 4 * 256 + 8 * 256, 16 * F + 8 * (F + 1) + 4 * (F + 1) + 20
        if counted == "computed from the arguments":   # ... and those
            link = link + np.array([vocab_up, vocab_down], np.float64)
        row = {"libvbm25_sha256_16": sha, "median_s": round(float(np.median(walls)), 4), "min_s": round(float(min(walls)), 4),
               "max_s": round(float(max(walls)), 4),
               **{name: round(float(np.median([p[name] for p in parts])), 4) for name in parts[0]},
               "readers_kernels_ms": round(float(reader[0]), 3), "readers_bytes_up": int(reader[1]), "readers_bytes_down": int(reader[2]),
               "elements": int(reader[3]), "compaction_bytes_up": int(link[0]), "compaction_bytes_down": int(link[1]),
               "compaction_bytes": counted, "host_link_bytes_up": int(reader[1] + link[0]), "host_link_bytes_down": int(reader[2] + link[1]),
               **{f"compaction_{n}_ms": round(float(x), 2) for n, x in zip(PHASES, phases)},
               "n_docs": ds.n_docs, "n_postings": ds.n_postings, "segment_crc32": segment_crc(ds)}
        if route == "old":
            row["note"] = "readers_bytes_*: the vectors tape's reader with the CSR copied back; the sealed flags' reader moves nothing over the link"
        else:
            # With a handle nothing O(elements) or O(documents) crosses the link: up go the index's term keys and the new
            # vocabulary's starts and first blocks, down come the new vocabulary's keys, starts and boundaries and 28 bytes of
            # scalars -- O(terms) both ways.  (O(1) down does not hold: the new vocabulary is the host's to keep.)
            assert link[0] == 16 * n_terms + vocab_up, (link[0], n_terms, vocab_up)
            assert link[1] == vocab_down + 28 + 4, (link[1], vocab_down)
            row["compaction_link_bytes_are_O_terms"] = True
        res[f"{route}_route"] = row
        print(json.dumps(row), file=sys.stderr, flush=True)
        del ds, last
    if "old_route" in res and "new_route" in res:
        o, n = res["old_route"], res["new_route"]
        res["segments_equal"] = o["segment_crc32"] == n["segment_crc32"] and o["n_docs"] == n["n_docs"]
        res["new_over_old"] = round(n["median_s"] / o["median_s"], 3)
        res["host_link_bytes_saved"] = (o["host_link_bytes_up"] + o["host_link_bytes_down"]) - (n["host_link_bytes_up"] + n["host_link_bytes_down"])
        assert res["segments_equal"], "the two routes' segments differ"
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
