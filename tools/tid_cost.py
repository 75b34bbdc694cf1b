#!/usr/bin/env python3
"""tid_cost.py -- what it costs to decide which documents a set of heap rows refers to, on the device (csrc/tid.hip) and on the host,
at C3's shape built on the device (10 M documents, 30 k vocabulary, synthetic ctids in heap order).

Sets of 1 k, 100 k, 1 M and 5 M TIDs drawn from the documents' payloads plus as many TIDs no document holds.  Per set size:
  create        TidSet(tids): upload, pack, sort, unique, directory (wall, ends in a synchronise)
  kernel        tid_match_kernel over the index's payload plane between two HIP events (vbm25_debug_tid_match_ms), for every tid_dir
                candidate, on the documents in ctid order (the index) and on a shuffled payload plane (a growing segment of 10 M
                documents without elements whose payloads are a permutation of the index's)
  match_index   the whole call, words and count on the host (wall)
  set_tids      DocFilter.set_tids, no bitmap crossing the link (wall)
  bulkdelete    DeviceVacuum.bulkdelete + DeviceSegment.maintain_device against maintain_device alone on the same handle, on the
                relation of tools/vacuum_device_cost.py (1 % of the sealed documents deleted in the pages, 100 000 inserted documents)
  host          the route a caller without the kernel takes, one thread: np.searchsorted of the documents' packed uint64 keys in the
                sorted set + np.packbits + vbm25_filter_update.  The documents' keys are held on the host already: the download of
                the 60 MB payload plane (or the page walk that rebuilds it) is NOT counted.
The load floor is the kernel against the empty set: payload loads, ballot and store, no search.
One warm-up and REPS repetitions each; median, min and max.  The results go to argv[1] as JSON with the library's sha256."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch  # (before the library is loaded: both bring a HIP runtime, and torch's has to be the process's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vectorchord_bm25_amd as vb  # noqa: E402
from bench import WORKLOADS  # noqa: E402

REPS = 5
SET_SIZES = (1_000, 100_000, 1_000_000, 5_000_000)
DIRS = (0, 4, 8, 10, 11, 12)


def stats(xs, scale=1.0, digits=6):
    xs = [x * scale for x in xs]
    return {"median": round(float(np.median(xs)), digits), "min": round(float(min(xs)), digits), "max": round(float(max(xs)), digits)}


def timed(fn, reps=REPS):
    """wall seconds of fn() ending in a device synchronise: one warm-up, then reps"""
    out = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep:
            out.append(time.perf_counter() - t)
    return out


def kernel_ms():
    f = vb.lib().vbm25_debug_tid_match_ms
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    out = np.zeros(1, np.float64)
    vb.api.check(f(out.ctypes.data_as(C.c_void_p)))
    return float(out[0])


def kernel_times(ts, target, growing, reps=REPS):
    out = []
    for rep in range(reps + 1):
        ts.match_growing(target) if growing else ts.match(target)
        if rep:
            out.append(kernel_ms())
    return out


def synthetic_payloads(n_docs):
    d = np.arange(n_docs, dtype=np.uint64)
    blk = d // 64
    return np.stack([blk >> 16, blk & 0xffff, d % 64 + 1], axis=1).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--docs", type=int, default=0, help="documents instead of C3's (a rehearsal)")
    ap.add_argument("--no-vacuum", action="store_true", help="skip the bulkdelete + maintain_device part (it writes the 2 GB relation)")
    args = ap.parse_args()
    with open(vb.library_path(), "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()[:16]
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C3"]
    if args.docs:
        n_docs = args.docs
    sizes = [s for s in SET_SIZES if s <= n_docs // 2]
    t0 = time.perf_counter()
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    payload = synthetic_payloads(n_docs)
    doc_keys = vb.TidSet.keys(payload)
    rng = np.random.default_rng(7)
    perm = rng.permutation(n_docs)
    empty_key = np.zeros((0, 16), np.uint8)
    shuffled = vb.GrowingSegment(gix, np.zeros(n_docs + 1, np.uint64), empty_key, np.zeros(0, np.uint32), np.zeros(n_docs, np.uint8),
                                 payload[perm])
    filt = vb.DocFilter(gix, np.zeros((1, n_docs), bool))
    print(f"{n_docs} documents set up in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    res = {"gpu": torch.cuda.get_device_name(0), "libvbm25_sha256_16": sha, "repetitions": REPS,
           "workload": f"C3 built on the device: {n_docs} documents / {dseg.n_terms} terms, synthetic ctids in heap order",
           "default_tid_dir": 11,
           "host_route_note": "documents' packed keys held on the host: the 60 MB payload download (or the page walk) is not counted; one thread",
           "sets": {}}

    # the load floor: the empty set
    with vb.TidSet(np.zeros((0, 3), np.uint16)) as ts:
        res["load_floor_kernel_ms"] = {"ctid_order": stats(kernel_times(ts, gix, False)), "shuffled": stats(kernel_times(ts, shuffled, True))}

    for n_set in sizes:
        members = payload[rng.choice(n_docs, n_set, replace=False)]
        # as many TIDs no document holds: offsets 65 .. of blocks the table has (ip_posid beyond the 64 tuples a block takes)
        absent = members.copy()
        absent[:, 2] += 64
        tids = np.concatenate([members, absent])[rng.permutation(2 * n_set)]
        row = {"tids": int(len(tids)), "members": n_set}
        holder = []

        def create():
            holder.clear()
            holder.append(vb.TidSet(tids))
        row["create_s"] = stats(timed(create))
        row["kernel_ms_by_tid_dir"] = {}
        for d in DIRS:
            vb.set_tuning("tid_dir", d)
            with vb.TidSet(tids) as ts:
                words, n_match = ts.match(gix)
                assert n_match == n_set, (n_match, n_set)
                w2, n2 = ts.match_growing(shuffled)
                assert n2 == n_set
                row["kernel_ms_by_tid_dir"][str(d)] = {"ctid_order": stats(kernel_times(ts, gix, False)),
                                                       "shuffled": stats(kernel_times(ts, shuffled, True))}
        vb.reset_tuning()
        ts = holder[0]
        row["device_bytes"] = ts.device_bytes()
        row["match_index_s"] = stats(timed(lambda: ts.match(gix)))
        row["set_tids_s"] = stats(timed(lambda: filt.set_tids(0, ts)))
        dev_words = filt.read(0)

        # the host route
        def host():
            sk = np.unique(vb.TidSet.keys(tids))
            at = np.searchsorted(sk, doc_keys)
            at[at == len(sk)] = 0
            hit = sk[at] == doc_keys
            pad = np.zeros(64 * ((n_docs + 63) // 64), bool)
            pad[:n_docs] = hit
            words = np.packbits(pad, bitorder="little").view("<u8")
            vb.api.check(vb.lib().vbm25_filter_update(filt.h, 0, words.ctypes.data_as(C.c_void_p)))
        row["host_route_s"] = stats(timed(host, reps=3))
        assert np.array_equal(filt.read(0), dev_words) and np.array_equal(dev_words, words), "the host route and the device route differ"
        row["host_over_device"] = round(row["host_route_s"]["median"] / max(row["set_tids_s"]["median"], 1e-9), 1)
        row["host_over_device_with_create"] = round(row["host_route_s"]["median"] / (row["set_tids_s"]["median"] + row["create_s"]["median"]), 1)
        res["sets"][str(n_set)] = row
        print(json.dumps({n_set: row}), file=sys.stderr, flush=True)
        holder.clear()
        del ts

    def save():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")
    save()
    if not args.no_vacuum:
        from growing_pages_cost import Images, page_reader  # noqa: E402
        from pages_write_cost import CALLBACKS  # noqa: E402
        import vacuum_device_cost as V  # noqa: E402
        hseg = dseg.download()
        term_key = hseg.arrays()["term_key"].reshape(-1, 16).copy()
        del hseg
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "cb.c"), "w") as fh:
                fh.write(CALLBACKS)
            subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(tmp, "cb.c"), "-o", os.path.join(tmp, "cb.so")])
            copy_page = C.CDLL(os.path.join(tmp, "cb.so")).copy_page
            read_page = page_reader(tmp)
        images, flags = V.build_relation(dseg, term_key, copy_page)
        ctx = Images(images.ctypes.data, len(images))
        L = vb.lib()
        res["vacuum_relation"] = f"{len(images)} pages, {int(flags.sum())} sealed documents deleted in them, {V.N_GROW} inserted documents"
        for n_set in sizes:
            members = payload[rng.choice(n_docs, n_set, replace=False)]
            alone, both, fresh = [], [], []
            with vb.TidSet(members) as ts:
                for rep in range(4):
                    h = C.c_void_p()
                    vb.api.check(L.vbm25_device_vacuum_from_pages(gix.h, read_page, C.byref(ctx), C.byref(h)))
                    dv = vb.DeviceVacuum(gix, h)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    seg = vb.DeviceSegment.maintain_device(gix, dv)
                    torch.cuda.synchronize()
                    t_alone = time.perf_counter() - t
                    del seg
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    new = dv.bulkdelete(gix, ts)
                    torch.cuda.synchronize()
                    t_bulk = time.perf_counter() - t
                    seg = vb.DeviceSegment.maintain_device(gix, dv)
                    torch.cuda.synchronize()
                    t_both = time.perf_counter() - t
                    if rep:
                        alone.append(t_alone), both.append(t_both), fresh.append(t_bulk)
                    kept = seg.n_docs
                    del seg, dv
            res["sets"][str(n_set)]["vacuum"] = {"maintain_device_alone_s": stats(alone), "bulkdelete_s": stats(fresh),
                                                 "bulkdelete_and_maintain_device_s": stats(both), "newly_deleted_sealed": new[0],
                                                 "documents_kept": kept}
            print(json.dumps({n_set: res["sets"][str(n_set)]["vacuum"]}), file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1), flush=True)
    save()


if __name__ == "__main__":
    main()
