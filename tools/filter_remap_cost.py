#!/usr/bin/env python3
"""filter_remap_cost.py -- what carrying a filter across VACUUM's compaction costs on the device (vbm25_filter_remap) at C3 (10 M
documents, device-generated index): {0, 1, 10} % deleted sealed documents x {0, 100 k, 1 M} growing documents (tests/growing_data.py
at its default of about 12 elements each -- the filter's cost depends on their number only --, 10 % of them deleted) x F = {1, 16}
bitmaps.  Per cell: the wall time of vbm25_filter_remap (best of three); the wall time of the host route it replaces -- the relabel
table's download (vbm25_index_maintain with and without relabel, best of two each, the difference), the F sealed and growing bitmaps
read with vbm25_filter_read, permuted through the relabel table with numpy, and vbm25_filter_create of the result --; the bytes
either route moves over the host link; and whether the two filters hold the same words.  Prints one JSON object (and writes it to
argv[1] when given)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vectorchord_bm25_amd as vb  # noqa: E402
from bench import WORKLOADS  # noqa: E402
from corpus import token_keys  # noqa: E402
from filter_remap_model import unpack_bits  # noqa: E402
from growing_data import make_growing  # noqa: E402

NONE = 0xFFFFFFFF


def best_of(n, fn):
    import torch

    best, out = None, None
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None else min(best, ms)
    return best, out


def main():
    import torch

    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C3"]
    t0 = time.perf_counter()
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    term_key, _ = token_keys(vocab)  # (the synthetic corpus' keys: decimals, bytewise order)
    rng = np.random.default_rng(1)
    grow = {0: None}
    for n_grow in (100_000, 1_000_000):
        grow[n_grow], _ = make_growing(term_key, n_grow, seed=n_grow)
    dels = {p: (rng.random(n_docs) < p / 100.0) for p in (0, 1, 10)}
    res = {"gpu": torch.cuda.get_device_name(0), "workload": f"C3: {n_docs} docs / {vocab} vocab / {dseg.n_postings} postings",
           "setup_s": round(time.perf_counter() - t0, 1), "cells": {}}
    W = (n_docs + 63) // 64
    for n_grow, G in grow.items():
        gs = vb.GrowingSegment(gix, **G) if G is not None else None
        GW = (n_grow + 63) // 64
        for p, deleted in dels.items():
            sd = deleted if p else None
            gdel = G["g_deleted"] if G is not None else None
            with_ms, (ds, relabel) = best_of(2, lambda: vb.DeviceSegment.maintain(gix, sd, G, return_relabel=True))
            without_ms, _ = best_of(2, lambda: vb.DeviceSegment.maintain(gix, sd, G))
            nix = vb.GpuIndex(ds)
            OW = (nix.n_docs + 63) // 64
            for F in (1, 16):
                bits = np.unpackbits(rng.integers(0, 256, (F, 8 * (W + GW)), dtype=np.uint8), axis=1, bitorder="little").astype(bool)
                f = vb.DocFilter(gix, bits[:, :n_docs])
                if gs is not None:
                    f.set_growing(gs, bits[:, 64 * W: 64 * W + n_grow])
                del bits
                remap_ms, nf = best_of(3, lambda: f.remap(nix, sd, gdel))

                def host_route():
                    old = np.stack([f.read(i) for i in range(F)])
                    ob = unpack_bits(old, n_docs)
                    if gs is not None:
                        ob = np.concatenate([ob, unpack_bits(np.stack([f.read(i, growing=True) for i in range(F)]), n_grow)], axis=1)
                    kept = relabel != NONE
                    nb = np.zeros((F, nix.n_docs), bool)
                    nb[:, relabel[kept]] = ob[:, kept]
                    return vb.DocFilter(nix, nb)

                host_ms, hf = best_of(1, host_route)
                same = all(np.array_equal(nf.read(i), hf.read(i)) for i in range(F))
                relabel_ms = max(with_ms - without_ms, 0.0)
                row = {"remap_ms": round(remap_ms, 3), "host_route_ms": round(host_ms + relabel_ms, 1),
                       "host_route_relabel_download_ms": round(relabel_ms, 2), "host_route_read_permute_create_ms": round(host_ms, 1),
                       "maintain_ms": round(without_ms, 1), "maintain_with_relabel_ms": round(with_ms, 1),
                       "remap_link_bytes": (8 * (W + GW) if p or G is not None else 0) + 8,
                       "host_route_link_bytes": 4 * (n_docs + n_grow) + 8 * F * (W + GW) + 8 * F * OW,
                       "n_docs_after": nix.n_docs, "same_words": bool(same)}
                res["cells"][f"del{p}_grow{n_grow}_F{F}"] = row
                print(f"del {p}% grow {n_grow} F {F}: {row}", file=sys.stderr)
                del f, nf, hf
            del nix, ds, relabel
        del gs
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
