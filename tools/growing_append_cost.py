#!/usr/bin/env python3
"""growing_append_cost.py -- what vbm25_device_growing_append and vbm25_device_growing_delete cost next to the re-upload they replace.
One job on one MI355X, C3's index (10 M documents), growing documents of about 60 elements (tests/growing_data.py, as
tools/growing_cost.py makes them), the host clock around each synchronous call, 3 warm-up and 20 timed repetitions on fresh segments
of the same size:
  * append of 1, 1 000 and 100 000 documents onto 100 k and onto 1 M documents -- the first append after an upload (it allocates the
    second copy of the postings) and the third (buffers in place: the steady state of a run of inserts) -- next to a
    vbm25_growing_upload of the concatenation, by this build and, with --parent-library, by an earlier build of the library in a child
    process of its own (children alternate between the builds); the HBM bytes an append moves, counted from shapes (24 B per old
    posting, 12 B per new one, 4 B per tile table entry, the delta's staging), over its time against 8 TB/s;
  * delete of 1 and of 10 000 documents at both sizes;
  * kernel_ms of C3's batch (k = 10, k = 100) with a 1 M segment built by 100 appends of 10 000 against a fresh upload of the same
    documents, alternating, with the spread of the repetitions, and vbm25_device_growing_bytes of both;
  * with --parent-tree (a checkout of the earlier commit with its library built): bench.py --gpus 1 --steps 50 --warmup 10 of that tree
    and of this one, alternating.
Prints one JSON object (and writes it to the path given first).

  python tools/growing_append_cost.py out.json [--parent-library PATH] [--parent-tree DIR] [--rounds 2]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, STEPS = 3, 20
BASES = (100_000, 1_000_000)
DELTAS = (1, 1_000, 100_000)
DELETES = (1, 10_000)
POOL = 1_300_000  # documents generated once: the largest base plus three of the largest deltas
HBM_BPS = 8e12
GT = 8192
NEW_SYMBOLS = ("vbm25_device_growing_append", "vbm25_device_growing_delete", "vbm25_device_growing_docs")
FIELDS = ("g_start", "g_key", "g_tf", "g_fieldnorm", "g_payload", "g_deleted")


def docs(G, a, b):
    s = G["g_start"]
    e0, e1 = int(s[a]), int(s[b])
    return dict(g_start=s[a:b + 1] - s[a], g_key=G["g_key"][16 * e0:16 * e1], g_tf=G["g_tf"][e0:e1], g_fieldnorm=G["g_fieldnorm"][a:b],
                g_payload=G["g_payload"][a:b], g_deleted=G["g_deleted"][a:b])


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def load_pool(path):
    return {k: np.load(os.path.join(path, k + ".npy"), mmap_mode="r") for k in FIELDS + ("g_term",)}


def child(pool_dir, appends):
    """one build's measurements (the library is the one VBM25_LIBRARY names, else this tree's)"""
    import ctypes
    from vectorchord_bm25_amd import _lib
    probe = ctypes.CDLL(_lib.library_path())
    for name in NEW_SYMBOLS:  # (an earlier build: only the upload is measured)
        if not hasattr(probe, name):
            _lib.ABI.pop(name, None)
    import vectorchord_bm25_amd as vb
    from bench import WORKLOADS, make_queries
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, _ = WORKLOADS["C3"]
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    P = load_pool(pool_dir)
    G = {k: np.array(P[k]) for k in FIELDS}  # (in memory: no page faults inside a timed call)
    g_term = np.asarray(P["g_term"])
    n_terms = dseg.download().n_terms
    res = {"library": os.path.basename(_lib.library_path()), "upload": {}, "append": {}, "delete": {}}
    live_el = np.repeat(G["g_deleted"] == 0, np.diff(G["g_start"].astype(np.int64))) & (g_term != 0xFFFFFFFF)
    post_upto = np.concatenate([[0], np.cumsum(live_el)])[G["g_start"].astype(np.int64)]  # postings of the documents below g

    def moved_bytes(base, n_new):
        old, new = int(post_upto[base]), int(post_upto[base + n_new] - post_upto[base])
        e0, e1 = int(G["g_start"][base]), int(G["g_start"][base + n_new])
        df = np.bincount(g_term[:e1][live_el[:e1]], minlength=n_terms)
        tiles = -(-(base + n_new) // GT)
        n_tab = int((df >= tiles).sum()) * (tiles + 1) if tiles > 1 else 0
        staging = (e1 - e0) * (16 + 4 + 2 * 12 + 4) + 6 * n_new
        return 24 * old + 12 * new + 4 * n_tab + 12 * n_terms + staging

    for base in BASES:
        B = docs(G, 0, base)
        for d in DELTAS:
            name = f"{base}+{d}"
            cat = docs(G, 0, base + d)
            ts = []
            for r in range(WARMUP + STEPS):
                t, gs = clock(lambda: vb.GrowingSegment(gix, **cat))
                ts.append(t)
                fresh_bytes = gs.device_bytes
                del gs
            res["upload"][name] = dict(stats(ts[WARMUP:]), device_bytes=fresh_bytes)
            if not appends:
                continue
            deltas = [docs(G, base + i * d, base + (i + 1) * d) for i in range(3)]
            first, third = [], []
            for r in range(WARMUP + STEPS):
                gs = vb.GrowingSegment(gix, **B)
                first.append(clock(lambda: gs.append(**deltas[0]))[0])
                gs.append(**deltas[1])
                before = gs.device_bytes
                third.append(clock(lambda: gs.append(**deltas[2]))[0])
                third_allocated = gs.device_bytes != before
                del gs
            mb1, mb3 = moved_bytes(base, d), moved_bytes(base + 2 * d, d)
            f, t3 = stats(first[WARMUP:]), stats(third[WARMUP:])
            f.update(hbm_bytes=mb1, hbm_fraction=round(mb1 / (f["median_ms"] * 1e-3) / HBM_BPS, 4))
            t3.update(hbm_bytes=mb3, hbm_fraction=round(mb3 / (t3["median_ms"] * 1e-3) / HBM_BPS, 4), allocated=bool(third_allocated))
            res["append"][name] = {"first_after_upload": f, "third": t3}
        if not appends:
            continue
        for n_del in DELETES:
            gone = np.random.default_rng(n_del).choice(base, n_del, replace=False).astype(np.uint32)
            ts = []
            for r in range(WARMUP + STEPS):
                gs = vb.GrowingSegment(gix, **B)
                gs.delete(gone[:1])  # (the stage exists)
                ts.append(clock(lambda: gs.delete(gone))[0])
                del gs
            res["delete"][f"{base}-{n_del}"] = stats(ts[WARMUP:])
    if appends:  # a segment built by appends against a fresh upload of the same documents
        terms, off = make_queries(dseg, vocab, nq, nterms, seed=1, zipf_s=zipf_s)
        gs = vb.GrowingSegment(gix, **docs(G, 0, 0))
        for i in range(100):
            gs.append(**docs(G, 10_000 * i, 10_000 * (i + 1)))
        fresh = vb.GrowingSegment(gix, **docs(G, 0, 1_000_000))
        res["built_by_appends"] = {"device_bytes": gs.device_bytes, "fresh_device_bytes": fresh.device_bytes,
                                   "bytes_factor": round(gs.device_bytes / fresh.device_bytes, 3)}
        for k in (10, 100):
            b = vb.Batch(gix, nq, len(terms), k)
            b.set_queries(terms, off)
            ms = {"appended": [], "fresh": []}
            records = {}
            for r in range(WARMUP + STEPS):
                for name, seg in (("appended", gs), ("fresh", fresh)):
                    b.set_growing(seg)
                    b.run()
                    b.fetch()
                    b.set_timing(True)
                    for _ in range(5):
                        b.run()
                    ms[name].append(b.kernel_ms()[0])
                    b.set_timing(False)
                    records[name] = b.fetch()
                    b.set_growing(None)
            assert np.array_equal(records["appended"][1], records["fresh"][1]) and records["appended"][0].tobytes() == records["fresh"][0].tobytes()
            res["built_by_appends"][f"k{k}_kernel_ms"] = {
                n: {"median": round(statistics.median(v[WARMUP:]), 4), "min": round(min(v[WARMUP:]), 4), "max": round(max(v[WARMUP:]), 4)}
                for n, v in ms.items()}
    print("RESULT " + json.dumps(res))


def run_child(pool_dir, library, appends):
    env = dict(os.environ)
    env.pop("VBM25_LIBRARY", None)
    if library:
        env["VBM25_LIBRARY"] = library
    cmd = [sys.executable, os.path.abspath(__file__), "--child", pool_dir] + (["--appends"] if appends else [])
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


def run_bench(tree):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], cwd=tree, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=600).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--parent-library")
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child")
    ap.add_argument("--appends", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.appends)
    from growing_data import make_growing
    import vectorchord_bm25_amd as vb
    from bench import WORKLOADS
    n_docs, vocab, mean_len, len_mode, zipf_s, _, _, _ = WORKLOADS["C3"]
    res = {"steps": STEPS, "warmup": WARMUP, "workload": f"C3: {n_docs} docs / {vocab} vocab", "children": [], "bench": []}

    def save():  # (after every step: a job that is cut short keeps what it has)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")

    with tempfile.TemporaryDirectory() as tmp:
        import torch
        res["gpu"] = torch.cuda.get_device_name(0)
        dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
        G, g_term = make_growing(dseg.download().arrays()["term_key"], POOL, seed=POOL, mean_elems=60)
        del dseg
        for k in FIELDS:
            np.save(os.path.join(tmp, k + ".npy"), G[k])
        np.save(os.path.join(tmp, "g_term.npy"), g_term)
        del G, g_term
        for r in range(a.rounds):  # one child process per build, alternating; the appends are measured once
            if a.parent_library:
                res["children"].append(dict(run_child(tmp, os.path.abspath(a.parent_library), False), build="parent", round=r))
                save()
            res["children"].append(dict(run_child(tmp, None, r == 0), build="this", round=r))
            save()
    if a.parent_tree:
        for r in range(a.rounds):
            for build, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
                res["bench"].append(dict(run_bench(tree), build=build, round=r))
                save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
