#!/usr/bin/env python3
"""stream_live_cost.py -- what a live table costs on the pipelined ring: vbm25_stream_* with a growing segment and a filter attached,
vbm25_filter_extend_growing next to the re-set it replaces, and the stall of the draining calls.  One job on one MI355X, C3's index
(10 M documents generated on the device), every build in a child process of its own:
  1. queries/s through host buffers: 1024 five-term queries, k = 10 and k = 100, through a depth-3 ring (submit / collect, the host
     clock around STEPS steps) with nothing attached, 100 k growing documents, a keep-9/10 sealed filter, both -- beside one batch at
     a time through a resident Batch (set_queries, run, fetch), which is all an earlier build offers for an attached table
     (--parent-library: the same loop timed on that build);
  2. vbm25_filter_extend_growing after appends of 1, 1 000 and 100 000 documents onto 100 k and 1 M, F = 1 and F = 16, beside
     vbm25_filter_set_growing of the full bitmaps (both builds).  The documents have about 4 elements: a bitmap's cost does not depend
     on them;
  3. the stall: wall time of an append of one document, a delete of one and an extend issued with three batches in flight, beside the
     same calls on an idle device;
  4. with --parent-tree (a checkout of the earlier commit with its library built): bench.py --gpus 1 --steps 50 --warmup 10 of that
     tree and of this one, alternating, three times.
Prints one JSON object (and writes it to the path given first).

  python tools/stream_live_cost.py profiles/stream_live_cost.json [--parent-library PATH] [--parent-tree DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, STEPS = 10, 60
BASES = (100_000, 1_000_000)
DELTAS = (1, 1_000, 100_000)
FS = (1, 16)
REPS = 5  # extends per (base, delta, F), the first one untimed
NEW_SYMBOLS = ("vbm25_stream_set_growing", "vbm25_stream_set_filter", "vbm25_stream_submit_filtered", "vbm25_filter_extend_growing",
               "vbm25_multi_batch_set_growing", "vbm25_multi_batch_set_filter")


def docs(G, a, b):
    s = G["g_start"]
    e0, e1 = int(s[a]), int(s[b])
    return dict(g_start=s[a:b + 1] - s[a], g_key=G["g_key"][16 * e0:16 * e1], g_tf=G["g_tf"][e0:e1], g_fieldnorm=G["g_fieldnorm"][a:b],
                g_payload=G["g_payload"][a:b], g_deleted=G["g_deleted"][a:b])


def ms(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def clock(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def child():
    """one build's measurements (the library is the one VBM25_LIBRARY names, else this tree's)"""
    import ctypes
    from vectorchord_bm25_amd import _lib
    probe = ctypes.CDLL(_lib.library_path())
    new = all(hasattr(probe, n) for n in NEW_SYMBOLS)
    if not new:  # (an earlier build: one batch at a time and the re-set only)
        for n in NEW_SYMBOLS:
            _lib.ABI.pop(n, None)
    import vectorchord_bm25_amd as vb
    from bench import WORKLOADS, make_queries
    from growing_data import make_growing
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, _ = WORKLOADS["C3"]
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    term_key = np.array(dseg.download().arrays()["term_key"])  # (a copy: the downloaded segment is not kept)
    terms, off = make_queries(dseg, vocab, nq, nterms, seed=1, zipf_s=zipf_s)
    res = {"library": os.path.basename(_lib.library_path()), "has_live_ring": new, "qps": {}, "bitmaps": {}, "stall": {}}

    # 1. queries/s through host buffers
    n_grow = 100_000
    G, _ = make_growing(term_key, n_grow, seed=11, mean_elems=60)
    gs = vb.GrowingSegment(gix, **G)
    f = vb.DocFilter(gix, np.arange(n_docs) % 10 != 7)
    f.set_growing(gs, np.arange(n_grow) % 10 != 3)
    sel = np.zeros(nq, np.uint32)
    for k in (10, 100):
        for case, a_gs, a_f in (("none", None, None), ("growing", gs, None), ("filter", None, f), ("both", gs, f)):
            row = {}
            b = vb.Batch(gix, nq, len(terms), k)
            if a_f is not None:
                b.set_filter(a_f, sel)
            b.set_growing(a_gs)

            def one():
                b.set_queries(terms, off)
                b.run()
                return b.fetch()
            for _ in range(WARMUP):
                ref = one()
            t = clock(lambda: [one() for _ in range(STEPS)])
            row["batch_qps"] = round(nq * STEPS / t)
            row["batch_step_ms"] = round(t / STEPS * 1e3, 4)
            del b
            if new or case == "none":
                st = vb.Stream(gix, 3, nq, len(terms), k)
                if new:
                    st.set_growing(a_gs)
                    st.set_filter(a_f)
                q_filter = sel if a_f is not None else None
                submit = (lambda: st.submit(terms, off, q_filter=q_filter)) if new else (lambda: st.submit(terms, off))
                out = (np.zeros((nq, k), dtype=vb.HIT_DTYPE), np.zeros(nq, dtype=np.uint32))

                def ring(n):
                    for _ in range(3):
                        submit()
                    for _ in range(n - 3):
                        st.collect(out)
                        submit()
                    for _ in range(3):
                        st.collect(out)
                ring(WARMUP)
                t = clock(lambda: ring(STEPS))
                assert np.array_equal(out[1], ref[1]) and out[0].tobytes() == ref[0].tobytes(), f"k={k} {case}: the ring's records differ"
                row["ring_qps"] = round(nq * STEPS / t)
                row["ring_step_ms"] = round(t / STEPS * 1e3, 4)
                row["ring_over_batch"] = round(row["ring_qps"] / row["batch_qps"], 3)
                del st
            res["qps"][f"k{k}_{case}"] = row

    # 3. the stall of the draining calls (this build): three k = 10 batches in flight, then the call
    if new:
        st = vb.Stream(gix, 3, nq, len(terms), 10)
        st.set_growing(gs)
        st.set_filter(f)
        extra, _ = make_growing(term_key, 64, seed=12, mean_elems=60)
        stall = {"append_1": ([], []), "delete_1": ([], []), "extend_1": ([], [])}
        nxt = iter(range(64))

        def fill(busy, filtered):
            for _ in range(3 if busy else 0):
                st.submit(terms, off, q_filter=sel if filtered else None)

        def drain():
            while st.in_flight:
                st.collect()
        for r in range(2 * 7):
            busy = r % 2
            i = next(nxt)
            fill(busy, True)
            stall["append_1"][busy].append(clock(lambda: gs.append(**docs(extra, i, i + 1))))
            drain()
            fill(busy, False)  # (the bitmaps are stale until the extend: plain submits)
            stall["extend_1"][busy].append(clock(lambda: f.extend_growing(gs, np.ones((1, 1), bool))))
            drain()
            fill(busy, True)
            stall["delete_1"][busy].append(clock(lambda: gs.delete(np.array([r], np.uint32))))
            drain()
        res["stall"] = {name: {"idle": ms(v[0][1:]), "three_in_flight": ms(v[1][1:])} for name, v in stall.items()}
        del st
    del gs, f

    # 2. extend against re-set (documents of about 4 elements)
    pool_n = BASES[-1] + REPS * DELTAS[-1]
    P, _ = make_growing(term_key, pool_n, seed=13, mean_elems=4, deleted=0.0)
    for base in BASES:
        for d in DELTAS:
            for F in FS:
                ff = vb.DocFilter.__new__(vb.DocFilter)  # (F sealed bitmaps of zeros, made by the library: nothing to pack here)
                ff.index, ff.growing, ff.grow_n, ff.n_bitmaps, ff.h = gix, None, 0, F, ctypes.c_void_p()
                vb.api.check(vb.lib().vbm25_filter_create(gix.h, F, None, ctypes.byref(ff.h)))
                seg = vb.GrowingSegment(gix, **docs(P, 0, base))
                bits = np.random.default_rng(F).random((F, base + REPS * d)) < 0.9
                row = {}
                n = base
                ff.set_growing(seg, bits[:, :n])
                ext, reset = [], []
                for r in range(REPS):
                    seg.append(**docs(P, n, n + d))
                    if new:
                        ext.append(clock(lambda: ff.extend_growing(seg, bits[:, n:n + d])))
                    n += d
                    words = vb.DocFilter.pack(bits[:, :n], n)  # (packed outside the clock: the call alone)
                    reset.append(clock(lambda: vb.api.check(vb.lib().vbm25_filter_set_growing(ff.h, seg.h, words.ctypes.data))))
                    ff.grow_n = n
                row["set_growing_full"] = dict(ms(reset[1:]), host_link_bytes=int(8 * F * ((n + 63) // 64)))
                if new:
                    row["extend"] = dict(ms(ext[1:]), host_link_bytes=int(8 * F * ((d + 63) // 64)))
                res["bitmaps"][f"{base}+{d}_F{F}"] = row
                del seg, ff
    print("RESULT " + json.dumps(res))


def run_child(library):
    env = dict(os.environ)
    env.pop("VBM25_LIBRARY", None)
    if library:
        env["VBM25_LIBRARY"] = library
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, stdout=subprocess.PIPE, text=True,
                         timeout=900).stdout
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
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    res = {"steps": STEPS, "warmup": WARMUP, "workload": "C3", "children": [], "bench": []}

    def save():  # (after every step: a job that is cut short keeps what it has)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")

    if a.parent_library:
        res["children"].append(dict(run_child(os.path.abspath(a.parent_library)), build="parent"))
        save()
    res["children"].append(dict(run_child(None), build="this"))
    save()
    if a.parent_tree:
        for r in range(3):
            for build, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
                res["bench"].append(dict(run_bench(tree), build=build, round=r))
                save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
