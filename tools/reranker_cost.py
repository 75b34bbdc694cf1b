#!/usr/bin/env python3
"""reranker_cost.py -- what the reranker ring (vbm25_reranker) buys on one MI355X, on the shape of tools/rerank_cost.py: --docs
documents (default 1 000 000) of log-normal length 100, 1024 queries x 5 lexemes, 1000 candidates each, k = 10.  All variants run in
one process on the same inputs, alternating inside every repetition, every shape warmed; their rows are compared byte for byte
before a time is reported.
  (a) parent      the parent route: a Resolver ring one batch ahead of Scorer.topk (resolve of batch i + 1 under the rerank of batch i;
                  the ids come home and go up again)
  (b) ring        Reranker.submit from lexemes with cand_doc, the ring kept full, at depth 1, 2 and 3
  (c) ctids       Reranker.submit with cand_tid at depth 3, against (b) at depth 3 plus the host-side map a caller needs without it:
                  np.searchsorted of the same ctids' keys in the sorted payload keys, every step
  (d) kernels     the device time of a batch between its slot's events (upload excluded, the rows' download included), depth 1
  times           host clock around --steps steps (default 200), --reps repetitions (default 7): median and min - max per step
  verdict         per variant the parent's median minus its own, and whether that margin exceeds three times the parent route's own
                  max - min spread in this run (the convention of DESIGN section 8)
  directory       the create-time cost of the payload directory: its kernels by events, and create with and without payloads by the clock
Writes one JSON object to the path given first.  One process on the GPU; run it under a timeout.

  python tools/reranker_cost.py profiles/reranker_cost.json [--docs 1000000] [--steps 200] [--reps 7]"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cast_cost import SEED, VOCAB, make_corpus, ms, vocabulary  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def debug(vb, reranker):
    f = vb.lib().vbm25_debug_reranker
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 4
    batch, directory = C.c_double(), C.c_double()
    vb._lib.check(f(reranker.h, C.byref(batch), None, C.byref(directory)))
    return batch.value, directory.value


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out", nargs="?")
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--reps", type=int, default=7)
    a = p.parse_args()
    import vectorchord_bm25_amd as vb

    alive = threading.Event()

    def heartbeat():
        t0 = time.perf_counter()
        while not alive.wait(60):
            say(f"... {time.perf_counter() - t0:.0f} s")

    threading.Thread(target=heartbeat, daemon=True).start()
    nq, n_lex, n_cand, k = 1024, 5, 1000, 10
    make_corpus.vocab = vocabulary()
    rng = np.random.default_rng(1)
    lens = np.clip(np.rint(rng.lognormal(np.log(0.8 * 100), 0.6, a.docs)), 8, 2000).astype(np.int64)
    corpus = make_corpus(a.docs, lens, 0.05, seed=3)
    say(f"corpus of {a.docs} documents made")
    h = vb.Documents.cast((corpus["data"], corpus["lex_off"], corpus["lex_count"], corpus["doc_lex"]), corpus["payload"], seed=SEED)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(h, 1.2, 0.75))
    resolver = vb.Resolver(gix, 2, nq, nq * n_lex, nq * n_lex * 8, seed=SEED)
    dt = h.bind(resolver)
    packed = vb.pack_lexemes([[b"%d" % i for i in rng.choice(VOCAB, n_lex, replace=False)] for _ in range(nq)])
    q_cand = (np.arange(nq + 1) * n_cand).astype(np.uint64)
    cand_doc = rng.integers(0, h.n_docs, nq * n_cand).astype(np.uint32)
    payload = np.ascontiguousarray(corpus["payload"])
    cand_tid = np.ascontiguousarray(payload[cand_doc])
    # the host-side map of a caller without the directory: the sorted payload keys and their documents (stable: the lowest first)
    keys = vb.TidSet.keys(payload)
    order = np.argsort(keys, kind="stable")
    sorted_keys, sorted_docs = keys[order], order.astype(np.uint32)

    def host_map():
        return sorted_docs[np.searchsorted(sorted_keys, vb.TidSet.keys(cand_tid))]

    # a ctid of several documents names the lowest: the rows are compared on these documents
    lowest = host_map()
    caps = (nq, nq * n_lex, nq * n_lex * 8, nq * n_cand, k)
    t0 = time.perf_counter()
    plain = [dt.reranker(resolver, d, *caps) for d in (1, 2, 3)]
    t1 = time.perf_counter()
    with_tids = dt.reranker(resolver, 3, *caps, documents=h)
    t2 = time.perf_counter()
    scorer = dt.scorer()
    res = {"unit": "ms", "n_docs": h.n_docs, "queries": nq, "query_lexemes": n_lex, "candidates_per_query": n_cand, "k": k, "steps": a.steps,
           "reps": a.reps, "vocabulary": VOCAB,
           "link_bytes_per_step": {"parent_up": int(packed[0].nbytes + packed[1].nbytes + packed[2].nbytes + 8 * (nq + 1) + 4 * nq * n_cand),
                                   "ring_up_cand_doc": int(packed[0].nbytes + packed[1].nbytes + packed[2].nbytes + 20 * (nq + 1) + 4 * nq * n_cand),
                                   "ring_up_cand_tid": int(packed[0].nbytes + packed[1].nbytes + packed[2].nbytes + 20 * (nq + 1) + 6 * nq * n_cand),
                                   "down": 16 * nq * k + 4 * nq},
           "directory": {"kernels_ms": round(debug(vb, with_tids)[1], 4), "create_depth_3_with_payloads_ms": round((t2 - t1) * 1e3, 3),
                         "create_depths_1_2_3_without_payloads_ms": round((t1 - t0) * 1e3, 3),
                         "reranker_device_bytes": {"depth_3_with_payloads": with_tids.device_bytes(), "depth_3": plain[2].device_bytes()}}}

    def parent(steps):
        resolver.submit(packed)
        out = None
        for _ in range(steps):
            resolver.submit(packed)
            ids, off = resolver.collect()
            out = scorer.topk(ids, off, k, q_cand, cand_doc)
        resolver.collect()
        return out

    def ring(r, steps, **cands):
        out = None
        for _ in range(steps):
            if r.in_flight() == r.depth:
                out = r.collect()
            r.submit(packed, k, q_cand, **cands)
        while r.in_flight():
            out = r.collect()
        return out

    variants = {"parent": lambda s: parent(s),
                "ring_depth_1": lambda s: ring(plain[0], s, cand_doc=cand_doc),
                "ring_depth_2": lambda s: ring(plain[1], s, cand_doc=cand_doc),
                "ring_depth_3": lambda s: ring(plain[2], s, cand_doc=cand_doc),
                "ring_depth_3_cand_tid": lambda s: ring(with_tids, s, cand_tid=cand_tid),
                "ring_depth_3_host_searchsorted": lambda s: ring_mapped(s)}

    def ring_mapped(steps):
        r, out = plain[2], None
        for _ in range(steps):
            if r.in_flight() == r.depth:
                out = r.collect()
            r.submit(packed, k, q_cand, cand_doc=host_map())
        while r.in_flight():
            out = r.collect()
        return out

    want = parent(2)
    resolver.submit(packed)
    want_low = scorer.topk(*resolver.collect(), k, q_cand, lowest)
    for name, fn in variants.items():  # every shape warmed, every variant's rows checked
        got = fn(4)
        ref = want if name in ("parent", "ring_depth_1", "ring_depth_2", "ring_depth_3") else want_low
        if got[0].tobytes() != ref[0].tobytes() or not np.array_equal(got[1], ref[1]):
            raise SystemExit(f"{name}: the rows differ from the parent route's")
    say("rows equal; timing")
    times = {name: [] for name in variants}
    for rep in range(a.reps):
        for name, fn in variants.items():
            t = time.perf_counter()
            fn(a.steps)
            times[name].append((time.perf_counter() - t) / a.steps)
        say(f"repetition {rep}: " + ", ".join(f"{n} {times[n][-1] * 1e3:.3f}" for n in variants))
    per_step = {name: ms(ts) for name, ts in times.items()}
    spread = per_step["parent"]["max"] - per_step["parent"]["min"]
    res["per_step_ms"] = per_step
    res["parent_spread_ms"] = round(spread, 4)
    res["verdict"] = {name: {"margin_ms": round(per_step["parent"]["median"] - t["median"], 4),
                             "margin_exceeds_3_spreads": bool(per_step["parent"]["median"] - t["median"] > 3 * spread)}
                      for name, t in per_step.items() if name != "parent"}
    tid_margin = per_step["ring_depth_3_host_searchsorted"]["median"] - per_step["ring_depth_3_cand_tid"]["median"]
    tid_spread = per_step["ring_depth_3_host_searchsorted"]["max"] - per_step["ring_depth_3_host_searchsorted"]["min"]
    res["verdict"]["cand_tid_against_host_searchsorted"] = {"margin_ms": round(tid_margin, 4), "host_route_spread_ms": round(tid_spread, 4),
                                                            "margin_exceeds_3_spreads": bool(tid_margin > 3 * tid_spread)}
    t_map = []
    for _ in range(10):
        t = time.perf_counter()
        host_map()
        t_map.append(time.perf_counter() - t)
    res["host_searchsorted_alone_ms"] = ms(t_map)
    # (d) the device time of a batch, by the slot's events
    share = {}
    for name, r, cands in (("cand_doc", plain[0], dict(cand_doc=cand_doc)), ("cand_tid", with_tids, dict(cand_tid=cand_tid))):
        batch = []
        for _ in range(50):
            r.submit(packed, k, q_cand, **cands)
            r.collect()
            batch.append(debug(vb, r)[0] / 1e3)
        share[name] = ms(batch[5:])
    res["batch_device_ms_between_events"] = share
    alive.set()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
