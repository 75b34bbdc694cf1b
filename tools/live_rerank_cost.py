#!/usr/bin/env python3
"""live_rerank_cost.py -- what following a live table costs the rerank stack on one MI355X: DocTerms.append_documents + Reranker.sync
(vbm25_doc_terms_append_documents, vbm25_reranker_sync: kernels by HIP events, the calls end to end) for deltas of 1, 1000 and 100 000
cast documents, ALTERNATED in the same run with the route the library forced before them -- GpuIndex.bind of the index again,
Documents.bind of every unsealed row so far, and a new reranker on the index-bound handle --, and the 1024 x 1000 rerank at k = 10 by
ctid on the grown handle beside the same rerank on a freshly built one (expected equal; the rows are compared byte for byte).
  corpus    --docs documents (default 1 000 000) of log-normal length 100 over 30 000 lexemes (tools/forward_cost.py's corpus); the
            index is DeviceSegment.from_documents of their cast, the handle GpuIndex.bind, the ring depth 2 from_index
  deltas    documents of the same kind with ctids of their own, cast before the clock starts (the cast is the caster's cost:
            tools/caster_cost.py)
Host clock around synchronous calls, one untimed and --reps timed repetitions a delta size (7), median / min / max.  A gain is a margin
of more than three times the old route's own max - min spread.
  stream    the step of a serving Stream on the same index (1024 queries of 5 terms, k = 10, depth 3; tools/caster_cost.py's stream part
            with 5000 steps after 20 untimed, so that the loop lasts through some hundred appends): alone, and beside a thread that appends
            a delta of 1 or of 1000 cast rows to a second index-bound handle and syncs its ring, over and over -- every append waits for the
            whole device once.  Median and largest step, each against the two loops alone by the three-spreads rule.
Writes one JSON object to the path given first.

  python tools/live_rerank_cost.py profiles/live_rerank_cost.json [--docs 1000000] [--reps 7]"""
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

from cast_cost import SEED, VOCAB, make_corpus, ms, timed, vocabulary  # noqa: E402

CAPS = dict(max_queries=1024, max_lexemes=1024 * 5, max_bytes=1024 * 5 * 8, max_candidates=1024 * 1000, max_k=10)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def debug_ms(vb, name, *handle):
    f = getattr(vb.lib(), name)
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * (len(handle) + 1)
    t = C.c_double()
    vb._lib.check(f(*handle, C.byref(t)))
    return t.value / 1e3


def corpus(n, seed, first_ctid):
    rng = np.random.default_rng(seed)
    lens = np.clip(np.rint(rng.lognormal(np.log(0.8 * 100), 0.6, n)), 8, 2000).astype(np.int64)
    c = make_corpus(n, lens, 0.05, seed=seed + 2)
    flat = first_ctid + np.arange(n, dtype=np.uint64)  # (ctids of their own, ascending: what a heap hands out)
    c["payload"] = np.stack([(flat >> 32) & 0xFFFF, (flat >> 16) & 0xFFFF, flat & 0xFFFF], axis=1).astype(np.uint16)
    return c


def stream_beside(vb, gix, resolver, term_ids, q_off, cast, steps=5000):
    """the step of a serving stream: alone, beside appends of 1 row + sync, beside appends of 1000 rows + sync, alone again"""
    st = vb.Stream(gix, 3, len(q_off) - 1, len(term_ids), 10)

    def loop():
        st.submit(term_ids, q_off)
        st.submit(term_ids, q_off)
        ts = []
        for _ in range(20 + steps):
            t0 = time.perf_counter()
            st.submit(term_ids, q_off)
            st.collect()
            ts.append(time.perf_counter() - t0)
        st.collect()
        st.collect()
        return ms(ts[20:])

    def beside(n_rows):
        deltas = [cast(corpus(n_rows, 500 + i, (1 << 40) + i * n_rows)) for i in range(8)]  # (cast before the loop: the neighbour only appends and syncs)
        dt = gix.bind()
        stop, count, errors = threading.Event(), [0], []
        with dt.reranker(resolver, 2, **CAPS, from_index=True) as ring:
            def run():
                try:
                    while not stop.is_set():
                        dt.append_documents(deltas[count[0] % len(deltas)], resolver)
                        ring.sync()
                        count[0] += 1
                except BaseException as e:  # noqa: BLE001
                    errors.append(repr(e))
            th = threading.Thread(target=run)
            th.start()
            time.sleep(0.2)  # (the neighbour is warm before the timed loop starts)
            before, t_loop = [count[0]], time.perf_counter()
            out = loop()
            stop.set()
            th.join()
        if errors:
            raise SystemExit(f"the neighbour failed: {errors}")
        out["neighbour_appends"], out["loop_ms"] = count[0] - before[0], round(1e3 * (time.perf_counter() - t_loop), 1)
        return out

    res = {"steps": steps, "warmup_steps": 20, "stream_depth": 3, "queries": len(q_off) - 1, "k": 10}
    res["alone"] = loop()
    res["beside_appends_of_1"] = beside(1)
    res["beside_appends_of_1000"] = beside(1000)
    res["alone_again"] = loop()
    spread = max(res["alone"]["max"], res["alone_again"]["max"]) - min(res["alone"]["min"], res["alone_again"]["min"])
    res["alone_spread_ms"] = round(spread, 4)
    for name in ("beside_appends_of_1", "beside_appends_of_1000"):
        for what in ("median", "max"):  # (the largest step against the larger of the two largest steps alone)
            d = res[name][what] - max(res["alone"][what], res["alone_again"][what])
            res[name][what + "_minus_alone_ms"] = round(d, 4)
            res[name][what + "_verdict"] = "slower shown" if d > 3 * spread else "no difference measured"
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out", nargs="?")
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=7)
    a = p.parse_args()
    if a.reps < 7:
        raise SystemExit("at least 7 repetitions")
    import vectorchord_bm25_amd as vb
    make_corpus.vocab = vocabulary()
    c = corpus(a.docs, 1, 0)
    res = {"warmup": 1, "reps": a.reps, "unit": "ms", "vocabulary": VOCAB, "n_docs": a.docs, "n_lexemes": len(c["lex_count"])}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    def cast(c):
        return vb.Documents.cast((c["data"], c["lex_off"], c["lex_count"], c["doc_lex"]), c["payload"], seed=SEED)

    sealed = cast(c)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(sealed, 1.2, 0.75))
    del sealed
    resolver = vb.Resolver(gix, 1, 1024, 1024 * 5, 1024 * 5 * 8, seed=SEED)
    dt = gix.bind()
    ring = dt.reranker(resolver, 2, **CAPS, from_index=True)
    unsealed = vb.Documents.empty(payload=True)
    res["index_bytes"], res["doc_terms_bytes_at_bind"], res["reranker_bytes_at_create"] = gix.device_bytes, dt.device_bytes(), ring.device_bytes()
    say("set-up done")
    res["deltas"] = []
    next_ctid = a.docs
    for n_delta in (1, 1000, 100_000):
        new = {k: [] for k in ("append", "append_kernels", "sync", "sync_kernels", "both")}
        old = {k: [] for k in ("index_bind", "documents_bind", "reranker", "sum")}
        for r in range(1 + a.reps):
            delta = cast(corpus(n_delta, 100 + next_ctid % 9973, next_ctid))
            next_ctid += n_delta
            t0 = time.perf_counter()
            dt.append_documents(delta, resolver)
            t1 = time.perf_counter()
            ring.sync()
            t2 = time.perf_counter()
            unsealed.extend(delta)
            # the route the library forced before: everything again
            t3 = time.perf_counter()
            again = gix.bind()
            t4 = time.perf_counter()
            tail = unsealed.bind(resolver)
            t5 = time.perf_counter()
            other = again.reranker(resolver, 2, **CAPS, from_index=True)
            t6 = time.perf_counter()
            other.close()
            del again, tail, other
            if r:
                for k, v in (("append", t1 - t0), ("sync", t2 - t1), ("both", t2 - t0), ("append_kernels", debug_ms(vb, "vbm25_debug_append_kernel_ms")),
                             ("sync_kernels", debug_ms(vb, "vbm25_debug_reranker_sync_ms", ring.h))):
                    new[k].append(v)
                for k, v in (("index_bind", t4 - t3), ("documents_bind", t5 - t4), ("reranker", t6 - t5), ("sum", t6 - t3)):
                    old[k].append(v)
        row = {"delta_docs": n_delta, "docs_after": dt.n_docs, "unsealed_after": unsealed.n_docs, "new_route_ms": {k: ms(v) for k, v in new.items()},
               "old_route_ms": {k: ms(v) for k, v in old.items()}, "doc_terms_bytes": dt.device_bytes(), "reranker_bytes": ring.device_bytes(),
               "reranker_allocations": ring.allocations()}
        margin = row["old_route_ms"]["sum"]["median"] - row["new_route_ms"]["both"]["median"]
        spread = row["old_route_ms"]["sum"]["max"] - row["old_route_ms"]["sum"]["min"]
        row["margin_ms"], row["old_route_spread_ms"] = round(margin, 4), round(spread, 4)
        row["verdict"] = "gain shown" if margin > 3 * spread else "no gain measured"
        res["deltas"].append(row)
        say(f"delta of {n_delta} done: {row['verdict']}")
        save()
    # the rerank by ctid on the grown handle and on a freshly built one
    rng = np.random.default_rng(5)
    queries = [[b"%d" % i for i in rng.choice(VOCAB, 5, replace=False)] for _ in range(1024)]
    q_cand = (np.arange(1025) * 1000).astype(np.uint64)
    flat = rng.integers(0, next_ctid, 1024 * 1000).astype(np.uint64)
    tids = np.stack([(flat >> 32) & 0xFFFF, (flat >> 16) & 0xFFFF, flat & 0xFFFF], axis=1).astype(np.uint16)

    def rerank(r):
        r.submit(queries, 10, q_cand, cand_tid=tids)
        return r.collect()

    t_grown, rows_grown = timed(lambda: rerank(ring), 2, max(a.reps, 15))
    fresh = gix.bind()
    fresh.append_documents(unsealed, resolver)
    with fresh.reranker(resolver, 2, **CAPS, from_index=True) as fresh_ring:
        t_fresh, rows_fresh = timed(lambda: rerank(fresh_ring), 2, max(a.reps, 15))
    if rows_grown[0].tobytes() != rows_fresh[0].tobytes() or not rows_grown[1].any():
        raise SystemExit("the grown and the fresh handle rerank differently")
    res["rerank_1024x1000_k10_by_ctid_ms"] = {"grown": t_grown, "fresh": t_fresh, "difference_ms": round(t_grown["median"] - t_fresh["median"], 4),
                                              "fresh_spread_ms": round(t_fresh["max"] - t_fresh["min"], 4)}
    save()
    del fresh
    resolver.submit(queries)
    term_ids, q_off = resolver.collect()
    res["stream"] = stream_beside(vb, gix, resolver, term_ids, q_off, cast)
    say("stream done")
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
