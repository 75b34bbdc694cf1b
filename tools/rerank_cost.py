#!/usr/bin/env python3
"""rerank_cost.py -- what the rerank step costs on one MI355X: a Scorer's top-k (vbm25_scorer_topk: score and select fused, k rows a
query over the link) and its evaluate (vbm25_scorer_evaluate: the handle's buffers kept), beside the route without a scorer in the
same process on the same inputs: DocTerms.evaluate (vbm25_evaluate_documents: every score over the link, buffers made and freed per
call) and a stable top-k per query in numpy on the host.  The two routes' rows are compared byte for byte before a time is reported.
  shapes    those of tools/evaluate_cost.py: 1024 queries x 5 lexemes, 1000 candidates each, out of --docs documents (default
            1 000 000) of log-normal length 100, k = 10 and k = 100; the same out of --docs-long documents (default 100 000) of mean
            length 1000; 64 x 5 as a cross product over the first 100 000 documents of the first corpus.
  times     host clock around synchronous calls, --warmup untimed and --reps timed repetitions (5 and 30), median / min / max; the
            scorer's times are of second and later calls (the first one allocates).  Kernel times by HIP events
            (vbm25_debug_rerank_kernel_ms, vbm25_debug_evaluate_kernel_ms).  Bytes over the link each way from the call's arrays.
  verdict   per shape and k: the parent route's median minus Scorer.topk's, and whether that margin exceeds three times the parent
            route's own spread (max - min) in this run.
Writes one JSON object to the path given first.  One process on the GPU; run it under a timeout.

  python tools/rerank_cost.py profiles/rerank_cost.json [--docs 1000000] [--docs-long 100000] [--reps 30] [--warmup 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cast_cost import SEED, VOCAB, make_corpus, ms, timed, vocabulary  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def debug_ms(vb, name):
    f = getattr(vb.lib(), name)
    f.argtypes = [C.c_void_p, C.c_void_p]
    x, y = C.c_double(), C.c_double()
    vb._lib.check(f(C.byref(x), C.byref(y)))
    return x.value / 1e3, y.value / 1e3


def host_topk(vb, scores, q_cand, cand_doc, k):
    """np.argsort(-scores, kind="stable")[:k] per query, all queries in one call (the lists here have one length) -> (ranks, n_ranks)"""
    nq = len(scores) if q_cand is None else len(q_cand) - 1
    rows = scores.reshape(nq, -1)
    order = np.argsort(-rows, axis=1, kind="stable")[:, :k]
    n = order.shape[1]
    ranks, n_ranks = np.zeros((nq, k), dtype=vb.RANK_DTYPE), np.full(nq, n, dtype=np.uint32)
    ranks["score"][:, :n] = np.take_along_axis(rows, order, axis=1)
    ranks["pos"][:, :n] = order
    ranks["doc"][:, :n] = order if q_cand is None else np.take_along_axis(cand_doc.reshape(nq, -1), order, axis=1)
    return ranks, n_ranks


def run(vb, name, h, gix, nq, n_lex, n_cand, ks, a, rng, parts):
    """n_cand == None: the cross product"""
    res = {"shape": name, "n_docs": h.n_docs, "queries": nq, "query_lexemes": n_lex, "candidates_per_query": n_cand if n_cand else h.n_docs}
    resolver = vb.Resolver(gix, 1, nq, nq * n_lex, nq * n_lex * 8, seed=SEED)
    resolver.submit([[b"%d" % i for i in rng.choice(VOCAB, n_lex, replace=False)] for _ in range(nq)])
    term_ids, q_off = resolver.collect()
    dt = h.bind(resolver)
    if n_cand:
        q_cand = (np.arange(nq + 1) * n_cand).astype(np.uint64)
        cand_doc = rng.integers(0, h.n_docs, nq * n_cand).astype(np.uint32)
    else:
        q_cand, cand_doc = None, None
    pairs = nq * (n_cand if n_cand else h.n_docs)
    up = 4 * len(term_ids) + 4 * (nq + 1) + (8 * (nq + 1) + 4 * pairs if n_cand else 0)
    res["pairs"] = pairs
    kernels = []

    def plain():
        s = dt.evaluate(term_ids, q_off, q_cand, cand_doc)
        kernels.append(debug_ms(vb, "vbm25_debug_evaluate_kernel_ms")[1])
        return s

    t_plain, scores = timed(plain, a.warmup, a.reps)
    res["doc_terms_evaluate"] = {"end_to_end_ms": t_plain, "kernel_ms": ms(kernels[a.warmup:]),
                                 "link_bytes": {"up": up + 4 * (nq + 1), "down": 8 * pairs}}
    say(f"{name}: DocTerms.evaluate done")
    with dt.scorer() as sc:
        kernels.clear()

        def kept():
            s = sc.evaluate(term_ids, q_off, q_cand, cand_doc)
            kernels.append(debug_ms(vb, "vbm25_debug_rerank_kernel_ms")[0])
            return s

        t_kept, again = timed(kept, a.warmup, a.reps)
        if not np.array_equal(again.view(np.uint64), scores.view(np.uint64)):
            raise SystemExit(f"{name}: Scorer.evaluate's scores differ")
        res["scorer_evaluate"] = {"end_to_end_ms": t_kept, "kernel_ms": ms(kernels[a.warmup:]),
                                  "link_bytes": {"up": up + 4 * (nq + 1), "down": 8 * pairs}}
        say(f"{name}: Scorer.evaluate done")
        res["topk"] = []
        for k in ks:
            t_parent, want = timed(lambda: host_topk(vb, dt.evaluate(term_ids, q_off, q_cand, cand_doc), q_cand, cand_doc, k), 2, a.reps)
            t_host, _ = timed(lambda: host_topk(vb, scores, q_cand, cand_doc, k), 1, 5)
            kernels.clear()

            def fused():
                r = sc.topk(term_ids, q_off, k, q_cand, cand_doc)
                kernels.append(debug_ms(vb, "vbm25_debug_rerank_kernel_ms")[1])
                return r

            t_topk, got = timed(fused, a.warmup, a.reps)
            if got[0].tobytes() != want[0].tobytes() or not np.array_equal(got[1], want[1]):
                raise SystemExit(f"{name}: the two routes' top-{k} rows differ")
            margin, spread = t_parent["median"] - t_topk["median"], t_parent["max"] - t_parent["min"]
            entry = {"k": k, "parent_evaluate_plus_host_topk_ms": t_parent, "host_topk_alone_ms": t_host, "scorer_topk_end_to_end_ms": t_topk,
                     "scorer_topk_kernels_ms": ms(kernels[a.warmup:]),
                     "link_bytes": {"up": up + 8 * (nq + 1) + 72, "down": 16 * nq * k + 4 * nq, "parent_down": 8 * pairs},
                     "margin_ms": round(margin, 4), "parent_spread_ms": round(spread, 4), "margin_exceeds_3_spreads": bool(margin > 3 * spread)}
            if k == ks[0]:  # the part size: candidates a workgroup, the queries' lists split and merged below it
                sweep = {}
                for part in parts:
                    vb.set_tuning("rerank_part", part)
                    kernels.clear()
                    t, r = timed(fused, 2, 10)
                    if r[0].tobytes() != want[0].tobytes():
                        raise SystemExit(f"{name}: rerank_part={part} changes the rows")
                    sweep[str(part)] = {"end_to_end_ms": t, "kernels_ms": ms(kernels[2:])}
                vb.reset_tuning()
                entry["rerank_part_sweep"] = sweep
            res["topk"].append(entry)
            say(f"{name}: k={k} done: parent {t_parent['median']} ms, Scorer.topk {t_topk['median']} ms")
        res["scorer_device_bytes"] = sc.device_bytes()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out", nargs="?")
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--docs-long", type=int, default=100_000)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parts", type=int, nargs="*", default=[256, 512, 1024, 4096])
    a = p.parse_args()
    import vectorchord_bm25_amd as vb
    make_corpus.vocab = vocabulary()
    res = {"warmup": a.warmup, "reps": a.reps, "unit": "ms", "vocabulary": VOCAB, "shapes": []}

    def save():  # (after every shape: a job that is cut short keeps what it has)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    def handle(c, n=None):
        n = len(c["doc_lex"]) - 1 if n is None else n
        e = int(c["doc_lex"][n])
        sub = (c["data"][:int(c["lex_off"][e])], c["lex_off"][:e + 1], c["lex_count"][:e], c["doc_lex"][:n + 1])
        return vb.Documents.cast(sub, c["payload"][:n], seed=SEED)

    rng = np.random.default_rng(1)
    for mean, n_docs, clip in ((100, a.docs, 2000), (1000, a.docs_long, 20000)):
        lens = np.clip(np.rint(rng.lognormal(np.log(0.8 * mean), 0.6, n_docs)), 8, clip).astype(np.int64)
        corpus = make_corpus(n_docs, lens, 0.05, seed=3)
        say(f"corpus of {n_docs} documents, {len(corpus['lex_count'])} lexemes made")
        h = handle(corpus)
        gix = vb.GpuIndex(vb.DeviceSegment.from_documents(h, 1.2, 0.75))
        res["shapes"].append(run(vb, f"1024 x 5, 1000 candidates of {n_docs} x log-normal({mean})", h, gix, 1024, 5, 1000, (10, 100), a, rng, a.parts))
        save()
        if mean == 100:
            hc = handle(corpus, min(100_000, n_docs))
            res["shapes"].append(run(vb, f"64 x 5 cross product over {hc.n_docs} x log-normal(100)", hc, gix, 64, 5, None, (10, 100), a, rng, a.parts))
            save()
            del hc
        del h, gix, corpus
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
