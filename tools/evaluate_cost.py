#!/usr/bin/env python3
"""evaluate_cost.py -- what the `<&>` operator from cast documents costs on one MI355X: the bind (vbm25_documents_bind), the scoring
kernel alone (HIP events) and vbm25_evaluate_documents end to end, beside the only route to the same scores without them:
Documents.download, vbm25_lookup_terms on the host for every element, and one vbm25_evaluate_batch call per query over that
query's candidates (whose host arrays have to be gathered first).  Same process, same inputs; the two routes' scores are compared bit
for bit before a time is reported.
  shapes    1024 queries x 5 lexemes, 1000 candidates each, out of --docs documents (default 1 000 000) of log-normal length 100
            (tools/cast_cost.py's corpus, 5 % of the lexemes hashed); the same out of --docs-long documents (default 100 000) of mean
            length 1000; 64 x 5 as a cross product over the first 100 000 documents of the first corpus.
  parent    the host route is timed on the first --parent-queries queries of the batch (default 128; the cross product: all 64) and the
            device route on the same sub-batch, so the ratio compares like with like; its one-off preparation (download + lookup) is
            reported apart from the per-batch work (gather + calls).
Host clock around synchronous calls, --warmup untimed and --reps timed repetitions (5 and 30; the parent route --parent-reps after one
untimed), median / min / max.  Writes one JSON object to the path given first.

  python tools/evaluate_cost.py profiles/evaluate_cost.json [--docs 1000000] [--docs-long 100000] [--reps 30] [--warmup 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cast_cost import SEED, VOCAB, make_corpus, ms, timed, vocabulary  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_ms(vb):
    L = vb.lib()
    L.vbm25_debug_evaluate_kernel_ms.argtypes = [C.c_void_p, C.c_void_p]
    b, s = C.c_double(), C.c_double()
    vb._lib.check(L.vbm25_debug_evaluate_kernel_ms(C.byref(b), C.byref(s)))
    return b.value / 1e3, s.value / 1e3


def lookup_all(vb, gix, key):
    """vbm25_lookup_terms for every element's key, straight from the downloaded array"""
    key = np.ascontiguousarray(key, dtype=np.uint8).reshape(-1)
    out = np.zeros(len(key) // 16, dtype=np.uint32)
    vb._lib.check(vb.lib().vbm25_lookup_terms(gix.h, key.ctypes.data, len(out), out.ctypes.data))
    return out


def parent_batch(vb, gix, start, term, tf, term_ids, q_off, lists):
    """one vbm25_evaluate_batch call per query over that query's candidates, their host arrays gathered first"""
    out = []
    for q, cand in enumerate(lists):
        if cand is None:  # (every document: the downloaded arrays as they are)
            out.append(vb.evaluate_batch(gix, term_ids[q_off[q]:q_off[q + 1]], start, term, tf))
            continue
        s, n = start[cand], start[cand + 1] - start[cand]
        ds = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
        idx = np.repeat(s - ds[:-1].astype(np.int64), n) + np.arange(int(ds[-1]), dtype=np.int64)
        out.append(vb.evaluate_batch(gix, term_ids[q_off[q]:q_off[q + 1]], ds, term[idx], tf[idx]))
    return np.concatenate(out) if out else np.zeros(0)


def run(vb, name, h, gix, nq, n_lex, n_cand, a, rng, parent_queries):
    """n_cand == None: the cross product"""
    res = {"shape": name, "n_docs": h.n_docs, "n_elements": h.n_elements, "queries": nq, "query_lexemes": n_lex,
           "candidates_per_query": n_cand if n_cand else h.n_docs}
    resolver = vb.Resolver(gix, 1, nq, nq * n_lex, nq * n_lex * 8, seed=SEED)
    resolver.submit([[b"%d" % i for i in rng.choice(VOCAB, n_lex, replace=False)] for _ in range(nq)])
    term_ids, q_off = resolver.collect()
    binds = []

    def bind():
        dt = h.bind(resolver)
        binds.append(kernel_ms(vb)[0])
        return dt

    t_bind, dt = timed(bind, a.warmup, a.reps)
    res["bind_end_to_end_ms"], res["bind_kernels_ms"] = t_bind, ms(binds[a.warmup:])
    res["n_known"], res["doc_terms_bytes"] = dt.n_known, dt.device_bytes()
    say(f"{name}: bind done")
    if n_cand:
        lists = [rng.integers(0, h.n_docs, n_cand) for _ in range(nq)]
        q_cand = (np.arange(nq + 1) * n_cand).astype(np.uint64)
        cand_doc = np.concatenate(lists).astype(np.uint32)
    else:
        lists, q_cand, cand_doc = [None] * nq, None, None
    kernels = []

    def score(n=nq):
        if q_cand is None:
            s = dt.evaluate(term_ids[:q_off[n]], q_off[:n + 1])
        else:
            s = dt.evaluate(term_ids[:q_off[n]], q_off[:n + 1], q_cand[:n + 1], cand_doc[:int(q_cand[n])])
        kernels.append(kernel_ms(vb)[1])
        return s

    t_eval, scores = timed(score, a.warmup, a.reps)
    res["evaluate_end_to_end_ms"], res["score_kernel_ms"] = t_eval, ms(kernels[a.warmup:])
    pairs = scores.size
    res["pairs"], res["nonzero_pairs"] = pairs, int((scores != 0).sum())
    res["score_kernel_ns_per_pair"] = round(res["score_kernel_ms"]["median"] * 1e6 / pairs, 4)
    # the bisection's dependent loads per pair: per query term ceil(log2(run + 1)) steps (an upper bound: the cursor only shortens them)
    start, _, _ = dt.download()
    run_len = np.diff(start.astype(np.int64))
    steps = np.ceil(np.log2(run_len + 1.0))
    mean_steps = float(steps[cand_doc].mean() if cand_doc is not None else steps.mean())
    res["mean_known_run"], res["bisection_loads_per_pair_bound"] = float(run_len.mean()), round(mean_steps * float(np.diff(q_off.astype(np.int64)).mean()), 2)
    say(f"{name}: evaluate done")
    # the parent route, on the first P queries; the device route on the same sub-batch
    P = min(parent_queries, nq)
    t0 = time.perf_counter()
    dl = h.download(with_length=False)
    t1 = time.perf_counter()
    term = lookup_all(vb, gix, dl["g_key"])
    t2 = time.perf_counter()
    res["parent_prepare_once_ms"] = {"download": round((t1 - t0) * 1e3, 2), "lookup_terms": round((t2 - t1) * 1e3, 2)}
    hs, htf = dl["g_start"].astype(np.int64), dl["g_tf"]
    t_parent, want = timed(lambda: parent_batch(vb, gix, hs, term, htf, term_ids, q_off, lists[:P]), 1, a.parent_reps)
    kernels.clear()
    t_sub, got = timed(lambda: score(P), a.warmup, a.reps)
    if not np.array_equal(got.reshape(-1).view(np.uint64), want.view(np.uint64)):
        raise SystemExit(f"{name}: the two routes' scores differ")
    res["same_sub_batch"] = {"queries": P, "parent_gather_and_calls_ms": t_parent, "evaluate_end_to_end_ms": t_sub,
                             "ratio_parent_over_device": round(t_parent["median"] / t_sub["median"], 2),
                             "ratio_with_prepare_and_bind": round((t_parent["median"] + (t2 - t0) * 1e3) / (t_sub["median"] + t_bind["median"]), 2)}
    say(f"{name}: parent route done")
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out", nargs="?")
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--docs-long", type=int, default=100_000)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parent-reps", type=int, default=3)
    p.add_argument("--parent-queries", type=int, default=128)
    a = p.parse_args()
    import vectorchord_bm25_amd as vb
    make_corpus.vocab = vocabulary()
    res = {"warmup": a.warmup, "reps": a.reps, "parent_reps": a.parent_reps, "unit": "ms", "vocabulary": VOCAB, "shapes": []}

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
        res["shapes"].append(run(vb, f"1024 x 5, 1000 candidates of {n_docs} x log-normal({mean})", h, gix, 1024, 5, 1000, a, rng, a.parent_queries))
        save()
        if mean == 100:
            hc = handle(corpus, min(100_000, n_docs))
            res["shapes"].append(run(vb, f"64 x 5 cross product over {hc.n_docs} x log-normal(100)", hc, gix, 64, 5, None, a, rng, 64))
            save()
            del hc
        del h, gix, corpus
    print(json.dumps(res))


if __name__ == "__main__":
    main()
