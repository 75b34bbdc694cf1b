#!/usr/bin/env python3
"""forward_cost.py -- what the forward index of an index's own documents costs on one MI355X: GpuIndex.bind (vbm25_index_bind: kernels by
HIP events, wall time, device bytes, documents per sort class) beside the route it replaces for an index that arrived without its
tsvectors -- Documents.cast of the whole corpus again and Documents.bind --, and the 1024 x 1000 rerank at k = 10 on both handles,
which read the same four arrays and must take the same time.  Same process, same corpus; the two handles' arrays are compared byte for
byte before a time is reported.
  corpus    --docs documents (default 1 000 000) of log-normal length 100 over 30 000 lexemes, 5 % of them hashed
            (tools/cast_cost.py's corpus); the index is DeviceSegment.from_documents of their cast
  old route Documents.cast (the upload of the lexemes included: that is what the caller has to repeat) + Documents.bind
Host clock around synchronous calls, --warmup untimed and --reps timed repetitions (2 and 7), median / min / max.  Writes one JSON
object to the path given first.

  python tools/forward_cost.py profiles/forward_cost.json [--docs 1000000] [--reps 7] [--warmup 2]"""
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


def bind_stats(vb):
    f = vb.lib().vbm25_debug_forward
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 4
    t, n = C.c_double(), [C.c_uint64() for _ in range(3)]
    vb._lib.check(f(C.byref(t), *[C.byref(x) for x in n]))
    return t.value / 1e3, [x.value for x in n]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out", nargs="?")
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    if a.reps < 5:
        raise SystemExit("at least 5 repetitions")
    import vectorchord_bm25_amd as vb
    make_corpus.vocab = vocabulary()
    rng = np.random.default_rng(1)
    lens = np.clip(np.rint(rng.lognormal(np.log(0.8 * 100), 0.6, a.docs)), 8, 2000).astype(np.int64)
    c = make_corpus(a.docs, lens, 0.05, seed=3)
    packed = (c["data"], c["lex_off"], c["lex_count"], c["doc_lex"])
    say(f"corpus of {a.docs} documents, {len(c['lex_count'])} lexemes made")
    res = {"warmup": a.warmup, "reps": a.reps, "unit": "ms", "vocabulary": VOCAB, "n_docs": a.docs, "n_lexemes": len(c["lex_count"]),
           "lexeme_bytes": len(c["data"])}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    h = vb.Documents.cast(packed, c["payload"], seed=SEED)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(h, 1.2, 0.75))
    resolver = vb.Resolver(gix, 1, 1024, 1024 * 5, 1024 * 5 * 8, seed=SEED)
    res["index_bytes"] = gix.device_bytes
    # the bind from the index
    kernels, classes = [], []

    def from_index():
        dt = gix.bind()
        t, n = bind_stats(vb)
        kernels.append(t)
        classes.append(n)
        return dt

    t_ix, dt_ix = timed(from_index, a.warmup, a.reps)
    res["index_bind"] = {"end_to_end_ms": t_ix, "kernels_ms": ms(kernels[a.warmup:]), "doc_terms_bytes": dt_ix.device_bytes(),
                         "n_known": dt_ix.n_known, "documents_per_class": dict(zip(("wave", "group", "long"), classes[-1]))}
    say("index bind done")
    save()
    # the route it replaces: the corpus cast again, then bound
    del h
    t_cast, h = timed(lambda: vb.Documents.cast(packed, c["payload"], seed=SEED), 1, a.reps)
    t_bind, dt_docs = timed(lambda: h.bind(resolver), 1, a.reps)
    both = {k: round(t_cast[k] + t_bind[k], 4) for k in t_cast}  # (min + min .. max + max: the widest the sum can be)
    res["documents_route"] = {"cast_ms": t_cast, "bind_ms": t_bind, "sum_ms": both, "doc_terms_bytes": dt_docs.device_bytes(),
                              "host_link_bytes": int(len(c["data"]) + 8 * len(c["lex_off"]) + 4 * len(c["lex_count"]) + 4 * len(c["doc_lex"]))}
    for x, y in zip(dt_ix.download(), dt_docs.download()):
        if x.tobytes() != y.tobytes():
            raise SystemExit("the two handles differ")
    margin = both["median"] - t_ix["median"]
    spread = both["max"] - both["min"]
    res["margin_ms"], res["documents_route_spread_ms"] = round(margin, 4), round(spread, 4)
    res["verdict"] = "gain shown" if margin >= 3 * spread else "no gain shown"
    say("documents route done")
    save()
    # the rerank on both handles
    queries = [[b"%d" % i for i in rng.choice(VOCAB, 5, replace=False)] for _ in range(1024)]
    resolver.submit(queries)
    term_ids, q_off = resolver.collect()
    q_cand = (np.arange(1025) * 1000).astype(np.uint64)
    cand_doc = rng.integers(0, a.docs, 1024 * 1000).astype(np.uint32)
    rows = {}
    for name, dt in (("index_bound", dt_ix), ("documents_bound", dt_docs)):
        with dt.scorer() as s:
            t, out = timed(lambda: s.topk(term_ids, q_off, 10, q_cand, cand_doc), a.warmup, max(a.reps, 15))
        res["rerank_1024x1000_k10_" + name + "_ms"] = t
        rows[name] = out
    if rows["index_bound"][0].tobytes() != rows["documents_bound"][0].tobytes():
        raise SystemExit("the two handles rerank differently")
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
