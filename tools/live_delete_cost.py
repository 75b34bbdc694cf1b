#!/usr/bin/env python3
"""live_delete_cost.py -- what deletes on a bound handle cost the rerank stack on one MI355X, on the corpus of tools/live_rerank_cost.py
(--docs documents, default 1 000 000, of log-normal length 100 over 30 000 lexemes; the index is DeviceSegment.from_documents of
their cast, the handle GpuIndex.bind, the ring depth 2 from_index).  Two steps, each a process of its own that adds its part to the
JSON file given first:
  --step parent   (a), the yardstick: the 1024 x 1000 rerank at k = 10 by ctid through ANOTHER build of the library -- the parent
                  commit's, given with --library -- which knows no deletion bitmap
  --step new      (a) the same rerank through this build on a handle nobody deleted from.  The claim is "unchanged"; it holds where
                  the two medians differ by less than the parent's own max - min spread.
                  (b) the same rerank with 1 % and with 50 % of the documents dead (DocTerms.delete of random documents).  Reported;
                  there is no threshold.
                  (c) DocTerms.delete_tids of 1, 1000 and 100 000 rows (sealed and unsealed ones, each repetition other rows; the
                  TidSet is made before the clock starts, as the search's deletes make it anyway; its own cost is reported beside)
                  ALTERNATED with the rebuild a delete forced before -- GpuIndex.bind of the index again, Documents.bind of every
                  unsealed row (100 000 of them), a new reranker.  A gain is a margin of more than three times the rebuild's own
                  max - min spread; anything else is "no gain measured".
Host clock around synchronous calls; the reranks 2 untimed and 15 timed, the deletes one untimed and --reps timed (7); median / min /
max.  Every step under its own time limit, the second only after the first:

  timeout -k 10 560 python tools/live_delete_cost.py profiles/live_delete_cost.json --step parent --library <parent's libvbm25.so> && \\
  timeout -k 10 560 python tools/live_delete_cost.py profiles/live_delete_cost.json --step new"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = ("vbm25_doc_terms_delete", "vbm25_doc_terms_delete_tids", "vbm25_doc_terms_dead_docs", "vbm25_doc_terms_read_dead")
N_UNSEALED = 100_000


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def tids_of(flat):
    flat = np.asarray(flat, np.uint64)
    return np.stack([(flat >> 32) & 0xFFFF, (flat >> 16) & 0xFFFF, flat & 0xFFFF], axis=1).astype(np.uint16)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("--step", choices=("parent", "new"), required=True)
    p.add_argument("--library", help="--step parent: the other build of libvbm25.so")
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=7)
    a = p.parse_args()
    if a.reps < 7:
        raise SystemExit("at least 7 repetitions")
    if (a.step == "parent") != bool(a.library):
        raise SystemExit("--library goes with --step parent, and only with it")
    if a.library:
        os.environ["VBM25_LIBRARY"] = os.path.abspath(a.library)  # (read when the package is imported)
    import vectorchord_bm25_amd as vb
    from vectorchord_bm25_amd import _lib
    if a.library:
        for name in NEW_SYMBOLS:  # (the parent's build does not export them, and this step does not call them)
            _lib.ABI.pop(name)
        assert os.path.samefile(vb.library_path(), a.library)
    from cast_cost import SEED, VOCAB, make_corpus, ms, timed, vocabulary
    from live_rerank_cost import CAPS, corpus
    make_corpus.vocab = vocabulary()

    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"unit": "ms", "n_docs": a.docs, "vocabulary": VOCAB, "rerank": "1024 queries of 5 lexemes x 1000 ctids, k = 10, 2 untimed and 15 timed"})

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    def cast(c):
        return vb.Documents.cast((c["data"], c["lex_off"], c["lex_count"], c["doc_lex"]), c["payload"], seed=SEED)

    t0 = time.perf_counter()
    sealed = cast(corpus(a.docs, 1, 0))
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(sealed, 1.2, 0.75))
    del sealed
    resolver = vb.Resolver(gix, 1, 1024, 1024 * 5, 1024 * 5 * 8, seed=SEED)
    dt = gix.bind()
    ring = dt.reranker(resolver, 2, **CAPS, from_index=True)
    say(f"set-up done in {time.perf_counter() - t0:.1f} s")
    rng = np.random.default_rng(5)
    queries = [[b"%d" % i for i in rng.choice(VOCAB, 5, replace=False)] for _ in range(1024)]
    q_cand = (np.arange(1025) * 1000).astype(np.uint64)
    tids = tids_of(rng.integers(0, a.docs, 1024 * 1000))

    def rerank(r):
        r.submit(queries, 10, q_cand, cand_tid=tids)
        return r.collect()

    # (a)
    t, rows = timed(lambda: rerank(ring), 2, 15)
    if not rows[1].any():
        raise SystemExit("the rerank found no row")
    part = res.setdefault("rerank_without_a_bitmap_ms", {})
    part[a.step] = dict(t, library_sha256_16=__import__("hashlib").sha256(open(vb.library_path(), "rb").read()).hexdigest()[:16],
                        rows_crc32=__import__("zlib").crc32(rows[0].tobytes()))
    if "parent" in part and "new" in part:
        spread = part["parent"]["max"] - part["parent"]["min"]
        diff = part["new"]["median"] - part["parent"]["median"]
        part["new_minus_parent_ms"], part["parent_spread_ms"] = round(diff, 4), round(spread, 4)
        part["verdict"] = "unchanged" if abs(diff) < spread else "a difference beyond the parent's spread"
        part["same_rows"] = part["parent"]["rows_crc32"] == part["new"]["rows_crc32"]
    save()
    say(f"(a) {a.step}: {t}")
    if a.step == "parent":
        return
    res["doc_terms_bytes_at_bind"] = dt.device_bytes()  # (no bitmap: nobody deleted from the handle)

    # (c) on this handle, grown by the unsealed rows; (b) afterwards on a handle of its own
    unsealed = cast(corpus(N_UNSEALED, 77, a.docs))
    dt.append_documents(unsealed, resolver)
    ring.sync()
    n_rows = a.docs + N_UNSEALED
    order = rng.permutation(n_rows)
    at = 0
    res["delete_tids"] = []
    for n_delete in (1, 1000, 100_000):
        new = {k: [] for k in ("tid_set", "delete_tids")}
        old = {k: [] for k in ("index_bind", "documents_bind", "reranker", "sum")}
        for r in range(1 + a.reps):
            rows_gone = tids_of(order[at:at + n_delete])
            at += n_delete
            t0 = time.perf_counter()
            ts = vb.TidSet(rows_gone)
            t1 = time.perf_counter()
            n_new = dt.delete_tids(ts)
            t2 = time.perf_counter()
            ts.close()
            if n_new != n_delete:
                raise SystemExit(f"{n_new} rows died, {n_delete} were named")
            # the route a delete forced before: everything again
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
                new["tid_set"].append(t1 - t0)
                new["delete_tids"].append(t2 - t1)
                for k, v in (("index_bind", t4 - t3), ("documents_bind", t5 - t4), ("reranker", t6 - t5), ("sum", t6 - t3)):
                    old[k].append(v)
        row = {"rows_deleted": n_delete, "docs": dt.n_docs, "unsealed": N_UNSEALED, "dead_after": dt.dead_docs,
               "new_route_ms": {k: ms(v) for k, v in new.items()}, "old_route_ms": {k: ms(v) for k, v in old.items()},
               "doc_terms_bytes": dt.device_bytes(), "reranker_allocations": ring.allocations()}
        margin = row["old_route_ms"]["sum"]["median"] - row["new_route_ms"]["delete_tids"]["median"]
        spread = row["old_route_ms"]["sum"]["max"] - row["old_route_ms"]["sum"]["min"]
        row["margin_ms"], row["old_route_spread_ms"] = round(margin, 4), round(spread, 4)
        row["verdict"] = "gain shown" if margin > 3 * spread else "no gain measured"
        res["delete_tids"].append(row)
        say(f"(c) {n_delete} rows: {row['new_route_ms']['delete_tids']} against {row['old_route_ms']['sum']}: {row['verdict']}")
        save()
    ring.close()
    del dt, unsealed

    # (b)
    dt = gix.bind()
    res["rerank_with_dead_documents_ms"] = []
    with dt.reranker(resolver, 2, **CAPS, from_index=True) as ring:
        order = rng.permutation(a.docs)
        for fraction in (0.01, 0.5):
            dt.delete(order[:int(fraction * a.docs)])
            t, rows = timed(lambda: rerank(ring), 2, 15)
            res["rerank_with_dead_documents_ms"].append(dict(t, dead_fraction=fraction, dead_docs=dt.dead_docs, ranks=int(rows[1].sum()),
                                                             doc_terms_bytes=dt.device_bytes()))
            say(f"(b) {fraction}: {t}")
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
