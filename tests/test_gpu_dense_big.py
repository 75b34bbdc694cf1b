"""scan_dense_kernel<1024> (256 < k <= 1024: the dense window scan with one survivor list per workgroup in LDS, switch dense_big)
through the C ABI.  Every case compares three things bit for bit: the oracle's brute force, the same batch under dense_big=0 (every
query through scan_many_kernel: the parent's route) and the new route; on the new route debug_routes()[4] counts the items that went
to the new kernel.
tuning(dense_x1000=0, dense_big_min_docs=0) declares every query dense and opens the route to small corpora.  -m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from growing_data import make_growing
from lifecycle_data import Expect, built, check, from_rows, rows_of

pytestmark = pytest.mark.gpu
_C = {}


def zipf_corpus():
    """make_corpus(20000, 2000), lognormal lengths and Zipf(1) tokens: (corpus, segment, GpuIndex, Expect), made once"""
    if "zipf" not in _C:
        c = make_corpus(20000, 2000, seed=7, length="lognormal", mean_len=60, zipf=1.0)
        seg = built(c)
        _C["zipf"] = (c, seg, vb.GpuIndex(seg), Expect(seg))
    return _C["zipf"]


def three_ways(tuning, gix, want, terms, off, k, new, runs=1, setup=None, served=True, failed=None):
    """`want` from the new route (tuning `new` on top of dense_big=1) on every one of `runs` runs of one batch, and the same bytes from
    dense_big=0; returns the new route's batch"""
    out, seen = [], {}
    for big in (1, 0):
        vb.reset_tuning()
        tuning(dense_big_min_docs=0, dense_x1000=0)
        tuning(**dict(new, dense_big=big))
        b = vb.Batch(gix, len(off) - 1, max(1, len(terms)), k)
        if setup:
            setup(b)
        b.set_queries(terms, off)
        for rep in range(runs if big else 1):
            b.run()
            hits, nh = b.fetch()
            check(want, hits, nh, f"k={k} dense_big={big} run {rep}")
            routes, counts = b.debug_routes(), b.debug_counts()
            print(f"k={k} dense_big={big} run {rep}: routes {routes}, (items, given up) {counts}")
            seen[big] = (routes, counts)
            if big and failed is not None:
                assert counts[1] == failed, f"{counts[1]} of {counts[0]} items were given up"
            out.append(b"".join(hits[q, :nh[q]].tobytes() for q in range(len(nh))))
        if big:
            new_batch = b
    assert len(set(out)) == 1, "the records' bytes differ between runs or between dense_big=1 and dense_big=0"
    # (the parent's route counts dense queries' items in [4] too, tests/work_items_model.py: "not served" = exactly dense_big=0's items)
    if served:
        assert seen[1][0][4] > 0, seen
    else:
        assert seen[1] == seen[0], seen
    return new_batch


@pytest.mark.parametrize("k", [257, 300, 512, 1000, 1024])
def test_parity_over_k(tuning, k):
    """48 queries of 3 to 10 terms (six of each count) at every k"""
    c, seg, gix, ex = zipf_corpus()
    rows = [r for nt in range(3, 11) for r in rows_of(*make_queries(c, 6, nt, seed=9 * k + nt, zipf=1.0))]
    terms, off = from_rows(rows)
    three_ways(tuning, gix, ex.plain(terms, off, k), terms, off, k, {}, failed=0)


@pytest.mark.parametrize("k", [257, 1024])
def test_list_edges(tuning, k):
    """one-term queries with k - 1, k, k + 1, 2k, 2k + 1 and 5k documents: the list first fills, first cuts, cuts more than once.  Then
    b = 0 and tf = 1: every document of a term scores the same, so the k-th place of the two-term query lies in a run of equal scores
    and the doc-id order decides the cut; the 15 000 equal scores of term 0 outrun the buffer between two cuts, and the item is given
    up (the records are asserted, not the count).  The queries are repeated to 258 a batch: one work item a query, the whole index."""
    n = 30_000
    rng = np.random.default_rng(k)
    rows = [np.sort(rng.choice(n, c, replace=False)) for c in (k - 1, k, k + 1, 2 * k, 2 * k + 1, 5 * k)]
    ties = [np.arange(0, n, 2), np.arange(0, n, 50)]
    for name, rows, b, queries in (("counts", rows, 0.75, [[i] for i in range(6)]), ("ties", ties, 0.0, [[0, 1], [0], [1]])):
        docs = np.concatenate(rows).astype(np.uint32)
        tfs = rng.integers(1, 4, len(docs)).astype(np.uint32) if b else np.ones(len(docs), np.uint32)
        keys = np.zeros((len(rows), 16), np.uint8)
        keys[:, 0] = np.arange(len(rows)) + 1
        seg = vb.Segment.build(1.2, b, rng.integers(5, 300, n).astype(np.uint32), np.zeros((n, 3), np.uint16), keys,
                               np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint64), docs, tfs)
        reps = 258 // len(queries)
        terms, off = from_rows(queries * reps)
        want = Expect(seg).plain(*from_rows(queries), k) * reps
        if name == "ties":
            assert want[0]["score"][k - 2] == want[0]["score"][k - 1] and len(want[0]) == k
        b1 = three_ways(tuning, vb.GpuIndex(seg), want, terms, off, k, dict(dense_items=256))
        assert b1.debug_counts()[0] == len(off) - 1


@pytest.mark.parametrize("grid", [1, None])
def test_many_items_share_a_threshold(tuning, grid):
    """every query cut into many items, drawn by one workgroup or by all, three runs of one batch: a stale list, cursor or threshold
    between items or between runs changes the bytes"""
    c, seg, gix, ex = zipf_corpus()
    terms, off = make_queries(c, 12, 6, seed=4, zipf=1.0)
    new = dict(dense_items=256, **(dict(dense_grid=grid) if grid else {}))
    b = three_ways(tuning, gix, ex.plain(terms, off, 300), terms, off, 300, new, runs=3, failed=0)
    assert b.debug_routes()[4] >= 12 * 8


@pytest.mark.parametrize("case", ["mixed", "filter", "growing"])
def test_neighbours(tuning, case):
    c, seg, gix, ex = zipf_corpus()
    k = 300
    df = seg.arrays()["term_df"].astype(np.int64)
    order = np.argsort(-df, kind="stable")
    dense_q, sparse_q, many_q = np.sort(order[:3]), np.sort(order[-2:]), np.sort(order[40:60])
    if case == "mixed":  # dense_x1000 at its default: a sparse, a dense and a 20-term query in one batch
        assert df[sparse_q].sum() * 10 < seg.n_docs <= df[dense_q].sum() * 10
        terms, off = from_rows([sparse_q, dense_q, many_q])
        b = three_ways(tuning, gix, ex.plain(terms, off, k), terms, off, k, dict(dense_x1000=100), failed=0)
        r = b.debug_routes()
        assert r[0] == 1 and r[3] == 0 and r[4] > 0 and r[5] > 0, r  # (items by kernel: the sparse kernels', the new one's, scan_many_kernel's)
        return
    terms, off = make_queries(c, 12, 5, seed=21, zipf=1.0)
    if case == "filter":  # half of the documents rejected: no candidate, no histogram count
        keeps = (np.arange(seg.n_docs) % 2 == 0)[None, :]
        sel = np.zeros(12, np.uint32)
        f = vb.DocFilter(gix, keeps)
        three_ways(tuning, gix, ex.filtered(terms, off, k, keeps, sel), terms, off, k, {}, setup=lambda b: b.set_filter(f, sel))
    else:
        G, _ = make_growing(seg.arrays()["term_key"], 500, seed=3, pool=terms, pool_p=0.4)
        gs = vb.GrowingSegment(gix, **G)
        three_ways(tuning, gix, ex.growing(terms, off, k, G), terms, off, k, {}, setup=lambda b: b.set_growing(gs))


def test_the_gate_keeps_small_indexes_on_the_old_route(tuning):
    """dense_big_min_docs at its default (65536): the 20 000-document index keeps the parent's route -- the work items of dense_big=0,
    not the ones the open gate makes -- with the same records"""
    c, seg, gix, ex = zipf_corpus()
    terms, off = make_queries(c, 12, 5, seed=33, zipf=1.0)
    want = ex.plain(terms, off, 300)
    kept = three_ways(tuning, gix, want, terms, off, 300, dict(dense_big_min_docs=65536), served=False)
    opened = three_ways(tuning, gix, want, terms, off, 300, {})
    assert kept.debug_counts()[0] != opened.debug_counts()[0]
