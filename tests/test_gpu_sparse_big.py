"""scan_sparse_big_kernel (sparse queries at 256 < k <= 1024: the rank-addressed window scan, switch sparse_big) through the C ABI.
Every case compares three things bit for bit: the oracle's brute force, the same batch under sparse_big=0 (scan_many_kernel: the
parent's route) and the new route, where debug_sparse_big()[0] counts the items the new kernel took.  The corpus is 3 x 2^16 + 5
documents -- three full windows and a tail of five -- with one term (or group of terms) per property; tuning(sparse_big_min_docs=0)
opens the gate where a case uses a smaller index.  -m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from growing_data import make_growing
from lifecycle_data import Expect, check, from_rows

pytestmark = pytest.mark.gpu
N = 3 * 65536 + 5
_C = {}

# term ids of the main corpus
SP = list(range(16))             # 16 sparse terms, 700 random documents each
ONE, TAIL = 16, 17               # 3000 random documents | the five documents of the tail
CUT = [18, 19]                   # 9500 random documents each: 19 000 postings, under 0.1 N, two work items cut inside window 1
CROWD = 20                       # 4500 documents, all in window 0: more than a tile's 4096 postings
WASTE = list(range(21, 37))      # 16 terms with 7 postings in window 0 and 250 in window 1: 4000 postings in 16 x 33 = 528 chunks
WIDE, DENSE, N_TERMS = 37, 38, 39  # 900 documents, one with tf = 300 | 25 000 documents: a dense query


def segment(rows, tfs, b, n=N, seed=1):
    rng = np.random.default_rng(seed)
    keys = np.zeros((len(rows), 16), np.uint8)
    keys[:, 0] = np.arange(len(rows)) + 1
    return vb.Segment.build(1.2, b, rng.integers(5, 300, n).astype(np.uint32), rng.integers(0, 65535, (n, 3)).astype(np.uint16), keys,
                            np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint64), np.concatenate(rows).astype(np.uint32),
                            np.concatenate(tfs).astype(np.uint32))


def main_corpus():
    """(segment, GpuIndex, Expect), made once"""
    if "main" not in _C:
        rng = np.random.default_rng(5)
        pick = lambda lo, hi, c: np.sort(rng.choice(np.arange(lo, hi), c, replace=False))
        rows = [pick(0, N, 700) for _ in SP] + [pick(0, N, 3000), np.arange(N - 5, N)]
        rows += [pick(0, N, 9500) for _ in CUT] + [pick(0, 65536, 4500)]
        rows += [np.r_[pick(0, 65536, 7), pick(65536, 131072, 250)] for _ in WASTE]
        rows += [pick(0, N, 900), pick(0, N, 25000)]
        tfs = [rng.integers(1, 5, len(r)) for r in rows]
        tfs[WIDE][450] = 300
        seg = segment(rows, tfs, 0.75)
        assert seg.n_terms == N_TERMS
        _C["main"] = (seg, vb.GpuIndex(seg), Expect(seg))
        _C["cut_docs"] = rows[CUT[0]]
    return _C["main"]


def three_ways(tuning, gix, want, rows, k, new=None, runs=1, setup=None, taken="all", given_up=0):
    """`want` and equal bytes from every run on the new route and from sparse_big=0; taken: the new kernel's items -- "all", ">0" or 0"""
    terms, off = from_rows(rows)
    out = []
    for on in (1, 0):
        vb.reset_tuning()
        tuning(sparse_big_min_docs=0)
        tuning(**dict(new or {}, sparse_big=on))
        b = vb.Batch(gix, len(rows), max(1, len(terms)), k)
        if setup:
            setup(b)
        b.set_queries(terms, off)
        for rep in range(runs if on else 1):
            b.run()
            hits, nh = b.fetch()
            check(want, hits, nh, f"k={k} sparse_big={on} run {rep}")
            stats, counts = b.debug_sparse_big(), b.debug_counts()
            print(f"k={k} sparse_big={on} run {rep}: (taken, given up, slow tiles, cuts) {stats}, (items, given up) {counts}, routes {b.debug_routes()}")
            if not on or taken == 0:
                assert stats == (0, 0, 0, 0), stats
            else:
                assert stats[0] == counts[0] if taken == "all" else stats[0] > 0, (stats, counts)
                assert stats[1] == given_up and counts[1] == given_up, (stats, counts)
            out.append(b"".join(hits[q, :nh[q]].tobytes() for q in range(len(nh))))
        if on:
            new_batch = b
    assert len(set(out)) == 1, "the records' bytes differ between runs or between sparse_big=1 and sparse_big=0"
    return new_batch


@pytest.mark.parametrize("k", [257, 512, 1000, 1024])
@pytest.mark.parametrize("nt", [1, 2, 8, 16])
def test_windows(tuning, k, nt):
    """queries of 1, 2, 8 and 16 terms over three full windows and the tail; the few matches: a query of the tail's five documents and
    one that matches fewer than k; no match: ids the index does not hold (no work item)"""
    seg, gix, ex = main_corpus()
    rows = {1: [[ONE], [SP[3]], [TAIL]], 2: [SP[0:2], [SP[5], ONE], [SP[7], TAIL]], 8: [SP[0:8], SP[8:16]], 16: [SP, WASTE]}[nt]
    rows = rows + [[N_TERMS + 3, N_TERMS + 9]]
    want = ex.plain(*from_rows(rows), k)
    assert len(want[-1]) == 0 and (nt > 1 or len(want[2]) == 5)
    b = three_ways(tuning, gix, want, rows, k)
    assert b.debug_sparse_big()[3] >= b.debug_sparse_big()[0]  # (every item ends with a cut)


def test_item_cuts_and_crowded_windows(tuning):
    """19 000 postings: two items, cut inside window 1 with postings on both sides, and 6333 postings a window: tiles on the slow path.
    4500 postings in one window, and 528 chunks of 4000 postings through the alignment waste alone: each halves its window."""
    seg, gix, ex = main_corpus()
    for rows, items in (([CUT], 2), ([[CROWD]], 1), ([WASTE], 1)):
        terms, off = from_rows(rows)
        b = three_ways(tuning, gix, ex.plain(terms, off, 1000), rows, 1000)
        assert b.debug_counts()[0] == items and b.debug_sparse_big()[2] > 0, (rows, b.debug_counts(), b.debug_sparse_big())
    d = _C["cut_docs"]
    assert (d < N // 2).any() and ((d >= N // 2) & (d < 131072)).any()  # postings of window 1 on both sides of the cut


@pytest.mark.parametrize("k", [257, 1024])
def test_ties(tuning, k):
    """b = 0 and tf = 1: every document of a term scores the same.  17 874 of them in two items, 5958 a window: every sweep round holds
    1024 equal scores, every cut falls inside the run, and the document order alone decides the k that stay"""
    if "ties" not in _C:
        rows = [np.arange(3, N, 11), np.arange(0, N, 400)]
        seg = segment(rows, [np.ones(len(r), np.int64) for r in rows], 0.0)
        _C["ties"] = (seg, vb.GpuIndex(seg), Expect(seg))
    seg, gix, ex = _C["ties"]
    rows = [[0], [0, 1], [1]]
    want = ex.plain(*from_rows(rows), k)
    assert want[0]["score"][0] == want[0]["score"][k - 1] and np.array_equal(want[0]["doc_id"], np.arange(3, N, 11)[:k])
    b = three_ways(tuning, gix, want, rows, k)
    assert b.debug_counts()[0] == 5 and b.debug_sparse_big()[3] > 10


def test_wide_tf_gives_the_item_up(tuning):
    """one posting with tf = 300 (a zero byte in post_tfn): its item goes to scan_many_kernel, the records are the same"""
    seg, gix, ex = main_corpus()
    rows = [[WIDE], [SP[0], SP[1]]]
    three_ways(tuning, gix, ex.plain(*from_rows(rows), 300), rows, 300, given_up=1)


@pytest.mark.parametrize("case", ["no_table", "17_terms", "no_planes", "min_docs"])
def test_gate_and_eligibility(tuning, case):
    """what keeps the parent's route: a term without a window table (one posting in five windows), a 17-term query, an index without
    the window planes, and the default sparse_big_min_docs (65 536) on an index of 30 000 documents -- which the open gate serves"""
    seg, gix, ex = main_corpus()
    k, new = 300, {}
    rows = [SP + [ONE]] if case == "17_terms" else [SP[0:3]]
    if case == "no_table":
        n5 = 4 * 65536 + 1
        seg = segment([np.arange(100, n5, 437), np.array([70000])], [np.ones(600, np.int64), np.ones(1, np.int64)], 0.75, n=n5)
        gix, ex, rows = vb.GpuIndex(seg), Expect(seg), [[0, 1]]
    if case == "no_planes":
        vb.reset_tuning()
        tuning(win_planes=0)
        gix = vb.GpuIndex(seg)
    if case == "min_docs":
        rng = np.random.default_rng(2)
        small = [np.sort(rng.choice(30000, 600, replace=False)) for _ in range(3)]
        seg = segment(small, [rng.integers(1, 4, 600) for _ in small], 0.75, n=30000)
        gix, ex, rows, new = vb.GpuIndex(seg), Expect(seg), [[0, 1, 2]], dict(sparse_big_min_docs=65536)
        three_ways(tuning, gix, ex.plain(*from_rows(rows), k), rows, k)  # (the open gate)
    three_ways(tuning, gix, ex.plain(*from_rows(rows), k), rows, k, new, taken=0)


@pytest.mark.parametrize("case", ["mixed", "filter", "growing", "three_runs"])
def test_neighbours(tuning, case):
    seg, gix, ex = main_corpus()
    k = 300
    rows = [SP[0:5], [SP[6], ONE], SP[8:12]]
    terms, off = from_rows(rows)
    if case == "mixed":  # a dense query in the batch: scan_dense_kernel<1024> and the new kernel in one run
        rows = rows + [[SP[0], DENSE]]
        b = three_ways(tuning, gix, ex.plain(*from_rows(rows), k), rows, k, taken=">0")
        assert b.debug_routes()[1] == 1 and b.debug_routes()[4] > 0, b.debug_routes()
    elif case == "filter":  # query 0 the even documents, query 1 no bitmap, query 2 every third
        keeps = np.stack([np.arange(N) % 2 == 0, np.arange(N) % 3 == 0])
        sel = np.array([0, vb.NO_FILTER, 1], np.uint32)
        f = vb.DocFilter(gix, keeps)
        three_ways(tuning, gix, ex.filtered(terms, off, k, keeps, sel), rows, k, setup=lambda b: b.set_filter(f, sel))
    elif case == "growing":
        G, _ = make_growing(seg.arrays()["term_key"], 500, seed=3, pool=terms, pool_p=0.4)
        gs = vb.GrowingSegment(gix, **G)
        three_ways(tuning, gix, ex.growing(terms, off, k, G), rows, k, setup=lambda b: b.set_growing(gs))
    else:
        three_ways(tuning, gix, ex.plain(terms, off, k), rows, k, runs=3)
