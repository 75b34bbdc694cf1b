"""bigk_scan_win_kernel (sparse queries at k > 1024: the candidate scan fed from the window planes, switch bigk_win) through the C ABI.
Every case checks three things: the records against the oracle's brute force, byte-for-byte equality with the same batch under
bigk_win=0 (bigk_scan_kernel) and under bigk_sparse=0 (the per-query path), and debug_bigk_win() = (items of the window scan, items of
the block scan, slow-path tiles, wide postings decoded).  Every batch runs twice: the second run finds the LDS-clean state and the
cursors of the first.  4 x 65536 + 5 documents: five windows, the last of five documents, so a term with one posting has no window
table.  Segments are built posting by posting.  -m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from growing_data import make_growing
from lifecycle_data import Expect, check, from_rows

pytestmark = pytest.mark.gpu
WIN = 65536
N = 4 * WIN + 5
KS = [1025, 4097]
_C = {}

THIN = list(range(16))            # 700 random documents each, over all windows: a tile spans several windows
BOUND, CROWD = 16, 17             # both sides of every window boundary, 0 and N - 1 | 4500 documents in window 1: halving
WASTE = list(range(18, 34))       # 7 postings in window 0 and 250 in window 2: 4000 postings in 16 x 33 = 528 chunks
ENDS, ONE, WIDE = 34, 35, 36      # the first and the tail window only | one posting: no table | tf = 300 and 70 000
AROUND = 37                       # per k of KS: terms of k - 1, k and k + 1 documents


def corpus():
    """(segment, GpuIndex, Expect), made once"""
    if "main" not in _C:
        rng = np.random.default_rng(5)
        pick = lambda lo, hi, c: np.sort(rng.choice(np.arange(lo, hi), c, replace=False))
        rows = [pick(0, N, 700) for _ in THIN]
        rows += [np.concatenate([[0], *[[c - 1, c, c + 1] for c in range(WIN, N, WIN)], [N - 1]]), pick(WIN, 2 * WIN, 4500)]
        rows += [np.r_[pick(0, WIN, 7), pick(2 * WIN, 3 * WIN, 250)] for _ in WASTE]
        rows += [np.r_[pick(0, WIN, 300), np.arange(N - 5, N)], np.array([70000]), pick(0, N, 200)]
        rows += [pick(0, N, k + d) for k in KS for d in (-1, 0, 1)]
        tfs = [rng.integers(1, 5, len(r)) for r in rows]
        # a full block (postings 0 .. 127) and the short last block (128 .. 199); the pair neighbours 51, 100, 134, 149 stay narrow
        tfs[WIDE][[50, 101, 135, 148]] = [300, 70000, 70000, 300]
        keys = np.zeros((len(rows), 16), np.uint8)
        keys[:, 0] = np.arange(len(rows)) + 1
        seg = vb.Segment.build(1.2, 0.75, rng.integers(5, 300, N).astype(np.uint32), rng.integers(0, 65535, (N, 3)).astype(np.uint16), keys,
                               np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint64), np.concatenate(rows).astype(np.uint32),
                               np.concatenate(tfs).astype(np.uint32))
        _C["main"] = (seg, vb.GpuIndex(seg), Expect(seg))
    return _C["main"]


def three_ways(tuning, gix, want, rows, k, new=None, setup=None):
    """`want` and equal bytes from two runs each under `new`, bigk_win=0 and bigk_sparse=0; returns the first's counters and paths"""
    terms, off = from_rows(rows)
    out, seen = [], None
    for t in (dict(new or {}), dict(new or {}, bigk_win=0), dict(new or {}, bigk_sparse=0)):
        vb.reset_tuning()
        tuning(**t)
        b = vb.Batch(gix, len(rows), max(1, len(terms)), k)
        if setup:
            setup(b)
        b.set_queries(terms, off)
        for rep in range(2):
            b.run()
            hits, nh = b.fetch()
            check(want, hits, nh, f"k={k} {t} run {rep}")
            stats = b.debug_bigk_win()
            print(f"k={k} {t} run {rep}: (window items, block items, slow tiles, wide decoded) {stats}, paths {b.bigk_queries()}")
            assert seen is None or stats[0] == 0 and stats[2:] == (0, 0), stats
            out.append(b"".join(hits[q, :nh[q]].tobytes() for q in range(len(nh))))
        seen = seen or (stats, b.bigk_queries())
    assert len(set(out)) == 1, "the records' bytes differ between runs or between the three paths"
    return seen


@pytest.mark.parametrize("k", KS)
def test_candidates_around_k(tuning, k):
    seg, gix, ex = corpus()
    a = AROUND + 3 * KS.index(k)
    rows = [[a], [a + 1], [a + 2], [a, a + 1, a + 2]]
    stats, paths = three_ways(tuning, gix, ex.plain(*from_rows(rows), k), rows, k)
    assert stats == (20, 0, 0, 0) and paths == (4, 0), (stats, paths)  # (five windows a query, one an item)


@pytest.mark.parametrize("item_win", [1, 1 << 20], ids=["one_window_an_item", "uncut"])
@pytest.mark.parametrize("tile", [1, 0], ids=["tile_1", "tile_max"])
@pytest.mark.parametrize("crowded", [False, True])
def test_tiles(tuning, tile, item_win, crowded):
    """thin terms over all windows, the window boundaries and a query of the first and the tail window (no slow-path tile); 4500
    postings in one window, and 528 chunks of 4000 postings through the alignment waste alone (each halves its window)"""
    seg, gix, ex = corpus()
    rows = [[CROWD], WASTE, [THIN[1], CROWD]] if crowded else [THIN[0:5], [BOUND], [THIN[0], BOUND], [ENDS], THIN]
    stats, paths = three_ways(tuning, gix, ex.plain(*from_rows(rows), 1025), rows, 1025, dict(bigk_win_tile=tile, bigk_item_win=item_win))
    assert stats[:2] == (len(rows) * (5 if item_win == 1 else 1), 0) and paths == (len(rows), 0), (stats, paths)
    assert (stats[2] > 0) == crowded and stats[3] == 0, stats


def test_wide_tf(tuning):
    """tf = 300 and tf = 70 000 in a full block and in the term's short last block: decoded in place, the four postings and their
    pair neighbours (a zero word covers the pair) in each of the two queries"""
    seg, gix, ex = corpus()
    rows = [[WIDE], [THIN[0], WIDE]]
    stats, _ = three_ways(tuning, gix, ex.plain(*from_rows(rows), 1025), rows, 1025)
    assert stats == (10, 0, 0, 16), stats
    stats, _ = three_ways(tuning, gix, ex.plain(*from_rows([[THIN[0]]]), 1025), [[THIN[0]]], 1025)
    assert stats == (5, 0, 0, 0), stats


def test_filters(tuning):
    """selector none, every second document, and a bitmap that rejects the unfiltered top k"""
    seg, gix, ex = corpus()
    rows, k = [THIN[0:3]] * 3, 1025
    terms, off = from_rows(rows)
    keeps = np.ones((2, N), bool)
    keeps[0] = np.arange(N) % 2 == 0
    keeps[1, ex.plain(terms[:3], off[:2], k)[0]["doc_id"].astype(np.int64)] = False
    sel = np.array([vb.NO_FILTER, 0, 1], np.uint32)
    f = vb.DocFilter(gix, keeps)
    stats, _ = three_ways(tuning, gix, ex.filtered(terms, off, k, keeps, sel), rows, k, setup=lambda b: b.set_filter(f, sel))
    assert stats[:2] == (15, 0), stats


def test_mixed_batch(tuning):
    """several chunks; an empty query, a table-less term and 17 terms (the block scan, 33 windows of 8192 documents each), one above
    bigk_cand_max (the per-query path), and three window-scan queries"""
    seg, gix, ex = corpus()
    rows = [[], [THIN[0], ONE], THIN + [BOUND], THIN[0:12] + [CROWD], [THIN[0]], [THIN[1], THIN[2]], [AROUND]]
    stats, paths = three_ways(tuning, gix, ex.plain(*from_rows(rows), 1025), rows, 1025, dict(bigk_cand_max=12000, bigk_chunk_cand=12000))
    assert stats[:2] == (15, 66) and paths == (6, 1), (stats, paths)


@pytest.mark.parametrize("gate", ["min_docs", "win_planes", "id16_plane"])
def test_gates(tuning, gate):
    seg, gix, ex = corpus()
    new = {}
    if gate == "min_docs":
        new = dict(bigk_win_min_docs=N + 1)
    else:
        tuning(**{gate: 0})
        gix = vb.GpuIndex(seg)
    rows = [THIN[0:3], [BOUND]]
    stats, paths = three_ways(tuning, gix, ex.plain(*from_rows(rows), 1025), rows, 1025, new)
    assert stats[0] == 0 and stats[1] > 0 and stats[2:] == (0, 0) and paths == (2, 0), (stats, paths)


def test_growing_merge(tuning):
    seg, gix, ex = corpus()
    terms, off = from_rows([THIN[0:2], [BOUND], [], [CROWD, WIDE]])
    G, _ = make_growing(seg.arrays()["term_key"], 300, seed=3, pool=terms, pool_p=0.4)
    out = []
    for t in ({}, dict(bigk_win=0), dict(bigk_sparse=0)):
        vb.reset_tuning()
        tuning(**t)
        hits, nh = vb.search_batch_growing(gix, vb.GrowingSegment(gix, **G), terms, off, 1025)
        check(ex.growing(terms, off, 1025, G), hits, nh, f"growing {t}")
        out.append([hits[q, :nh[q]].tobytes() for q in range(len(nh))])
    assert out[0] == out[1] == out[2]
