"""The batched path of k > 1024 for dense queries (bigk_dense.h: bigk_dense_scan_kernel's histogram and emit scans,
bigk_dense_walk_kernel, then bigk.hip's select, sort and emit).  As in test_gpu_bigk.py every case checks its records against the
oracle's brute force and byte for byte against the same batch under tuning(bigk_sparse=0), the per-query path; Batch.bigk_queries()
and Batch.debug_bigk_dense() say what ran.  Small indexes reach the route with bigk_dense_min_docs=0 and a small bigk_cand_max.
-m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from growing_data import make_growing
from lifecycle_data import check, from_rows
from test_gpu_bigk import KS, NONE, W, _counts, _run, _segment

pytestmark = pytest.mark.gpu
ON = dict(bigk_dense=1, bigk_dense_min_docs=0, bigk_cand_max=5000)


@pytest.mark.parametrize("seg_max", [None, 4096], ids=["default_segment", "segment_4096"])
@pytest.mark.parametrize("k", [1025, 4097, 65535])
def test_candidates_around_k_and_the_threshold(tuning, k, seg_max):
    """150 000 and more candidates a query.  The default segment holds them all (settled at level 0, nothing cut); 4096 entries --
    k rounded up to tiles when that is more: 8192, 65536 -- do not: the histogram scans find a threshold and the emit scan cuts
    there, leaving at least k and at most the capacity.  A three-term query sums in term order."""
    seg, gix, ex = _counts()
    i = 3 * KS.index(k)
    terms, off = from_rows([[12], [i + 1, 12, 13], [12, 13]])
    tune = dict(ON, bigk_dense_seg=seg_max) if seg_max else ON
    b = _run(tuning, gix, ex.plain(terms, off, k), terms, off, k, (3, 0), **tune)
    n, levels, _, emitted = b.debug_bigk_dense()
    cap = max(-(-k // 4096) * 4096, seg_max or 1 << 20)
    assert n == 3 and 3 * k <= emitted <= 3 * cap
    assert levels == 1 if cap >= 160_000 else levels >= 1


@pytest.mark.parametrize("k", [1025, 4097])
def test_tie_mass_down_to_the_id_digits(tuning, k):
    """b = 0 and tf = 1: the 9000 documents of term 0 score the same and the segment (4096 entries, 8192 at k = 4097) holds fewer:
    the boundary lies inside the mass.  Levels 0 .. 3 cut at shifts 76, 64, 52 and 40 of the 96-bit composite, inside the key; only
    a level from 4 on reads the id's 32 bits -- the search must get there, and the records of the mass are its lowest ids."""
    rows = [np.arange(0, 18_000, 2), np.arange(0, 18_000, 60)]
    seg, gix, ex = _segment("ties", 20_000, rows, b=0.0, tf=[np.ones(len(r)) for r in rows])
    terms, off = from_rows([[0], [0, 1], [1]])
    want = ex.plain(terms, off, k)
    assert want[0]["doc_id"].tolist() == list(range(0, 2 * k, 2))
    b = _run(tuning, gix, want, terms, off, k, (3, 0), bigk_dense_seg=4096, **ON)
    n, levels, _, emitted = b.debug_bigk_dense()
    assert n == 2 and levels >= 5 and 2 * k <= emitted <= 2 * -(-k // 4096) * 4096


def _windows():
    """test_gpu_bigk.py's segment of 4 W + 77 documents: postings at every window cut, a term every 100 documents, a term in every
    document, a term in the first and the last window only"""
    n = 4 * W + 77
    cuts = np.concatenate([[0], *[[c - 1, c, c + 1] for c in (W, 2 * W, 3 * W, 4 * W)], [n - 1]])
    return _segment("windows", n, [cuts, np.arange(0, 3 * W, 100), np.arange(n), np.r_[5:W:3, 4 * W + 3:n:2]])


@pytest.mark.parametrize("item_win", [1 << 20, 2, 1], ids=["uncut", "two_windows_an_item", "one_window_an_item"])
def test_window_and_item_cuts(tuning, item_win):
    """every non-empty query dense (bigk_cand_max = 0): items of five, two and one window add into the same histograms and the
    same segments"""
    seg, gix, ex = _windows()
    terms, off = from_rows([[0], [1], [2], [0, 1, 3], [0, 1, 2, 3], [3]])
    tune = dict(ON, bigk_cand_max=0, bigk_dense_seg=4096, bigk_item_win=item_win)
    b = _run(tuning, gix, ex.plain(terms, off, 1025), terms, off, 1025, (6, 0), **tune)
    assert b.debug_bigk_dense()[0] == 6


def test_clip_bin(tuning):
    """1000 terms of one document each and one term in 19 000 documents, one query of all 1001: the sum of the s0 (the level-0
    bound, about 20 900) is more than 2^17 times the k-th score (a document of the common term alone), so the level-0 boundary is
    further than the 16 octaves of the ordinary bins below the bound: the clip bin, refined by the later levels"""
    n, k = 20_000, 1025
    rows = [np.array([19 * t + 3]) for t in range(1000)] + [np.arange(19_000)]
    seg, gix, ex = _segment("clip", n, rows)
    terms, off = from_rows([np.arange(1001)])
    want = ex.plain(terms, off, k)
    s0 = np.log((n + 1.0) / (np.array([len(r) for r in rows]) + 0.5)) * (1.2 + 1.0)  # (bm25.rs:285-289, 348)
    assert s0.sum() > 2.0 ** 17 * want[0]["score"][k - 1] > 0
    b = _run(tuning, gix, want, terms, off, k, (1, 0), bigk_dense_seg=4096, **ON)
    n_dense, levels, clipped, emitted = b.debug_bigk_dense()
    assert (n_dense, clipped) == (1, 1) and levels >= 2 and k <= emitted <= 4096


def test_mixed_batch_and_chunks(tuning):
    """an empty query, a query of unknown terms, sparse queries and three dense ones in one batch; 10 000 candidate entries a chunk
    hold two dense segments of 4096, so the dense queries take two chunks behind the sparse one.  A second, smaller query set
    leaves the records behind its counts as the first set wrote them."""
    seg, gix, ex = _counts()
    k = 1025
    terms, off = from_rows([[], [seg.n_terms + 5, seg.n_terms + 9], [0], [12], [1], [12, 13], [13], [2, 12]])
    b = _run(tuning, gix, ex.plain(terms, off, k), terms, off, k, (8, 0), bigk_dense_seg=4096, bigk_chunk_cand=10_000, **ON)
    assert b.debug_bigk_dense()[0] == 3
    first, _ = b.fetch()
    t2, o2 = from_rows([[13], [], [12]])
    b.set_queries(t2, o2)
    b.run()
    hits, nh = b.fetch()
    check(ex.plain(t2, o2, k), hits, nh, "second set")
    assert b.bigk_queries() == (3, 0) and b.debug_bigk_dense()[0] == 1
    assert hits[0, 10:].tobytes() == first[0, 10:].tobytes() and hits[1].tobytes() == first[1].tobytes()


def test_filter_selectors(tuning):
    """selector none, a bitmap of all documents, every second document, and one that rejects the unfiltered top k: the filter's bit
    is applied before an entry is counted or listed"""
    seg, gix, ex = _windows()
    k = 1025
    terms, off = from_rows([[0, 2]] * 4 + [[1, 2]])
    top = ex.plain(terms[:2], off[:2], k)[0]["doc_id"].astype(np.int64)
    keeps = np.ones((3, seg.n_docs), bool)
    keeps[1] = np.arange(seg.n_docs) % 2 == 0
    keeps[2, top] = False
    sel = np.array([NONE, 0, 1, 2, 1], np.uint32)
    want = ex.filtered(terms, off, k, keeps, sel)
    assert not set(want[3]["doc_id"].tolist()) & set(top.tolist())
    tune = dict(ON, bigk_cand_max=0, bigk_dense_seg=4096)
    b = _run(tuning, gix, want, terms, off, k, (5, 0), f=vb.DocFilter(gix, keeps), sel=sel, **tune)
    assert b.debug_bigk_dense()[0] == 5


@pytest.mark.parametrize("caller", ["growing", "stream"])
def test_callers_of_the_exhaustive_route(tuning, caller):
    """search_batch_growing and a Stream reach the dense route through run_exhaustive: the oracle's records, and the bytes of
    bigk_sparse=0"""
    seg, gix, ex = _counts()
    k = 1025
    terms, off = from_rows([[12, 13], [3], [], [12]])
    out = []
    for t in (dict(ON, bigk_dense_seg=4096), dict(bigk_sparse=0)):
        vb.reset_tuning()
        tuning(**t)
        if caller == "growing":
            G, _ = make_growing(seg.arrays()["term_key"], 300, seed=3, pool=terms, pool_p=0.4)
            hits, nh = vb.search_batch_growing(gix, vb.GrowingSegment(gix, **G), terms, off, k)
            check(ex.growing(terms, off, k, G), hits, nh, f"growing {t}")
        else:
            st = vb.Stream(gix, 2, 4, len(terms), k)
            st.submit(terms, off)
            st.submit(terms[:off[2]], off[:3])
            hits, nh = st.collect()
            check(ex.plain(terms, off, k), hits, nh, f"stream {t}")
            check(ex.plain(terms[:off[2]], off[:3], k), *st.collect(), f"stream {t} second batch")
        out.append([hits[q, :nh[q]].tobytes() for q in range(len(nh))])
    assert out[0] == out[1]
