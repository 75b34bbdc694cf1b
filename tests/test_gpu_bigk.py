"""The batched path of k > 1024 for sparse queries (bigk.hip: bigk_scan_kernel, bigk_select_kernel, bigk_sort_kernel,
bigk_rank_emit_kernel).  Every case checks its records two ways: against the oracle's brute force (score descending, id ascending, cut
at k) and byte for byte against the same batch under tuning(bigk_sparse=0), the per-query path; and Batch.bigk_queries() says which
path ran.  Segments are built posting by posting, so the number of candidates of a query, the documents at the window cuts (8192
documents a window) and the tie masses are exact.  set_queries refuses a query with a repeated term (ids strictly ascending), so no
batch can hold one.  -m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from growing_data import make_growing
from lifecycle_data import Expect, check, from_rows

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
W = 8192
KS = [1025, 4096, 4097, 65535]
_C = {}


def _segment(name, n_docs, rows, b=0.75, tf=None):
    """(segment, GpuIndex, Expect) of terms with the documents `rows` (one ascending id array a term), made once"""
    if name not in _C:
        rng = np.random.default_rng(len(rows) + n_docs)
        docs = np.concatenate(rows).astype(np.uint32)
        tfs = np.concatenate(tf).astype(np.uint32) if tf else rng.integers(1, 4, len(docs)).astype(np.uint32)
        lens = np.bincount(docs, weights=tfs, minlength=n_docs).astype(np.uint32) + (np.arange(n_docs, dtype=np.uint32) * 7) % 61
        keys = np.zeros((len(rows), 16), np.uint8)
        keys[:, 0], keys[:, 1] = np.arange(len(rows)) >> 8, np.arange(len(rows)) & 255
        start = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint64)
        seg = vb.Segment.build(1.2, b, lens, rng.integers(0, 65536, (n_docs, 3)).astype(np.uint16), keys, start, docs, tfs)
        _C[name] = (seg, vb.GpuIndex(seg), Expect(seg))
    return _C[name]


def _run(tuning, gix, want, terms, off, k, paths, f=None, sel=None, **tune):
    """the batch under `tune` and under bigk_sparse=0: `want`, the same bytes, `paths` = bigk_queries() of the first"""
    out, batches = [], []
    for t, p in ((tune, paths), (dict(bigk_sparse=0), (0, len(off) - 1))):
        vb.reset_tuning()
        tuning(**t)
        b = vb.Batch(gix, len(off) - 1, max(1, len(terms)), k)
        if f is not None:
            b.set_filter(f, sel)
        b.set_queries(terms, off)
        for rep in range(2):  # (the second run finds the cursors and the LDS-clean state of the first)
            b.run()
            hits, nh = b.fetch()
            assert b.bigk_queries() == p, f"queries by path {b.bigk_queries()}, want {p} under {t}"
            check(want, hits, nh, f"k={k} {t} run {rep}")
        assert b.debug_route() == 4 and b.debug_counts() == (0, 0)
        out.append((hits, nh))
        batches.append(b)
    (h1, n1), (h0, n0) = out
    assert np.array_equal(n1, n0) and all(h1[q, :n1[q]].tobytes() == h0[q, :n0[q]].tobytes() for q in range(len(n1)))
    return batches[0]


def _counts():
    """200 000 documents; per k of KS terms with k - 1, k and k + 1 documents (terms 3i .. 3i + 2), term 12 with 150 000, term 13
    with 10"""
    rng = np.random.default_rng(1)
    n = 200_000
    rows = [np.sort(rng.choice(n, c, replace=False)) for k in KS for c in (k - 1, k, k + 1)]
    rows += [np.sort(rng.choice(n, 150_000, replace=False)), np.sort(rng.choice(n, 10, replace=False))]
    return _segment("counts", n, rows)


@pytest.mark.parametrize("k", KS)
def test_candidates_around_k(tuning, k):
    """k - 1, k, k + 1 and far more than k non-zero candidates: one partial tile (1025), exactly one full tile (4096), two (4097),
    sixteen (65535); below k every candidate survives, above it the select cuts; a three-term query sums in term order"""
    seg, gix, ex = _counts()
    i = 3 * KS.index(k)
    terms, off = from_rows([[i], [i + 1], [i + 2], [12], [i + 1, 12, 13]])
    _run(tuning, gix, ex.plain(terms, off, k), terms, off, k, (5, 0))


@pytest.mark.parametrize("k", [1025, 4097])
def test_tie_mass_at_kth_place(tuning, k):
    """b = 0 and tf = 1: the 9000 documents of term 0 score the same, the 300 of term 1 on top of them more -- the k-th place lies
    in a mass of equal keys: the select goes through the doc digits, the tile rank decides by id"""
    n = 20_000
    rows = [np.arange(0, 18_000, 2), np.arange(0, 18_000, 60)]
    seg, gix, ex = _segment("ties", n, rows, b=0.0, tf=[np.ones(len(r)) for r in rows])
    terms, off = from_rows([[0], [0, 1], [1]])
    want = ex.plain(terms, off, k)
    assert want[0]["score"][k - 2] == want[0]["score"][k - 1] and len(want[0]) == k
    _run(tuning, gix, want, terms, off, k, (3, 0))


@pytest.mark.parametrize("item_win", [1 << 20, 2, 1], ids=["uncut", "two_windows_an_item", "one_window_an_item"])
def test_window_and_item_cuts(tuning, item_win):
    """postings at W - 1, W, W + 1 of every window cut (every item cut with one window an item; uncut -- the switch is clamped to
    the index's five windows -- one item walks all five, sweeping and clearing the LDS between them), a term with a posting every
    100 documents (a block of 128 spans two windows), a term in every document (more than k candidates across the cuts; its 257
    blocks in the uncut item take the wave's 64-ary block search beyond one step), and a query (term 3) that touches the first and
    the last window only; the last window is short"""
    n = 4 * W + 77
    cuts = np.concatenate([[0], *[[c - 1, c, c + 1] for c in (W, 2 * W, 3 * W, 4 * W)], [n - 1]])
    rows = [cuts, np.arange(0, 3 * W, 100), np.arange(n), np.r_[5:W:3, 4 * W + 3:n:2]]
    seg, gix, ex = _segment("windows", n, rows)
    terms, off = from_rows([[0], [1], [2], [0, 1, 3], [0, 1, 2, 3], [3]])
    _run(tuning, gix, ex.plain(terms, off, 1025), terms, off, 1025, (6, 0), bigk_item_win=item_win)


@pytest.mark.parametrize("chunk", [1 << 22, 5000], ids=["one_chunk", "several_chunks"])
def test_mixed_batch_and_chunks(tuning, chunk):
    """an empty query, a query of unknown terms only, sparse queries and one whose 150 000 postings exceed bigk_cand_max (the
    per-query path) in one batch; with 5000 candidate entries a chunk the seven sparse queries take two chunks.  A second query
    set with fewer hits leaves the records behind its counts as the first set wrote them."""
    seg, gix, ex = _counts()
    k = 1025
    terms, off = from_rows([[], [seg.n_terms + 5, seg.n_terms + 9], [0], [12], [1], [2], [3], [13]])
    b = _run(tuning, gix, ex.plain(terms, off, k), terms, off, k, (7, 1), bigk_cand_max=5000, bigk_chunk_cand=chunk)
    first, _ = b.fetch()
    t2, o2 = from_rows([[13], [], [13]])
    b.set_queries(t2, o2)
    b.run()
    hits, nh = b.fetch()
    assert nh.tolist() == [10, 0, 10]
    assert hits[:, 10:].tobytes() == first[:3, 10:].tobytes() and hits[1].tobytes() == first[1].tobytes()


def test_filter_selectors(tuning):
    """selector none, a bitmap of all documents, every second document, and one that rejects the unfiltered top k"""
    seg, gix, ex = _counts()
    k = 1025
    terms, off = from_rows([[8, 13]] * 4 + [[0, 1]])  # (4098 + 10 documents: the oracle's filtered ranking is not cut)
    top = ex.plain(terms[:2], off[:2], k)[0]["doc_id"].astype(np.int64)
    keeps = np.ones((3, seg.n_docs), bool)
    keeps[1] = np.arange(seg.n_docs) % 2 == 0
    keeps[2, top] = False
    sel = np.array([NONE, 0, 1, 2, 1], np.uint32)
    want = ex.filtered(terms, off, k, keeps, sel)
    assert not set(want[3]["doc_id"].tolist()) & set(top.tolist())
    _run(tuning, gix, want, terms, off, k, (5, 0), f=vb.DocFilter(gix, keeps), sel=sel)


def test_fewer_documents_than_k(tuning):
    n = 1500
    seg, gix, ex = _segment("small", n, [np.arange(n), np.arange(0, n, 3)])
    terms, off = from_rows([[0], [0, 1], [1]])
    want = ex.plain(terms, off, 2000)
    assert len(want[0]) == n
    _run(tuning, gix, want, terms, off, 2000, (3, 0))


@pytest.mark.parametrize("caller", ["growing", "stream"])
def test_callers_of_the_exhaustive_route(tuning, caller):
    """search_batch_growing and a Stream reach the sparse path through run_exhaustive: the oracle's records, and the bytes of
    bigk_sparse=0"""
    seg, gix, ex = _counts()
    k = 1025
    terms, off = from_rows([[0, 13], [3], [], [1, 2]])
    out = []
    for t in ({}, dict(bigk_sparse=0)):
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
