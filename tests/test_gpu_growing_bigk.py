"""The growing segment at k > 1024 on the batched route (growing_bigk.h, tuning value bigk_grow): the records equal the host composition
and the per-query branch's (bigk_grow=0) byte for byte, and a second run of the same batch object gives the same bytes.  -m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from growing_data import make_growing
from lifecycle_data import Expect, check as check_fields
from test_gpu_growing import GT, _base, _queries, assert_records, host_composition
from test_gpu_growing_append import docs
from test_gpu_growing_filter import expected as filtered_expected

pytestmark = pytest.mark.gpu


def run_case(tuning, gix, gs, terms, off, k, want, what, f=None, sel=None, between=None, check=assert_records, **tune):
    """both routes against `want` (between: called after a first run, before the checked ones); returns the batched route's tally"""
    got = {}
    for grow in (1, 0):
        tuning(bigk_grow=grow, **tune)
        b = vb.Batch(gix, len(off) - 1, max(1, len(terms)), k)
        if f is not None:
            b.set_filter(f, sel)
        b.set_growing(gs[grow] if between else gs)
        b.set_queries(terms, off)
        if between:
            b.run()
            between(gs[grow])
        b.run()
        hits, nh = b.fetch()
        check(want, hits, nh, f"{what} bigk_grow={grow}")
        dbg = b.debug_bigk_grow()
        if grow:
            assert dbg[0] > 0 and dbg[3] >= 1, f"{what}: the batched route did not run: {dbg}"
            b.run()
            h2, n2 = b.fetch()
            assert np.array_equal(nh, n2) and hits.tobytes() == h2.tobytes() and b.debug_bigk_grow() == dbg, f"{what}: the second run differs"
            got["dbg"] = dbg
        else:
            assert dbg == (0, 0, 0, 0), f"{what}: bigk_grow=0 ran the batched route: {dbg}"
        got[grow] = [hits[q, :nh[q]].tobytes() for q in range(len(nh))]
    assert got[1] == got[0], f"{what}: the routes' records differ"
    return got["dbg"]


def _query_set(c, seg, seed):
    """_queries (1 .. 20 terms, empty, unknown ids) plus a query of unknown ids only and one of 300 terms: past the LDS term table's first fill"""
    terms, off = _queries(c, seg, seed)
    extra = [np.array([seg.n_terms + 3, seg.n_terms + 9], np.uint32), np.arange(5, 1205, 4, dtype=np.uint32)]
    return np.r_[terms, extra[0], extra[1]].astype(np.uint32), np.r_[off, off[-1] + 2, off[-1] + 302].astype(np.uint32)


@pytest.mark.parametrize("n_grow", [0, 1, GT - 1, GT, GT + 1, 3 * GT + 5])
def test_tile_boundaries(tuning, n_grow):
    c, seg, gix = _base()
    terms, off = _query_set(c, seg, seed=n_grow)
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=n_grow + 1, pool=terms[terms < seg.n_terms], pool_p=0.5)  # (a tenth deleted)
    want = host_composition(seg, gix, terms, off, 1025, G)
    dbg = run_case(tuning, gix, vb.GrowingSegment(gix, **G), terms, off, 1025, want, f"n_grow={n_grow}")
    if n_grow > GT:  # the 300-term query's sealed list is full: its low growing sums never reach the candidate segments
        assert dbg[1] > 0 and dbg[2] > 0, dbg
    if n_grow == 3 * GT + 5:
        assert run_case(tuning, gix, vb.GrowingSegment(gix, **G), terms, off, 1025, want, "three chunks", bigk_chunk_cand=1)[3] >= 3


def _one_term_docs(seg, t, tf, fn):
    """growing documents of the single term t: document g scores f(tf[g], fn[g]) on the query [t]"""
    n = len(tf)
    key = seg.arrays()["term_key"].reshape(-1, 16)
    return dict(g_start=np.arange(n + 1, dtype=np.uint64), g_key=np.tile(key[t], n), g_tf=np.asarray(tf, np.uint32),
                g_fieldnorm=np.asarray(fn, np.uint8), g_payload=(np.arange(3 * n).reshape(n, 3) % 65521).astype(np.uint16), g_deleted=None)


@pytest.mark.parametrize("m,k", [(1024, 1025), (1025, 1025), (1026, 1025), (5000, 4097), (5000, 65535)])
def test_candidate_counts_and_ties_by_g(tuning, m, k):
    """m candidates of a rare term around k and beyond one sort tile; half share one score: the k-th place lies in a mass ranked by g"""
    c, seg, gix = _base()
    df = np.diff(c["term_start"].astype(np.int64))
    t = int(np.argmin(np.where(df > 0, df, 1 << 30)))
    rng = np.random.default_rng(m + k)
    same = rng.random(m) < 0.5
    G = _one_term_docs(seg, t, np.where(same, 2, rng.integers(1, 6, m)), np.where(same, 40, rng.integers(0, 200, m)))
    terms, off = np.array([t, t, seg.n_terms + 1], np.uint32), np.array([0, 1, 3], np.uint32)
    want = host_composition(seg, gix, terms, off, k, G)
    assert len(want[0]) == min(k, m + df[t])
    assert run_case(tuning, gix, vb.GrowingSegment(gix, **G), terms, off, k, want, f"m={m} k={k}")[1] == 2 * m


def test_growing_scores_equal_to_sealed_scores_at_the_cut(tuning):
    """two growing copies (same tf and fieldnorm) of every sealed posting of a term: every growing score ties with a sealed one"""
    c, seg, gix = _base()
    df = np.diff(c["term_start"].astype(np.int64))
    t = int(np.argmax(np.where(df < 1000, df, 0)))
    assert 3 * df[t] > 1025
    p = slice(int(c["term_start"][t]), int(c["term_start"][t + 1]))
    fn = seg.arrays()["doc_fieldnorm"][c["post_doc"][p]]
    G = _one_term_docs(seg, t, np.tile(c["post_tf"][p], 2), np.tile(fn, 2))
    terms, off = np.array([t], np.uint32), np.array([0, 1], np.uint32)
    want = host_composition(seg, gix, terms, off, 1025, G)
    assert (np.diff(want[0]["score"]) == 0).sum() > 500 and len(want[0]) == 1025
    run_case(tuning, gix, vb.GrowingSegment(gix, **G), terms, off, 1025, want, "ties across the segments")


def test_filtered(tuning):
    """bitmaps on both halves: a random half, one that rejects the whole first growing tile, one that rejects everything; selector none"""
    c, seg, gix = _base()
    terms, off = _query_set(c, seg, seed=4)
    nq, n = len(off) - 1, 2 * GT + 100
    G, _ = make_growing(seg.arrays()["term_key"], n, seed=6, pool=terms[terms < seg.n_terms], pool_p=0.5)
    rng = np.random.default_rng(2)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, np.arange(seg.n_docs) % 3 == 0, np.zeros(seg.n_docs, bool)])
    gkeeps = np.stack([rng.random(n) < 0.5, np.arange(n) >= GT, np.zeros(n, bool)])
    sel = np.array([[vb.NO_FILTER, 0, 1, 2][q % 4] for q in range(nq)], np.uint32)
    gs = vb.GrowingSegment(gix, **G)
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs, gkeeps)
    want = filtered_expected(Expect(seg), terms, off, 1025, G, keeps, gkeeps, sel)
    run_case(tuning, gix, gs, terms, off, 1025, want, "filtered", f=f, sel=sel, check=check_fields)  # (field by field: the oracle's records leave their padding undefined)


def test_append_outgrows_the_scratch_and_a_stream_step(tuning):
    c, seg, gix = _base()
    terms, off = _query_set(c, seg, seed=8)
    G, _ = make_growing(seg.arrays()["term_key"], 2 * GT + 50, seed=31, pool=terms[terms < seg.n_terms])
    want = host_composition(seg, gix, terms, off, 1500, G)
    small = {grow: vb.GrowingSegment(gix, **docs(G, 0, 100)) for grow in (0, 1)}  # (the batch's scratch is sized for 100 documents)
    run_case(tuning, gix, small, terms, off, 1500, want, "appended", between=lambda gs: gs.append(**docs(G, 100, 2 * GT + 50)))
    tuning(bigk_grow=1)
    s = vb.Stream(gix, 2, len(off) - 1, len(terms), 1500)
    s.set_growing(small[1])
    s.submit(terms, off)
    assert_records(want, *s.collect(), "a k > 1024 step of a Stream")
