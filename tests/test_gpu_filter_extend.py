"""vbm25_filter_extend_growing: a filter's growing bitmaps extended in place after vbm25_device_growing_append.  After every extend the
filter must be, for every search, what vbm25_filter_set_growing of the concatenated bitmaps is: the records through the extended filter
are compared byte for byte with those through a filter freshly set, and two single-term queries whose term is in every growing
document, with k beyond the number of growing documents they can match, observe every bit directly.  -m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from lifecycle_data import built
from test_gpu_growing_append import docs

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
INVALID = -1
HALF = 60_000  # growing documents below HALF hold term TA, the others term TB: one k = 65535 query observes each half


def same(want, got, what):
    (wh, wn), (gh, gn) = want, got
    assert np.array_equal(wn, gn), f"{what}: counts differ"
    for q in range(len(wn)):
        assert wh[q, :wn[q]].tobytes() == gh[q, :gn[q]].tobytes(), f"{what} q{q}: records differ"


_C = {}


def _base():
    """20 000 sealed documents; 110 000 growing documents of four elements: TA or TB (by position) and three terms of the queries"""
    if "A" not in _C:
        c = make_corpus(20_000, 1500, seed=3, length="lognormal", mean_len=40)
        seg = built(c)
        gix = vb.GpuIndex(seg)
        terms, off = make_queries(c, 8, 3, seed=4)
        key = seg.arrays()["term_key"].reshape(-1, 16)
        n_terms, n = seg.n_terms, 110_000
        df = seg.arrays()["term_df"]
        ta, tb = np.argsort(df)[:2].astype(np.int64)  # (the two rarest terms: few sealed hits compete for the k = 65535 records)
        rng = np.random.default_rng(1)
        pool = terms[terms < n_terms].astype(np.int64)
        ids = np.concatenate([np.where(np.arange(n) < HALF, ta, tb)[:, None], pool[rng.integers(0, len(pool), (n, 3))]], axis=1)
        code = np.unique(np.arange(n, dtype=np.int64)[:, None] * n_terms + ids)
        d, t = code // n_terms, code % n_terms
        start = np.r_[0, np.cumsum(np.bincount(d, minlength=n))].astype(np.uint64)
        G = dict(g_start=start, g_key=key[t].reshape(-1), g_tf=rng.integers(1, 6, len(t)).astype(np.uint32),
                 g_fieldnorm=rng.integers(0, 200, n).astype(np.uint8), g_payload=rng.integers(0, 65535, (n, 3)).astype(np.uint16),
                 g_deleted=None)
        _C["A"] = (seg, gix, G, terms, off, int(ta), int(tb), int(df[ta]) + int(df[tb]))
    return _C["A"]


def observe(gix, gs, f, F, n, gkeeps, what):
    """the single-term queries over TA and TB under every bitmap: the growing documents returned are exactly the kept ones"""
    seg, _, _, _, _, ta, tb, n_sealed = _base()
    assert min(n, HALF) + n_sealed <= 65535 and max(n - HALF, 0) + n_sealed <= 65535
    for i in range(F):
        terms, off, sel = np.array([ta, tb], np.uint32), np.array([0, 1, 2], np.uint32), np.full(2, i, np.uint32)
        hits, nh = vb.search_batch_growing_masked(gix, gs, terms, off, 65535, f, sel)
        ids = np.concatenate([hits["doc_id"][q, :nh[q]] for q in range(2)]).astype(np.int64)
        g = np.sort(0xFFFFFFFF - ids[ids >= seg.n_docs])
        assert np.array_equal(g, np.flatnonzero(gkeeps[i, :n])), f"{what}: bitmap {i} does not hold the concatenated bits"


def compare(gix, gs, f, gkeeps, n, what, k=10):
    """the extended filter against one freshly set with the concatenated bitmaps, on the same segment"""
    seg, _, _, terms, off, _, _, _ = _base()
    F = len(gkeeps)
    ff = vb.DocFilter(gix, np.ones((F, seg.n_docs), bool))
    ff.set_growing(gs, gkeeps[:, :n])
    sel = (np.arange(len(off) - 1) % F).astype(np.uint32)
    sel[-1] = NONE
    got = vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    same(vb.search_batch_growing_masked(gix, gs, terms, off, k, ff, sel), got, what)
    return got


@pytest.mark.parametrize("F", [1, 3, 17])
@pytest.mark.parametrize("rem", [0, 1, 31, 63])
def test_extend_matches_a_fresh_set(rem, F):
    seg, gix, G, _, _, _, _, _ = _base()
    rng = np.random.default_rng(100 * F + rem)
    n_old = 4096 + rem
    for d in (1, 63, 64, 65, 1000, 100_000):
        n = n_old + d
        gkeeps = rng.random((F, n)) < 0.5
        gkeeps[0, n_old:] = True
        gs = vb.GrowingSegment(gix, **docs(G, 0, n_old))
        f = vb.DocFilter(gix, np.ones((F, seg.n_docs), bool))
        f.set_growing(gs, gkeeps[:, :n_old])
        gs.append(**docs(G, n_old, n))
        f.extend_growing(gs, gkeeps[:, n_old:])
        what = f"n_old={n_old} d={d} F={F}"
        compare(gix, gs, f, gkeeps, n, what)
        observe(gix, gs, f, F, n, gkeeps, what)
        # update_growing after an extend takes the new word count
        gkeeps[F - 1] = rng.random(n) < 0.3
        f.update_growing(F - 1, gkeeps[F - 1])
        compare(gix, gs, f, gkeeps, n, what + " after update_growing", k=100)
        if d in (1, 100_000):
            observe(gix, gs, f, F, n, gkeeps, what + " after update_growing")


def test_200_single_appends():
    """from an empty segment, one document at a time, each append followed by an extend: the capacity doubles several times on the way
    (1, 2, 4 words); the address of a bitmap may change across an extend"""
    seg, gix, G, _, _, _, _, _ = _base()
    F = 3
    rng = np.random.default_rng(9)
    gkeeps = rng.random((F, 200)) < 0.6
    gs = vb.GrowingSegment(gix, **docs(G, 0, 0))
    f = vb.DocFilter(gix, np.ones((F, seg.n_docs), bool))
    f.set_growing(gs, gkeeps[:, :0])
    addresses = set()
    for n in range(1, 201):
        gs.append(**docs(G, n - 1, n))
        f.extend_growing(gs, gkeeps[:, n - 1:n])
        addresses.add((f.growing_device_words(0), f.growing_device_words(F - 1) - f.growing_device_words(0)))
        compare(gix, gs, f, gkeeps, n, f"after {n} appends")
        if n % 8 == 0 or n in (1, 63, 64, 65, 127, 128, 129):
            observe(gix, gs, f, F, n, gkeeps, f"after {n} appends")
    assert len({stride for _, stride in addresses}) >= 3, "the bitmaps were never re-strided"
    # an all-zero delta (keep_new = None) and an empty one
    gs.append(**docs(G, 200, 300))
    f.extend_growing(gs)
    zeros = np.concatenate([gkeeps, np.zeros((F, 100), bool)], axis=1)
    compare(gix, gs, f, zeros, 300, "all-zero delta")
    observe(gix, gs, f, F, 300, zeros, "all-zero delta")
    f.extend_growing(gs, np.zeros((F, 0), bool))
    assert vb.lib().vbm25_filter_extend_growing(f.h, gs.h, None) == 0
    observe(gix, gs, f, F, 300, zeros, "d = 0")


def test_failures_leave_the_filter_as_it_was():
    seg, gix, G, _, _, _, _, _ = _base()
    F, n_old, d = 2, 1000, 70
    rng = np.random.default_rng(3)
    gkeeps = rng.random((F, n_old + d)) < 0.5
    gs = vb.GrowingSegment(gix, **docs(G, 0, n_old))
    f = vb.DocFilter(gix, np.ones((F, seg.n_docs), bool))
    L = vb.lib()
    delta = vb.DocFilter.pack(gkeeps[:, n_old:], d)
    assert L.vbm25_filter_extend_growing(f.h, gs.h, delta.ctypes.data) == INVALID  # no growing bitmaps
    f.set_growing(gs, gkeeps[:, :n_old])
    before = compare(gix, gs, f, gkeeps, n_old, "before")
    other = vb.GrowingSegment(gix, **docs(G, 0, n_old + d))  # (another upload, even of more documents)
    assert L.vbm25_filter_extend_growing(f.h, other.h, delta.ctypes.data) == INVALID
    assert L.vbm25_filter_extend_growing(f.h, None, delta.ctypes.data) == INVALID
    assert L.vbm25_filter_extend_growing(None, gs.h, delta.ctypes.data) == INVALID
    gs.append(**docs(G, n_old, n_old + d))
    bad = vb.DocFilter.pack(np.ones((F, d + 1), bool), d + 1)  # (a bit at d, in the last word of bitmap 1 only)
    bad[0] = delta[0]
    assert bad.shape == delta.shape
    assert L.vbm25_filter_extend_growing(f.h, gs.h, bad.ctypes.data) == INVALID
    # nothing changed: the bitmaps still cover n_old documents (stale for the appended segment, exact for a re-upload of the old one)
    assert f.grow_n == n_old
    with pytest.raises(vb.Vbm25Error) as e:
        compare(gix, gs, f, gkeeps, n_old + d, "stale")
    assert e.value.code == INVALID
    f.extend_growing(gs, gkeeps[:, n_old:])
    compare(gix, gs, f, gkeeps, n_old + d, "after the valid extend")
    observe(gix, gs, f, F, n_old + d, gkeeps, "after the valid extend")
    # the records for the old documents' state were those of `before`: a fresh filter over the old count on a fresh upload agrees
    gs_old = vb.GrowingSegment(gix, **docs(G, 0, n_old))
    f_old = vb.DocFilter(gix, np.ones((F, seg.n_docs), bool))
    f_old.set_growing(gs_old, gkeeps[:, :n_old])
    same(before, compare(gix, gs_old, f_old, gkeeps, n_old, "old state"), "old state")
