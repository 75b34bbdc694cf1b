"""Document filters on the growing segment (vbm25_filter_set_growing / update_growing / growing_device_words,
vbm25_search_batch_growing_filtered, a Batch holding a filter and a growing segment together).  For query q with selector s the
records are byte for byte
    vbm25_merge_hits(the sealed records filtered by sealed bitmap s, vbm25_growing_search(..., deleted OR NOT growing bit s), k)
and the expectation is computed without the device: the oracle's brute-force full ranking filtered and cut at k for the sealed half
(lifecycle_data.Expect.filtered), vb.growing_search with the rejected growing documents marked deleted for the growing half, the two
combined with vb.merge_hits.  Every sealed route, k from 1 to 1500, bitmap densities from none to all, the tile skip of
growing_scan_kernel, ties across the segments, bit updates on a resident batch, stale and foreign bitmaps, and C3 at full size.
-m gpu only."""
import ctypes

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from growing_data import make_growing
from lifecycle_data import Expect, built, check, rows_of

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
GT = 8192  # documents per tile of growing_scan_kernel
INVALID, UNSUPPORTED = -1, -4


def _sealed(n_docs, vocab, seed, mean_len=40):
    c = make_corpus(n_docs, vocab, seed=seed, length="lognormal", mean_len=mean_len)
    return c, built(c)


def _deleted(G):
    d = G["g_deleted"]
    return np.zeros(len(G["g_start"]) - 1, bool) if d is None else d.astype(bool)


def expected(ex, terms, off, k, G, keeps, gkeeps, sel):
    """per query: merge_hits(oracle's filtered sealed records, growing_search with the rejected growing documents deleted, k)"""
    key = ex.seg.arrays()["term_key"].reshape(-1, 16)
    sealed = ex.filtered(terms, off, k, keeps, sel)
    out = []
    for q, t in enumerate(rows_of(terms, off)):
        s = int(sel[q])
        Gq = G
        if s != NONE:
            Gq = dict(G)
            Gq["g_deleted"] = (_deleted(G) | ~gkeeps[s]).astype(np.uint8)
        t = t[t < ex.n_terms]
        grow = vb.growing_search(ex.seg, vb.Query([key[r].tobytes() for r in t]), k, **Gq)
        out.append(vb.merge_hits(sealed[q], grow, k))
    return out


def run_both(gix, gs, f, terms, off, k, sel, want, what, route=None):
    """the one-shot call and a resident Batch (filter set first, then the segment): both equal `want`, and each other byte for byte"""
    hits, nh = vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    check(want, hits, nh, f"{what} one-shot")
    b = vb.Batch(gix, len(off) - 1, max(1, len(terms)), k)
    b.set_filter(f, sel)
    b.set_growing(gs)
    b.set_queries(terms, off)
    if route is not None:
        assert b.debug_route() == route, f"{what}: route {b.debug_route()} instead of {route}"
    b.run()
    h2, n2 = b.fetch()
    check(want, h2, n2, f"{what} batch")
    assert np.array_equal(nh, n2) and all(hits[q, :nh[q]].tobytes() == h2[q, :nh[q]].tobytes() for q in range(len(nh)))
    return b, h2, n2


def n_growing_hits(records, n_grow):
    return sum(int((w["doc_id"] > 0xFFFFFFFF - n_grow).sum()) for w in records)


_C = {}


def _base():
    """60 000 sealed documents (every sealed route), its oracle"""
    if "A" not in _C:
        c, seg = _sealed(60_000, 4000, seed=8)
        _C["A"] = (c, seg, vb.GpuIndex(seg), Expect(seg))
    return _C["A"]


ROUTES = [  # (case, tuning, k, terms per query, nq, expected route: vbm25_batch_debug_route)
    ("win_k1", dict(fused=0, win_force=1), 1, 4, 48, 3),
    ("win_k10", dict(fused=0, win_force=1), 10, 4, 48, 3),
    ("win_k64", dict(fused=0, win_force=1), 64, 4, 48, 3),
    ("win_k256", dict(fused=0, win_force=1), 256, 4, 48, 3),
    ("range_k10", dict(fused=0, win=0), 10, 4, 48, 2),
    ("range_k256", dict(fused=0, win=0), 256, 4, 48, 2),
    ("plan_range_k64", dict(fused=0, arith=0, win=0), 64, 4, 48, 0),
    ("fused_k10", {}, 10, 4, 4, 1),
    ("dense_k10", dict(dense_x1000=0), 10, 4, 48, 0),
    ("many_terms_k10", {}, 10, 20, 16, 0),
    ("many_k1024", {}, 1024, 4, 24, 0),
    ("bigk_k1025", {}, 1025, 4, 6, 4),
    ("bigk_k1500", {}, 1500, 4, 6, 4),
]


@pytest.mark.parametrize("case,tune,k,nterms,nq,route", ROUTES, ids=[r[0] for r in ROUTES])
def test_k_and_routes_with_mixed_selectors(tuning, case, tune, k, nterms, nq, route):
    """selectors NONE, 0, 1 in turn: bitmap 0 keeps a random half of both segments, bitmap 1 a tenth of the sealed documents and a
    seventh of the growing ones"""
    c, seg, _, ex = _base()
    tuning(**tune)
    gix = vb.GpuIndex(seg)
    terms, off = make_queries(c, nq, nterms, seed=nq + k + nterms)
    n_grow = 2 * GT + 777
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=k, pool=terms, pool_p=0.4)
    gs = vb.GrowingSegment(gix, **G)
    rng = np.random.default_rng(k)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, np.arange(seg.n_docs) % 10 == 3])
    gkeeps = np.stack([rng.random(n_grow) < 0.5, np.arange(n_grow) % 7 == 2])
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs, gkeeps)
    sel = np.array([[NONE, 0, 1][q % 3] for q in range(nq)], np.uint32)
    want = expected(ex, terms, off, k, G, keeps, gkeeps, sel)
    assert n_growing_hits(want, n_grow) > 0
    b, hits, nh = run_both(gix, gs, f, terms, off, k, sel, want, case, route=route)
    # the unfiltered queries get the records of search_batch_growing
    uh, un = vb.search_batch_growing(gix, gs, terms, off, k)
    for q in np.flatnonzero(sel == NONE):
        assert nh[q] == un[q] and hits[q, :nh[q]].tobytes() == uh[q, :un[q]].tobytes(), f"{case}: unfiltered q{q} changed"
    # a re-run merges from the new sealed records (nothing of the last run's threshold survives)
    b.run()
    check(want, *b.fetch(), f"{case} re-run")


DENSITY_ROUTES = [("win", dict(fused=0, win_force=1), 10), ("range", dict(fused=0, win=0), 100), ("bigk", {}, 1025)]


@pytest.mark.parametrize("case,tune,k", DENSITY_ROUTES, ids=[r[0] for r in DENSITY_ROUTES])
def test_growing_bitmap_densities(tuning, case, tune, k):
    c, seg, _, ex = _base()
    tuning(**tune)
    gix = vb.GpuIndex(seg)
    nq = 24
    terms, off = make_queries(c, nq, 4, seed=31)
    n_grow = 3 * GT + 101
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=17, pool=terms, pool_p=0.4)
    gs = vb.GrowingSegment(gix, **G)
    rng = np.random.default_rng(5)
    skeep = np.arange(seg.n_docs) % 3 != 0  # (the sealed half is filtered in every case)
    # keep all, keep none, 1/2, 1/100, one document (the best growing document of query 0)
    key = seg.arrays()["term_key"].reshape(-1, 16)
    t0 = terms[off[0]:off[1]]
    top0 = vb.growing_search(seg, vb.Query([key[r].tobytes() for r in t0[t0 < seg.n_terms]]), 1, **G)
    assert len(top0) == 1
    one = np.zeros(n_grow, bool)
    one[0xFFFFFFFF - int(top0["doc_id"][0])] = True
    gkeeps = np.stack([np.ones(n_grow, bool), np.zeros(n_grow, bool), rng.random(n_grow) < 0.5, rng.random(n_grow) < 0.01, one])
    keeps = np.repeat(skeep[None], len(gkeeps), axis=0)
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs, gkeeps)
    masked, mn = vb.search_batch_masked(gix, terms, off, k, vb.DocFilter(gix, skeep), np.zeros(nq, np.uint32))
    for i in range(len(gkeeps)):
        sel = np.full(nq, i, np.uint32)
        want = expected(ex, terms, off, k, G, keeps, gkeeps, sel)
        _, hits, nh = run_both(gix, gs, f, terms, off, k, sel, want, f"{case} bitmap {i}")
        if i == 1:  # keep none: exactly the filtered sealed records
            assert np.array_equal(nh, mn) and all(hits[q, :nh[q]].tobytes() == masked[q, :mn[q]].tobytes() for q in range(nq))
        if i == 4:
            assert n_growing_hits([hits[0, :nh[0]]], n_grow) == 1
    # adversarial: bitmap q rejects exactly query q's unfiltered growing top-k (the sealed half keeps everything): a kernel that
    # offered a rejected document, or let one raise its threshold, returns short or wrong lists
    adv = np.ones((nq, n_grow), bool)
    for q, t in enumerate(rows_of(terms, off)):
        g = vb.growing_search(seg, vb.Query([key[r].tobytes() for r in t[t < seg.n_terms]]), k, **G)
        adv[q, 0xFFFFFFFF - g["doc_id"].astype(np.int64)] = False
    assert (~adv).sum() > nq
    f2 = vb.DocFilter(gix, np.ones((nq, seg.n_docs), bool))
    f2.set_growing(gs, adv)
    sel = np.arange(nq, dtype=np.uint32)
    want = expected(ex, terms, off, k, G, np.ones((nq, seg.n_docs), bool), adv, sel)
    _, hits, nh = run_both(gix, gs, f2, terms, off, k, sel, want, f"{case} adversarial")
    for q in range(nq):
        g = 0xFFFFFFFF - hits[q, :nh[q]]["doc_id"].astype(np.int64)
        g = g[g < n_grow]
        assert adv[q, g].all(), f"{case} q{q}: a rejected growing document was returned"


TILE_CASES = ["one_tile", "one_doc_of_the_last_word", "last_partial_tile", "first_and_last_tiles"]


@pytest.mark.parametrize("nq", [48, 600])
@pytest.mark.parametrize("case", TILE_CASES)
def test_tile_skip(tuning, case, nq):
    """n_grow = 4 GT + 5: bits in one tile only, in one document of the partial last word only, in the last partial tile only, in
    the first 64 documents and the last partial tile only (the tiles between are skipped).  48 queries: one tile per workgroup; 600 queries: one workgroup runs over every tile, skipping
    some and scanning others."""
    c, seg, _, ex = _base()
    tuning(fused=0, win_force=1)
    gix = vb.GpuIndex(seg)
    terms, off = make_queries(c, nq, 4, seed=nq + 7)
    n_grow = 4 * GT + 5
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=nq, pool=terms, pool_p=0.6, mean_elems=30)
    gs = vb.GrowingSegment(gix, **G)
    keeps = (np.arange(seg.n_docs) % 2 == 0)[None]
    sel = np.zeros(nq, np.uint32)
    gkeep = np.zeros(n_grow, bool)
    if case == "one_tile":
        gkeep[GT:2 * GT] = np.random.default_rng(1).random(GT) < 0.5
    elif case == "one_doc_of_the_last_word":  # (the last growing document that reaches a query's top-10 with the last tile kept)
        last = np.zeros(n_grow, bool)
        last[4 * GT:] = True
        w = expected(ex, terms, off, 10, G, keeps, last[None], sel)
        gkeep[max(0xFFFFFFFF - int(d) for r in w for d in r["doc_id"] if d > 0xFFFFFFFF - n_grow)] = True
    elif case == "last_partial_tile":
        gkeep[4 * GT:] = True
    else:
        gkeep[:64] = True
        gkeep[4 * GT:] = True
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs, gkeep[None])
    for k in (10, 1025) if nq == 48 else (10,):
        want = expected(ex, terms, off, k, G, keeps, gkeep[None], sel)
        assert n_growing_hits(want, n_grow) > 0, "no growing document of the kept ones matches: the case shows nothing"
        run_both(gix, gs, f, terms, off, k, sel, want, f"{case} k={k}", route=3 if k == 10 else 4)


def test_ties_across_segments_under_a_filter():
    """growing copies of sealed documents tie with them: under a filter the kept sealed hit still comes first, and the kept copies
    follow by growing index"""
    c, seg, gix, ex = _base()
    a = seg.arrays()
    key = a["term_key"].reshape(-1, 16)
    rng = np.random.default_rng(4)
    term_start, post_doc, post_tf = c["term_start"], c["post_doc"], c["post_tf"]
    rank_of = np.repeat(np.arange(len(term_start) - 1), np.diff(term_start.astype(np.int64)))
    docs = rng.choice(seg.n_docs, 40, replace=False)
    starts, keys, tfs, fns, pls = [0], [], [], [], []
    for rep in range(3):  # three copies of each chosen sealed document, the second round in tile 1
        for d in docs:
            s = np.nonzero(post_doc == d)[0]
            r = rank_of[s]
            o = np.argsort(r)
            keys.append(key[r[o]].reshape(-1))
            tfs.append(post_tf[s][o])
            starts.append(starts[-1] + len(s))
            fns.append(a["doc_fieldnorm"][d])
            pls.append([rep, int(d) & 0xFFFF, 9])
        pad = GT - len(fns) if rep == 0 else 0
        starts += [starts[-1]] * pad
        fns += [0] * pad
        pls += [[0, 0, 0]] * pad
    G = dict(g_start=np.array(starts, np.uint64), g_key=np.concatenate(keys), g_tf=np.concatenate(tfs).astype(np.uint32),
             g_fieldnorm=np.array(fns, np.uint8), g_payload=np.array(pls, np.uint16), g_deleted=None)
    n_grow = len(fns)
    gs = vb.GrowingSegment(gix, **G)
    rows = []
    for d in docs[:24]:
        r = np.sort(rank_of[post_doc == d])
        rows.append(r[:min(len(r), 1 + len(rows) % 5)])
    terms = np.concatenate(rows).astype(np.uint32)
    off = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint32)
    # bitmap 0: the chosen sealed documents and every copy but those of round 1; bitmap 1: every other chosen document, round 2 only
    skeep = np.zeros((2, seg.n_docs), bool)
    skeep[0, docs] = True
    skeep[1, docs[::2]] = True
    skeep[:, rng.random(seg.n_docs) < 0.3] = True
    g = np.arange(n_grow)
    rnd = np.minimum(g // len(docs), 2)
    rnd[(g >= len(docs)) & (g < GT)] = -1
    rnd[g >= GT] = 1 + (g[g >= GT] - GT) // len(docs)
    gkeep = np.stack([rnd != 1, rnd == 2])
    f = vb.DocFilter(gix, skeep)
    f.set_growing(gs, gkeep)
    nq = len(off) - 1
    for k in (1, 4, 10, 1500):
        for sel in (np.zeros(nq, np.uint32), np.array([[0, 1, NONE][q % 3] for q in range(nq)], np.uint32)):
            want = expected(ex, terms, off, k, G, skeep, gkeep, sel)
            run_both(gix, gs, f, terms, off, k, sel, want, f"ties k={k}")
    tied = sum(int((np.diff(w["score"]) == 0).sum()) for w in want)
    assert tied > 0


def test_bit_updates_on_a_resident_batch(tuning):
    """update_growing, then growing_device_words with bits packed by torch on the GPU: the next run follows the new bits"""
    import torch

    c, seg, gix, ex = _base()
    tuning(fused=0, win_force=1)
    nq, k = 32, 10
    terms, off = make_queries(c, nq, 4, seed=77)
    n_grow = 2 * GT + 333
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=21, pool=terms, pool_p=0.4)
    gs = vb.GrowingSegment(gix, **G)
    keeps = (np.arange(seg.n_docs) % 2 == 1)[None]
    g = np.arange(n_grow)
    gk0 = g % 2 == 0
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs, gk0[None])
    sel = np.zeros(nq, np.uint32)
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_growing(gs)
    b.set_filter(f, sel)
    b.set_queries(terms, off)
    b.run()
    check(expected(ex, terms, off, k, G, keeps, gk0[None], sel), *b.fetch(), "before")
    gk1 = g % 2 == 1  # (disjoint from the first)
    f.update_growing(0, gk1)
    b.run()
    want1 = expected(ex, terms, off, k, G, keeps, gk1[None], sel)
    check(want1, *b.fetch(), "after update_growing")
    gk2 = g % 7 == 5
    n_words = (n_grow + 63) // 64
    bits = torch.zeros(64 * n_words, dtype=torch.bool, device="cuda")
    bits[:n_grow] = torch.arange(n_grow, device="cuda") % 7 == 5
    words = (bits.view(n_words, 64).to(torch.int64) << torch.arange(64, device="cuda")).sum(dim=1)
    assert np.array_equal(words.cpu().numpy().view(np.uint64), vb.DocFilter.pack(gk2, n_grow)[0])
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so.7")  # (the one HIP runtime of the process: torch's and the library's)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(f.growing_device_words(0), words.data_ptr(), 8 * n_words, 3) == 0  # hipMemcpyDeviceToDevice
    b.run()
    want2 = expected(ex, terms, off, k, G, keeps, gk2[None], sel)
    check(want2, *b.fetch(), "after growing_device_words")
    assert n_growing_hits(want1, n_grow) > 0 and n_growing_hits(want2, n_grow) > 0


def _raise(code, fn, *args):
    with pytest.raises(vb.Vbm25Error) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)


def test_lifecycle_and_errors():
    c, seg, gix, ex = _base()
    nq, k = 16, 10
    terms, off = make_queries(c, nq, 3, seed=5)
    n_grow = GT + 70  # (not a multiple of 64: a partial last word)
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=8, pool=terms, pool_p=0.5)
    gs = vb.GrowingSegment(gix, **G)
    rng = np.random.default_rng(2)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, rng.random(seg.n_docs) < 0.2])
    gkeeps = np.stack([rng.random(n_grow) < 0.5, rng.random(n_grow) < 0.2])
    sel = np.array([0, 1, NONE, 1] * (nq // 4), np.uint32)
    want = expected(ex, terms, off, k, G, keeps, gkeeps, sel)
    f = vb.DocFilter(gix, keeps)
    # without growing bitmaps: UNSUPPORTED, as before this feature, from either setter and from the one-shot call
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_growing(gs)
    _raise(UNSUPPORTED, b.set_filter, f, sel)
    _raise(UNSUPPORTED, vb.search_batch_growing_masked, gix, gs, terms, off, k, f, sel)
    _raise(INVALID, f.growing_device_words, 0)
    assert vb.lib().vbm25_filter_update_growing(f.h, 0, vb.DocFilter.pack(gkeeps[0], n_grow).ctypes.data) == INVALID
    # both setter orders
    f.set_growing(gs, gkeeps)
    b.set_filter(f, sel)
    b.set_queries(terms, off)
    b.run()
    check(want, *b.fetch(), "growing, then filter")
    b2 = vb.Batch(gix, nq, len(terms), k)
    b2.set_filter(f, sel)
    b2.set_growing(gs)
    b2.set_queries(terms, off)
    b2.run()
    h_ok, n_ok = b2.fetch()
    check(want, h_ok, n_ok, "filter, then growing")
    # a re-upload of the same documents is another segment: the bitmaps of the first are stale for it
    gs2 = vb.GrowingSegment(gix, **G)
    b3 = vb.Batch(gix, nq, len(terms), k)
    b3.set_growing(gs2)
    _raise(INVALID, b3.set_filter, f, sel)
    _raise(INVALID, vb.search_batch_growing_masked, gix, gs2, terms, off, k, f, sel)
    # the filter's growing half set for gs2: a batch attached to gs refuses to run and keeps its records
    f.set_growing(gs2, gkeeps)
    _raise(INVALID, b2.run)
    h, n = b2.fetch()
    assert np.array_equal(n, n_ok) and h.tobytes() == h_ok.tobytes()
    _raise(INVALID, b2.run)
    b2.set_growing(gs2)  # (the batch follows the filter to the new upload)
    b2.run()
    check(want, *b2.fetch(), "after the re-upload")
    b3.set_filter(f, sel)
    b3.set_queries(terms, off)
    b3.run()
    check(want, *b3.fetch(), "re-upload, filter set after")
    hits, nh = vb.search_batch_growing_masked(gix, gs2, terms, off, k, f, sel)
    check(want, hits, nh, "re-upload one-shot")
    _raise(INVALID, b.set_growing, gs)  # (b holds f, whose bitmaps are gs2's now)
    # freeing the segment the bitmaps belong to stays legal; a later upload (perhaps at the freed address) does not match them
    b2.set_growing(None)
    b3.set_growing(None)
    vb.lib().vbm25_device_growing_free(gs2.h)
    gs2.h = None
    gs3 = vb.GrowingSegment(gix, **G)
    _raise(INVALID, b3.set_growing, gs3)
    # removing the growing half: UNSUPPORTED again
    f.set_growing(None)
    _raise(UNSUPPORTED, b3.set_growing, gs3)
    _raise(UNSUPPORTED, vb.search_batch_growing_masked, gix, gs3, terms, off, k, f, sel)
    _raise(INVALID, f.growing_device_words, 0)
    # a bit at or beyond n_grow, through set_growing and update_growing
    words = vb.DocFilter.pack(np.ones((2, n_grow + 1), bool), n_grow + 1)
    assert words.shape[1] == (n_grow + 63) // 64
    rc = vb.lib().vbm25_filter_set_growing(f.h, gs3.h, words.ctypes.data)
    assert rc == INVALID
    f.set_growing(gs3, gkeeps)
    rc = vb.lib().vbm25_filter_update_growing(f.h, 1, words[1].ctypes.data)
    assert rc == INVALID
    _raise(INVALID, f.update_growing, 2, gkeeps[0])  # (bitmap 2 of a filter of 2)
    # a segment of another index, a filter of another index
    gix2 = vb.GpuIndex(seg)
    gs_other = vb.GrowingSegment(gix2, **G)
    _raise(INVALID, f.set_growing, gs_other, gkeeps)
    f_other = vb.DocFilter(gix2, keeps)
    f_other.set_growing(gs_other, gkeeps)
    _raise(INVALID, vb.search_batch_growing_masked, gix, gs3, terms, off, k, f_other, sel)
    _raise(INVALID, vb.search_batch_growing_masked, gix, gs_other, terms, off, k, f, sel)
    # a selector out of range
    _raise(INVALID, vb.search_batch_growing_masked, gix, gs3, terms, off, k, f, np.full(nq, 2, np.uint32))
    b4 = vb.Batch(gix, nq, len(terms), k)
    b4.set_growing(gs3)
    _raise(INVALID, b4.set_filter, f, np.full(nq, 2, np.uint32))
    # and the valid state still answers
    b4.set_filter(f, sel)
    b4.set_queries(terms, off)
    b4.run()
    check(want, *b4.fetch(), "after the errors")
    # an empty growing segment takes growing bitmaps of no words
    G0, _ = make_growing(seg.arrays()["term_key"], 0, seed=1)
    gs0 = vb.GrowingSegment(gix, **G0)
    f.set_growing(gs0)
    hits, nh = vb.search_batch_growing_masked(gix, gs0, terms, off, k, f, sel)
    check(ex.filtered(terms, off, k, keeps, sel), hits, nh, "empty growing segment")


def test_full_size_c3():
    """C3's 10 M-document device index, 100 000 growing documents, a filter keeping a tenth of each segment, the window route: a
    64-query sample equals the expectation, one-shot and resident batch agree byte for byte"""
    from bench import make_queries as bench_queries
    dseg = vb.DeviceSegment.synth(10_000_000, 30_000, mean_len=100, len_mode=1, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    nq, k = 1024, 10
    terms, off = bench_queries(dseg, 30_000, nq, 5, seed=3, zipf_s=0.0)
    hseg = dseg.download()
    n_grow = 100_000
    G, _ = make_growing(hseg.arrays()["term_key"], n_grow, seed=11, mean_elems=60)
    gs = vb.GrowingSegment(gix, **G)
    keep = np.arange(hseg.n_docs) % 10 == 7
    gkeep = np.arange(n_grow) % 10 == 3
    f = vb.DocFilter(gix, keep)
    f.set_growing(gs, gkeep)
    sel = np.zeros(nq, np.uint32)
    hits, nh = vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_growing(gs)
    b.set_filter(f, sel)
    b.set_queries(terms, off)
    assert b.debug_route() == 3, f"route {b.debug_route()}"
    b.run()
    h2, n2 = b.fetch()
    assert np.array_equal(nh, n2) and hits.tobytes() == h2.tobytes()
    sample = np.sort(np.random.default_rng(0).choice(nq, 64, replace=False))
    rows = rows_of(terms, off)
    oix = Expect(hseg).oix
    key = hseg.arrays()["term_key"].reshape(-1, 16)
    Gq = dict(G)
    Gq["g_deleted"] = (_deleted(G) | ~gkeep).astype(np.uint8)
    got_growing = 0
    for q in sample:
        t = rows[q]
        full = oix.search_brute(t, 65535)  # (a prefix of the full ranking: complete once it holds k kept documents)
        kept = full[keep[full["doc_id"]]]
        assert len(kept) >= k or len(full) < 65535
        grow = vb.growing_search(hseg, vb.Query([key[r].tobytes() for r in t[t < hseg.n_terms]]), k, **Gq)
        want = vb.merge_hits(kept[:k], grow, k)
        check([want], hits[q:q + 1], nh[q:q + 1], f"C3 q{q}")
        got_growing += n_growing_hits([want], n_grow)
    assert got_growing > 0
