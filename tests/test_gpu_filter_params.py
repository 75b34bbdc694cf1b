"""Filtered search (vbm25_batch_set_filter, vbm25_search_batch_filtered, vbm25_search_batch_growing_filtered) across the legal BM25
parameters and the corpora of test_gpu_bm25_params.py: every scan kernel has a FILT instantiation of its own, and a filter changes the
logic the parameters stress -- a filtered query starts without theta0 (term_kth_ub), its threshold rises only from admitted documents,
scan_dense_kernel leaves rejected documents out of its histogram and its re-scoring, the exhaustive route zeroes rejected scores
before its sort.

The expected records of a filtered query are the oracle's complete brute-force ranking with the rejected documents removed, cut to k
(bit for bit: doc ids, score bits, payloads); a keep-all bitmap or NO_FILTER gives the bytes of the unfiltered run of the same batch
(the FILT instantiation against its unfiltered twin).  Every case asserts its route and that a second run gives the same bytes.
-m gpu only."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from growing_data import make_growing
from lifecycle_data import check, from_rows, rows_of
from test_gpu_bm25_params import EDGE_ROUTES, PARAMS, PIDS, ROUTES, _corpus, _cut, _fieldnorm_coverage, _hazard, _raw
from test_gpu_docfilter import _check, _full, _want

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
K_REF = 65535  # (the oracle's ranking is asked for this many records: fewer means it is complete)

_FULL = {}  # key -> per query the oracle's complete unfiltered ranking


def _fulls(key, oix, terms, off):
    if key not in _FULL:
        _FULL[key] = _full(oix, terms, off)
    return _FULL[key]


def _prefixes(oix, terms, off, keeps, sel, k):
    """per query the oracle's top-65535 where a query matches more documents (head terms): the filtered answer taken from it is
    still exact when the prefix holds k admitted documents -- asserted"""
    out, seen = [], {}
    for q, t in enumerate(rows_of(terms, off)):
        key = t.tobytes()
        if key not in seen:
            seen[key] = oix.search_brute(t, K_REF)
        f = seen[key]
        s = int(sel[q])
        assert len(f) < K_REF or s == NONE or int(keeps[s][f["doc_id"]].sum()) >= k, f"q{q}: the reference prefix is too short"
        out.append(f)
    return out


def _sel(nq, cycle):
    return np.array([cycle[q % len(cycle)] for q in range(nq)], dtype=np.uint32)


def run_filtered(tuning, seg, terms, off, k, route, tune, keeps, sel, fulls, index_tune=None, keep_all=None, what=""):
    """the batch on `route` under `tune`, first unfiltered, then query q under bitmap sel[q] of `keeps`: records bit for bit the
    filtered oracle ranking, the same bytes on a second run and through search_batch_masked; the NO_FILTER queries and those of the
    keep-all bitmap (index keep_all) the bytes of the unfiltered run.  Returns (batch, debug_counts, debug_routes, hits, n_hits) of
    the filtered run."""
    if index_tune:
        tuning(**index_tune)
    gix = vb.GpuIndex(seg)
    vb.reset_tuning()
    tuning(**tune)
    f = vb.DocFilter(gix, keeps)
    nq = len(off) - 1
    bt = vb.Batch(gix, nq, max(1, len(terms)), k)
    bt.set_queries(terms, off)
    assert bt.debug_route() == route, f"{what}: route {bt.debug_route()} instead of {route}"
    bt.run()
    plain, n_plain = bt.fetch()
    bt.set_filter(f, sel)
    bt.run()
    hits, nh = bt.fetch()
    counts, routes = bt.debug_counts(), bt.debug_routes()
    _check(hits, nh, fulls, keeps, sel, k, what)
    for q in range(nq):
        if sel[q] == NONE or (keep_all is not None and sel[q] == keep_all):
            assert nh[q] == n_plain[q] and hits[q, :nh[q]].tobytes() == plain[q, :nh[q]].tobytes(), f"{what} q{q}: not the unfiltered bytes"
        else:  # (no rejected document, also where fewer than k are admitted)
            assert keeps[sel[q]][hits[q, :nh[q]]["doc_id"]].all(), f"{what} q{q}: a rejected document"
    bt.run()
    h2, n2 = bt.fetch()
    assert h2.tobytes() == hits.tobytes() and np.array_equal(n2, nh), f"{what}: the second run differs"
    h3, n3 = vb.search_batch_masked(gix, terms, off, k, f, sel)
    _check(h3, n3, fulls, keeps, sel, k, what + " (search_batch_masked)")
    return bt, counts, routes, hits, nh


# ---- A1: every route at every parameter pair under keep-all, a random half and the adversarial bitmap
def _route_keeps(n_docs, fulls, sel, k, seed):
    """keep-all; a seeded random half; every document but the unfiltered top-(4k) of each query that selects bitmap 2"""
    adv = np.ones(n_docs, bool)
    for q in np.flatnonzero(sel == 2):
        adv[fulls[q]["doc_id"][:4 * k]] = False
    return np.stack([np.ones(n_docs, bool), np.random.default_rng(seed).random(n_docs) < 0.5, adv])


@pytest.mark.parametrize("k1,b", PARAMS, ids=PIDS)
@pytest.mark.parametrize("case,corpus,k,route,tune,index_tune,given_up", ROUTES, ids=[r[0] for r in ROUTES])
def test_filtered_routes(tuning, k1, b, case, corpus, k, route, tune, index_tune, given_up):
    seg, oix, terms, off = _corpus(corpus, k1, b)
    fulls = _fulls((corpus, k1, b), oix, terms, off)
    if route in (1, 4):  # (a handful of queries: the one-launch route, the exhaustive route)
        terms, off = _cut(terms, off, 4)
        fulls = fulls[:4]
    sel = _sel(len(off) - 1, [NONE, 0, 1, 2])
    keeps = _route_keeps(seg.n_docs, fulls, sel, k, seed=3)
    bt, (items, failed), routes, hits, nh = run_filtered(tuning, seg, terms, off, k, route, tune, keeps, sel, fulls, index_tune,
                                                         keep_all=0, what=case)
    for q in np.flatnonzero(sel == 2):  # the adversarial bitmap did bite
        if len(fulls[q]) > 4 * k:
            assert not np.isin(hits[q, :nh[q]]["doc_id"], fulls[q]["doc_id"][:4 * k]).any()
    if given_up == "some":
        assert failed > 0, f"{case}: this shape is expected to give items up under the filter too"
    if given_up == "served":
        assert failed < items, f"{case}: all {items} items were given up"
    if case.startswith("dense"):
        assert routes[4] > 0, f"{case}: no item went to scan_dense_kernel"


# ---- A2: long and short documents: bitmaps that keep only the longest or only the shortest documents
# the most admitted matches any query of the corpus has under a bitmap, in round figures (the corpora are fixed): the test asserts
# that some query keeps min(k, cap) of them (L127 / Lwide: about 400 matches of codes >= 200 and 90 of codes <= 20 at most;
# S: 24 documents have a code >= 200, 8 of them in one query at most)
_CAP = {"L127": (300, 80), "Lwide": (300, 80), "S": (5, 300)}
_EDGE = {}


def _edge_set(corpus, b, seg, oix, terms, off):
    """(terms, off, fulls, keeps) of the corpus's queries, the best query of each bitmap first (the routes of a handful of queries
    take the first four)"""
    key = (corpus, b)
    if key not in _EDGE:
        fn = seg.arrays()["doc_fieldnorm"]
        keeps = np.stack([fn >= 200, fn <= 20])
        fulls = _fulls((corpus, 2.0, b), oix, terms, off)
        adm = np.array([[int(kp[f["doc_id"]].sum()) for kp in keeps] for f in fulls])
        first = [int(np.argmax(adm[:, 0]))]
        first.append(int(np.argmax(np.where(np.arange(len(fulls)) == first[0], -1, adm[:, 1]))))
        order = first + [q for q in range(len(fulls)) if q not in first]
        rows = rows_of(terms, off)
        t, o = from_rows([rows[q] for q in order])
        _EDGE[key] = (t, o, [fulls[q] for q in order], keeps)
    return _EDGE[key]


@pytest.mark.parametrize("b", [0.0, 1.0])
@pytest.mark.parametrize("corpus", ["L127", "Lwide", "S"])
@pytest.mark.parametrize("case,k,route,tune", EDGE_ROUTES, ids=[r[0] for r in EDGE_ROUTES])
def test_filtered_long_and_short_documents(tuning, b, corpus, case, k, route, tune):
    """k1 = 2.  Bitmap 0 keeps the documents of fieldnorm code >= 200 (at b = 1 they score lowest: they surface only because
    everything above them is rejected), bitmap 1 those of code <= 20."""
    seg, oix, terms, off = _corpus(corpus, 2.0, b)
    if corpus != "S":
        _fieldnorm_coverage(seg)
    terms, off, fulls, keeps = _edge_set(corpus, b, seg, oix, terms, off)
    if route in (1, 4):
        terms, off = _cut(terms, off, 4)
        fulls = fulls[:4]
    sel = _sel(len(off) - 1, [0, 1, NONE])
    for i in (0, 1):  # (so the case cannot pass on short or empty lists)
        most = max(int(keeps[i][f["doc_id"]].sum()) for f, s in zip(fulls, sel) if s == i)
        assert most >= min(k, _CAP[corpus][i]), f"bitmap {i}: {most} admitted matches at most"
    run_filtered(tuning, seg, terms, off, k, route, tune, keeps, sel, fulls, what=f"{corpus} {case}")


# ---- A3: the window hazard (word 0 of post_tfn holds zeros, S1[0] = 0 at b = 1) in scan_win_kernel's FILT instantiations
@pytest.mark.parametrize("id16", [True, False], ids=["planes", "id16_decoded"])
@pytest.mark.parametrize("b", [1.0, 0.99])
def test_window_hazard_under_a_filter(tuning, b, id16):
    """The index and queries of test_window_lanes_that_found_nothing_add_zero, every query filtered (keep-all, random half): a lane
    that found nothing adds exactly +0.0 in the filtered kernels too -- no NaN, no item given up, the oracle's records; the queries
    that touch the zero word give their items up and still return the oracle's records."""
    seg, oix, plain, touch = _hazard(b)
    index_tune = {} if id16 else dict(id16_plane=0, rel16_plane=0)
    n = seg.n_docs
    keeps = np.stack([np.ones(n, bool), np.random.default_rng(8).random(n) < 0.5])
    for name, (terms, off), ks in (("plain", plain, (10, 100)), ("touch", touch, (10,))):
        fulls = _fulls(("hazard", b, name), oix, terms, off)
        sel = _sel(len(off) - 1, [0, 1])
        for k in ks:
            _, (items, failed), _, hits, nh = run_filtered(tuning, seg, terms, off, k, 3, {}, keeps, sel, fulls, index_tune,
                                                           keep_all=0, what=f"{name} k={k}")
            if name == "plain":
                assert failed == 0, f"{failed} of {items} items given up"
                assert not any(np.isnan(hits["score"][q, :nh[q]]).any() for q in range(len(nh))), "NaN scores"
            else:
                assert failed > 0, "no item met the zero word"


# ---- A4: tie masses at b = 0 under a filter
def _tie_keeps(n_docs, group, m0, k, seed):
    """(i) every other document of the tie group rejected; (ii)-(iv) exactly k - 1, k, k + 1 of query 0's matches admitted (every
    other document of the group among them first); (v) none of query 0's matches admitted"""
    rng = np.random.default_rng(seed)
    alt = np.ones(n_docs, bool)
    alt[group[1::2]] = False
    out = [alt]
    pool = np.r_[group[::2], rng.permutation(np.setdiff1d(m0, group[::2]))]
    for m in (k - 1, k, k + 1):
        keep = np.ones(n_docs, bool)
        keep[m0] = False
        keep[pool[:m]] = True
        out.append(keep)
    none = np.ones(n_docs, bool)
    none[m0] = False
    out.append(none)
    return np.stack(out)


@pytest.mark.parametrize("k1", [1.2, 2.0])
def test_filtered_tie_masses_at_b0(tuning, k1):
    """Corpus T at b = 0 (whole blocks of equal scores).  Query 0 five times, once under each bitmap of _tie_keeps, the other
    queries (none of the head terms: complete rankings) cycling through NO_FILTER and the bitmaps; k cuts inside the tie group that
    ends at g (as test_tie_masses_at_b0 finds it), through scan_range_kernel, scan_dense_kernel, scan_win_kernel, scan_many_kernel
    (k = 300) and the exhaustive route (k = 2000)."""
    seg, oix, terms, off = _corpus("T", k1, 0.0)
    head = set(_raw("T")["token_to_term"][:3].tolist())
    rows = [r for r in rows_of(terms, off) if not head & set(r.tolist())]
    rows = [rows[0]] * 5 + rows[1:]
    terms, off = from_rows(rows)
    fulls = _fulls(("T", k1, "ties"), oix, terms, off)
    s = fulls[0]["score"]
    g = next(i for i in range(5, len(s) - 1) if s[i] != s[i - 1] and s[i - 1] == s[i - 2] and s[i] == s[i + 1])
    group = fulls[0]["doc_id"][s == s[g - 1]]
    m0 = fulls[0]["doc_id"]
    at = np.flatnonzero(s == s[g - 1])
    assert len(group) >= 3 and at[0] < g - 1 <= at[-1], "k = g - 1 does not cut inside the tie group"
    sel = np.r_[np.arange(5), [[NONE, 0, 1, 2, 3, 4][q % 6] for q in range(len(rows) - 5)]].astype(np.uint32)
    dense_off = dict(dense_x1000=10 ** 9)
    for k, route, tune in ((g - 1, 2, dict(fused=0, win=0, **dense_off)), (g - 1, 0, dict(dense_x1000=0)),
                           (g - 1, 3, dict(fused=0, win_force=1, **dense_off)), (300, 0, {}), (2000, 4, {})):
        t, o, fu, se = terms, off, fulls, sel
        if route == 4:
            t, o = _cut(terms, off, 5)
            fu, se = fulls[:5], sel[:5]
        keeps = _tie_keeps(seg.n_docs, group, m0, k, seed=k)
        _, _, _, hits, nh = run_filtered(tuning, seg, t, o, k, route, tune, keeps, se, fu, what=f"k={k} route {route}")
        assert nh[1] == k - 1 and nh[2] == k and nh[3] == k and nh[4] == 0, nh[:5]
    # the head-term queries (one item each over all 300 000 documents) through scan_dense_kernel under a random half
    h = _raw("T")["token_to_term"][:3]
    ht, ho = from_rows([np.sort(r).astype(np.uint32) for r in [h[[0, 1]], h[[0, 2]], h[[1, 2]], h] * 64])
    keeps = (np.random.default_rng(5).random(seg.n_docs) < 0.5)[None]
    sel = _sel(len(ho) - 1, [0, 0, 0, NONE, 0])
    for k in (10, 256):
        fu = _prefixes(oix, ht, ho, keeps, sel, k)
        _, _, routes, _, _ = run_filtered(tuning, seg, ht, ho, k, 0, dict(dense_x1000=0, dense_items=256), keeps, sel, fu,
                                          what=f"head terms k={k}")
        assert routes[4] > 0, "no item went to scan_dense_kernel"
    # near-equal scores (seg2 of test_tie_masses_at_b0): items beyond the dense kernel's re-scoring cap, filtered
    n = 200_000
    rng = np.random.default_rng(int(k1 * 10))
    keys = np.zeros((2, 16), np.uint8)
    keys[:, 0] = [ord("a"), ord("b")]
    docs_b = np.flatnonzero(rng.random(n) < 0.5).astype(np.uint32)
    tf_a = rng.integers(30_000, 65_000, n).astype(np.uint32)
    lens = tf_a.astype(np.int64)
    lens[docs_b] += 1
    seg2 = vb.Segment.build(k1, 0.0, lens.astype(np.uint32), rng.integers(0, 65536, (n, 3)).astype(np.uint16), keys,
                            np.array([0, n, n + len(docs_b)], np.uint64), np.r_[np.arange(n, dtype=np.uint32), docs_b],
                            np.r_[tf_a, np.ones(len(docs_b), np.uint32)])
    oix2 = orc.OracleIndex.from_arrays(seg2.meta(), seg2.arrays())
    nt, no = from_rows([np.array(r, np.uint32) for r in [[0], [0, 1]] * 128])
    keeps = (np.random.default_rng(6).random(n) < 0.5)[None]
    sel = _sel(len(no) - 1, [0, 0, NONE, 0])
    for k in (10, 100):
        fu = _prefixes(oix2, nt, no, keeps, sel, k)
        _, (items, failed), routes, _, _ = run_filtered(tuning, seg2, nt, no, k, 0, dict(dense_x1000=0, dense_items=256), keeps,
                                                        sel, fu, what=f"near-equal k={k}")
        assert routes[4] > 0, "no item went to scan_dense_kernel"
        assert failed > 0, "no filtered item reached the dense kernel's re-scoring cap"


# ---- A5: a growing segment (fieldnorms 0..255) and a filter on both segments
GROWING_ROUTES = [(10, 3, dict(fused=0, win_force=1)), (10, 2, dict(fused=0, win=0)), (100, 0, dict(dense_x1000=0)), (300, 0, {}),
                  (1500, 4, {})]


def _growing_want(seg, fulls, G, terms, off, k, keeps, gkeeps, sel):
    """vbm25_merge_hits(the filtered sealed answer, vbm25_growing_search with the rejected growing documents marked deleted)"""
    key = seg.arrays()["term_key"].reshape(-1, 16)
    deleted = G["g_deleted"].astype(bool)
    want = []
    for q, t in enumerate(rows_of(terms, off)):
        s = int(sel[q])
        sealed = fulls[q][:k] if s == NONE else _want(fulls[q], keeps[s], k)
        Gq = dict(G)
        if s != NONE:
            Gq["g_deleted"] = (deleted | ~gkeeps[s]).astype(np.uint8)
        t = t[t < seg.n_terms]
        want.append(vb.merge_hits(sealed, vb.growing_search(seg, vb.Query([key[r].tobytes() for r in t]), k, **Gq), k))
    return want


def _growing_keeps(seg, fulls, G, terms, off, k, sel, n_grow, seed):
    """sealed and growing bitmaps: a random half; every document of the merged unfiltered top-(4k) of each query of selector 1
    rejected; every growing document rejected (the sealed bitmap keeps all)"""
    rng = np.random.default_rng(seed)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, np.ones(seg.n_docs, bool), np.ones(seg.n_docs, bool)])
    gkeeps = np.stack([rng.random(n_grow) < 0.5, np.ones(n_grow, bool), np.zeros(n_grow, bool)])
    top = _growing_want(seg, fulls, G, terms, off, 4 * k, keeps, gkeeps, np.full(len(off) - 1, NONE, np.uint32))
    for q in np.flatnonzero(sel == 1):
        d = top[q]["doc_id"].astype(np.int64)
        keeps[1, d[d < seg.n_docs]] = False
        gkeeps[1, 0xFFFFFFFF - d[d > 0xFFFFFFFF - n_grow]] = False
    return keeps, gkeeps


def _run_growing_filtered(tuning, seg, oix, G, terms, off, key, what):
    gix = vb.GpuIndex(seg)
    n_grow = len(G["g_start"]) - 1
    gs = vb.GrowingSegment(gix, **G)
    fulls = _fulls(key, oix, terms, off)
    nq = len(off) - 1
    sel = _sel(nq, [NONE, 0, 1, 2])
    n_growing_hits = 0
    for k, route, tune in GROWING_ROUTES:
        vb.reset_tuning()
        tuning(**tune)
        keeps, gkeeps = _growing_keeps(seg, fulls, G, terms, off, k, sel, n_grow, seed=k)
        f = vb.DocFilter(gix, keeps)
        f.set_growing(gs, gkeeps)
        want = _growing_want(seg, fulls, G, terms, off, k, keeps, gkeeps, sel)
        n_growing_hits += sum(int((w["doc_id"] > 0xFFFFFFFF - n_grow).sum()) for w, s in zip(want, sel) if s != NONE)
        bt = vb.Batch(gix, nq, len(terms), k)
        bt.set_growing(gs)
        bt.set_queries(terms, off)
        assert bt.debug_route() == route, f"{what} k={k}: route {bt.debug_route()} instead of {route}"
        bt.set_filter(f, sel)
        bt.run()
        hits, nh = bt.fetch()
        check(want, hits, nh, f"{what} k={k} batch")
        bt.run()
        h2, n2 = bt.fetch()
        assert h2.tobytes() == hits.tobytes() and np.array_equal(n2, nh), f"{what} k={k}: the second run differs"
        check(want, *vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel), f"{what} k={k} one-shot")
    assert n_growing_hits > 0, "no filtered query returned a growing document"
    return gix


@pytest.mark.parametrize("b", [0.0, 1.0])
def test_growing_and_filter_at_the_edges(tuning, b):
    """L127 at k1 = 2 with 24 653 growing documents of every fieldnorm 0..255, the five sealed routes of
    test_growing_fieldnorms_0_to_255, query q under NO_FILTER, a random half, the adversarial bitmap of the merged ranking or one
    that rejects every growing document."""
    seg, oix, terms, off = _corpus("L127", 2.0, b)
    n_grow = 3 * 8192 + 77
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=11, pool=terms[terms < seg.n_terms], pool_p=0.4, fieldnorm_hi=256)
    assert len(np.unique(G["g_fieldnorm"])) == 256
    _run_growing_filtered(tuning, seg, oix, G, terms, off, ("L127", 2.0, b), f"b={b}")


def test_growing_copies_tie_sealed_documents_under_a_filter(tuning):
    """b = 0: growing documents copy the (term, tf) rows of the sealed documents at the top of every query, some twice -- exact
    ties across the segments, sealed ids before growing ids, the random-half bitmaps cutting inside the tie groups."""
    seg, oix, terms, off = _corpus("L127", 2.0, 0.0)
    c = _raw("L127")
    fulls = _fulls(("L127", 2.0, 0.0), oix, terms, off)
    src = np.unique(np.concatenate([f["doc_id"][:30] for f in fulls]))
    src = np.r_[src, src[::3]].astype(np.int64)  # (a third of them twice)
    ts = c["term_start"].astype(np.int64)
    term_of = np.repeat(np.arange(len(ts) - 1), np.diff(ts))
    by_doc = np.argsort(c["post_doc"], kind="stable")  # (doc-major, ascending term inside a document: the key order)
    d_start = np.searchsorted(c["post_doc"][by_doc], np.arange(c["n_docs"] + 1))
    el = np.concatenate([by_doc[d_start[d]:d_start[d + 1]] for d in src])
    n_el = np.array([d_start[d + 1] - d_start[d] for d in src])
    key = seg.arrays()["term_key"].reshape(-1, 16)
    rng = np.random.default_rng(12)
    G = dict(g_start=np.r_[0, np.cumsum(n_el)].astype(np.uint64), g_key=key[term_of[el]].reshape(-1),
             g_tf=c["post_tf"][el].astype(np.uint32), g_fieldnorm=seg.arrays()["doc_fieldnorm"][src].copy(),
             g_payload=rng.integers(0, 65535, (len(src), 3)).astype(np.uint16), g_deleted=np.zeros(len(src), np.uint8))
    # the copies tie their originals exactly
    q0 = rows_of(terms, off)[0]
    g0 = vb.growing_search(seg, vb.Query([key[r].tobytes() for r in q0[q0 < seg.n_terms]]), 30, **G)
    assert np.isin(g0["score"], fulls[0]["score"][:30]).all()
    _run_growing_filtered(tuning, seg, oix, G, terms, off, ("L127", 2.0, 0.0), "copies")
