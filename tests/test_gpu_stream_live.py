"""A live table on the pipelined ring (vbm25_stream_set_growing / _set_filter / _submit_filtered): a growing segment that takes appends
and deletes and a filter whose bitmaps are updated and extended, searched through a ring with batches in flight across every mutation.
Every collected batch equals, byte for byte, vbm25_search_batch_growing_filtered on a state REBUILT for its submit (a fresh upload of
the concatenated documents, a fresh filter of the concatenated bitmaps) and, for a sample of queries, the host composition
merge_hits(the oracle's filtered sealed records, growing_search with the rejected documents deleted).  -m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from growing_data import make_growing
from lifecycle_data import Expect, built, check, from_rows, rows_of
from test_gpu_growing_append import docs, with_deleted
from test_gpu_growing_filter import ROUTES, expected

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
GT = 8192  # documents per tile of growing_scan_kernel
INVALID, UNSUPPORTED = -1, -4


def same(want, got, what):
    (wh, wn), (gh, gn) = want, got
    assert np.array_equal(wn, gn), f"{what}: counts differ"
    for q in range(len(wn)):
        assert wh[q, :wn[q]].tobytes() == gh[q, :gn[q]].tobytes(), f"{what} q{q}: records differ"


def one_shot(gix, gs, f, terms, off, k, sel):
    """the single-batch entry point for what is attached: _growing_filtered, _growing, _filtered or plain"""
    if gs is not None and f is not None:
        return vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    if gs is not None:
        return vb.search_batch_growing(gix, gs, terms, off, k)
    if f is not None:
        return vb.search_batch_masked(gix, terms, off, k, f, sel)
    return vb.search_batch(gix, terms, off, k)


def _raise(code, fn, *args, **kw):
    with pytest.raises(vb.Vbm25Error) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)


_C = {}


def _base():
    """60 000 sealed documents (the corpus of tests/test_gpu_growing_filter.py: every sealed route), its oracle"""
    if "A" not in _C:
        c = make_corpus(60_000, 4000, seed=8, length="lognormal", mean_len=40)
        seg = built(c)
        _C["A"] = (c, seg, vb.GpuIndex(seg), Expect(seg))
    return _C["A"]


def test_snapshot_rule():
    """Depth 3 on 300 000 documents.  Every mutation is issued with the ring full -- three batches in flight -- and is followed by one
    collect and one submit; the records are compared after the ring has drained, against the state of each batch's submit."""
    c = make_corpus(300_000, 6000, seed=21, length="lognormal", mean_len=40)
    seg = built(c)
    gix, ex = vb.GpuIndex(seg), Expect(seg)
    nq, k = 48, 10
    qsets = [make_queries(c, nq, 4, seed=100 + i) for i in range(4)]
    pool = np.concatenate([t for t, _ in qsets])
    pool = pool[pool < seg.n_terms]
    total = 3 * GT + 2500
    G, _ = make_growing(seg.arrays()["term_key"], total, seed=5, pool=pool, pool_p=0.4, deleted=None)
    rng = np.random.default_rng(7)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, np.arange(seg.n_docs) % 10 == 3])
    gkeeps = np.stack([rng.random(total) < 0.5, np.arange(total) % 3 != 1])
    n = 5000
    gone = np.zeros(total, bool)
    gs = vb.GrowingSegment(gix, **docs(G, 0, n))
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs, gkeeps[:, :n])
    st = vb.Stream(gix, 3, nq, len(qsets[0][0]), k)
    st.set_growing(gs)
    st.set_filter(f)
    submitted, collected = [], []

    def submit(i):
        terms, off = qsets[i % len(qsets)]
        sel = np.array([[0, 1, NONE][(q + i) % 3] for q in range(nq)], np.uint32)
        st.submit(terms, off, q_filter=sel)
        submitted.append(dict(terms=terms, off=off, sel=sel, n=n, gone=gone.copy(), keeps=keeps.copy(), gkeeps=gkeeps.copy()))

    def append(m):
        nonlocal n
        gs.append(**docs(G, n, n + m))
        f.extend_growing(gs, gkeeps[:, n:n + m])
        n += m

    def delete():
        g = rng.choice(n, 300, replace=False)
        gs.delete(g)
        gone[g] = True

    def update():
        keeps[0] = rng.random(seg.n_docs) < 0.3
        f.update(0, keeps[0])

    def update_growing():
        gkeeps[1, :n] = rng.random(n) < 0.6
        f.update_growing(1, gkeeps[1, :n])

    ops = [lambda: append(1), lambda: append(1000), delete, lambda: append(GT - n), lambda: append(1), update, update_growing,
           lambda: append(GT + 63), delete, lambda: append(1), update, lambda: append(1000), update_growing, lambda: append(total - n)]
    for i in range(3):
        submit(i)
    for i, op in enumerate(ops):
        assert st.in_flight == 3
        op()  # (three batches in flight across the mutation)
        collected.append(st.collect())
        submit(3 + i)
    while st.in_flight:
        collected.append(st.collect())
    assert n == total and len(collected) == len(submitted) == 3 + len(ops)
    n_growing = 0
    for i, (s, got) in enumerate(zip(submitted, collected)):
        Gnow = with_deleted(docs(G, 0, s["n"]), np.flatnonzero(s["gone"][:s["n"]]))
        fresh = vb.GrowingSegment(gix, **Gnow)
        ff = vb.DocFilter(gix, s["keeps"])
        ff.set_growing(fresh, s["gkeeps"][:, :s["n"]])
        same(vb.search_batch_growing_masked(gix, fresh, s["terms"], s["off"], k, ff, s["sel"]), got, f"batch {i} against a rebuilt state")
        pick = np.sort(np.random.default_rng(i).choice(nq, 16, replace=False))
        rows = rows_of(s["terms"], s["off"])
        t16, o16 = from_rows([rows[q] for q in pick])
        want = expected(ex, t16, o16, k, Gnow, s["keeps"], s["gkeeps"][:, :s["n"]], s["sel"][pick])
        check(want, got[0][pick], got[1][pick], f"batch {i} against the host composition")
        n_growing += sum(int((w["doc_id"] > 0xFFFFFFFF - total).sum()) for w in want)
    assert n_growing > 0


@pytest.mark.parametrize("depth", [1, 16])
def test_ring_wraps_at_the_extreme_depths(depth):
    """2 * depth + 1 batches of two to four queries through a ring of `depth` batches: full, then collect one and submit one until
    none is left, then drained -- the cursor passes its end twice; every batch against vbm25_search_batch"""
    c, seg, gix, _ = _base()
    k = 10
    batches = [make_queries(c, 2 + i % 3, 4, seed=700 + 40 * depth + i) for i in range(2 * depth + 1)]
    want = [vb.search_batch(gix, terms, off, k) for terms, off in batches]
    st = vb.Stream(gix, depth, 4, max(len(t) for t, _ in batches), k)
    _raise(INVALID, st.collect_raw)
    got = []
    for i, (terms, off) in enumerate(batches):
        if st.in_flight == depth:
            got.append(st.collect())
        st.submit(terms, off)
        assert st.in_flight == min(i + 1, depth)
    while st.in_flight:
        got.append(st.collect())
    assert len(got) == len(batches)
    for i, (w, g) in enumerate(zip(want, got)):
        same(w, g, f"depth {depth}, batch {i}")
    _raise(INVALID, st.collect_raw)


MODES = ["segment", "filter", "both"]


def _attach(st, mode, gs, f):
    st.set_growing(gs if mode != "filter" else None)
    st.set_filter(f if mode != "segment" else None)
    return (gs if mode != "filter" else None), (f if mode != "segment" else None)


@pytest.mark.parametrize("k", [1, 10, 100, 256, 257, 1024, 1500])
def test_shapes(k):
    """nq 1 .. 300 (the one-launch route for <= 8 queries, a k > 1024 ring) with only a segment, only a filter, both; selectors all
    NONE, mixed and -- plain submit on a ring that holds a filter -- none at all.  Up to three batches in flight, the ring re-used."""
    c, seg, gix, _ = _base()
    n_grow = GT + 777
    allq = {nq: make_queries(c, nq, 4, seed=nq + k) for nq in (1, 5, 8, 9, 33, 300)}
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=k, pool=np.concatenate([t[t < seg.n_terms] for t, _ in allq.values()]), pool_p=0.4)
    gs = vb.GrowingSegment(gix, **G)
    rng = np.random.default_rng(k)
    f = vb.DocFilter(gix, np.stack([rng.random(seg.n_docs) < 0.5, np.arange(seg.n_docs) % 10 == 3]))
    f.set_growing(gs, np.stack([rng.random(n_grow) < 0.5, np.arange(n_grow) % 7 == 2]))
    st = vb.Stream(gix, 3, 300, max(len(t) for t, _ in allq.values()), k)
    grew = 0
    for mode in MODES:
        a_gs, a_f = _attach(st, mode, gs, f)
        for nq, (terms, off) in allq.items():
            mixed = np.array([[NONE, 0, 1][q % 3] for q in range(nq)], np.uint32)
            sels = [None] if a_f is None else [mixed, np.full(nq, NONE, np.uint32), None]
            for sel in sels:
                st.submit(terms, off, q_filter=sel)
            for sel in sels:
                want = one_shot(gix, a_gs, a_f if sel is not None else None, terms, off, k, sel)
                got = st.collect()
                same(want, got, f"k={k} {mode} nq={nq} sel={'plain' if sel is None else sel[:3]}")
                if a_gs is not None:
                    grew += int((got[0]["doc_id"][0, :got[1][0]] > 0xFFFFFFFF - n_grow).sum())
    assert grew > 0, "no growing document in any first query's records: the case shows nothing"


@pytest.mark.parametrize("case,tune,k,nterms,nq,route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_sealed_route(tuning, case, tune, k, nterms, nq, route):
    """the sealed routes tests/test_gpu_growing_filter.py reaches with its tuning switches, through a ring with segment and filter"""
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
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_queries(terms, off)
    assert b.debug_route() == route, f"{case}: route {b.debug_route()} instead of {route}"
    st = vb.Stream(gix, 3, nq, len(terms), k)
    st.set_growing(gs)
    st.set_filter(f)
    for _ in range(3):
        st.submit(terms, off, q_filter=sel)
    want = expected(ex, terms, off, k, G, keeps, gkeeps, sel)
    ref = vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    for i in range(3):
        got = st.collect()
        check(want, got[0], got[1], f"{case} batch {i} against the host composition")
        same(ref, got, f"{case} batch {i}")


@pytest.mark.parametrize("nq,k", [(5, 10), (33, 10), (33, 257), (5, 1500)])
def test_adversarial_bitmaps(nq, k):
    """bitmap q rejects exactly query q's unfiltered top-4k of both segments: the filtered records are the ranks 4k + 1 .. 5k"""
    c, seg, gix, _ = _base()
    terms, off = make_queries(c, nq, 4, seed=3 * nq + k)
    n_grow = GT + 300
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=nq, pool=terms[terms < seg.n_terms], pool_p=0.05)
    gs = vb.GrowingSegment(gix, **G)
    deep, dn = vb.search_batch_growing(gix, gs, terms, off, 5 * k)
    keeps, gkeeps = np.ones((nq, seg.n_docs), bool), np.ones((nq, n_grow), bool)
    for q in range(nq):
        ids = deep["doc_id"][q, :min(dn[q], 4 * k)].astype(np.int64)
        keeps[q, ids[ids < seg.n_docs]] = False
        gkeeps[q, 0xFFFFFFFF - ids[ids >= seg.n_docs]] = False
    assert (~gkeeps).sum() > 0 and (~keeps).sum() > 0
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs, gkeeps)
    sel = np.arange(nq, dtype=np.uint32)
    st = vb.Stream(gix, 2, nq, len(terms), k)
    st.set_growing(gs)
    st.set_filter(f)
    st.submit(terms, off, q_filter=sel)
    st.submit(terms, off, q_filter=sel)
    ref = vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    for _ in range(2):
        hits, nh = st.collect()
        same(ref, (hits, nh), f"adversarial nq={nq} k={k}")
        for q in range(nq):  # (the ranks behind the rejected ones, straight from the deep unfiltered ranking)
            tail = deep[q, min(dn[q], 4 * k):dn[q]][:k]
            assert nh[q] == len(tail) and hits[q, :nh[q]].tobytes() == tail.tobytes(), f"q{q}"


def test_ties_across_segments():
    """growing copies of sealed documents tie with them: sealed first, then the kept copies by growing index"""
    c, seg, gix, ex = _base()
    a = seg.arrays()
    key = a["term_key"].reshape(-1, 16)
    rng = np.random.default_rng(4)
    term_start, post_doc, post_tf = c["term_start"], c["post_doc"], c["post_tf"]
    rank_of = np.repeat(np.arange(len(term_start) - 1), np.diff(term_start.astype(np.int64)))
    chosen = rng.choice(seg.n_docs, 40, replace=False)
    starts, keys, tfs, fns, pls = [0], [], [], [], []
    for rep in range(2):
        for d in chosen:
            s = np.nonzero(post_doc == d)[0]
            o = np.argsort(rank_of[s])
            keys.append(key[rank_of[s][o]].reshape(-1))
            tfs.append(post_tf[s][o])
            starts.append(starts[-1] + len(s))
            fns.append(a["doc_fieldnorm"][d])
            pls.append([rep, int(d) & 0xFFFF, 9])
    G = dict(g_start=np.array(starts, np.uint64), g_key=np.concatenate(keys), g_tf=np.concatenate(tfs).astype(np.uint32),
             g_fieldnorm=np.array(fns, np.uint8), g_payload=np.array(pls, np.uint16), g_deleted=None)
    n_grow = len(fns)
    gs = vb.GrowingSegment(gix, **G)
    rows = []
    for d in chosen[:24]:
        r = np.sort(rank_of[post_doc == d])
        rows.append(r[:min(len(r), 1 + len(rows) % 5)])
    terms, off = from_rows(rows)
    nq = len(rows)
    keeps = np.zeros((1, seg.n_docs), bool)
    keeps[0, chosen] = True
    keeps[0, rng.random(seg.n_docs) < 0.3] = True
    gkeeps = (np.arange(n_grow) >= len(chosen))[None]  # (the second round of copies only)
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs, gkeeps)
    for k in (4, 10, 1500):
        st = vb.Stream(gix, 2, nq, len(terms), k)
        st.set_growing(gs)
        st.set_filter(f)
        for sel in (np.zeros(nq, np.uint32), np.array([[0, NONE][q % 2] for q in range(nq)], np.uint32)):
            st.submit(terms, off, q_filter=sel)
            want = expected(ex, terms, off, k, G, keeps, gkeeps, sel)
            check(want, *st.collect(), f"ties k={k}")
        assert sum(int((np.diff(w["score"]) == 0).sum()) for w in want) > 0


def test_empty_growing_segment_and_empty_index():
    c, seg, gix, _ = _base()
    nq, k = 12, 10
    terms, off = make_queries(c, nq, 3, seed=2)
    keeps = (np.arange(seg.n_docs) % 2 == 0)[None]
    sel = np.array([0, NONE] * (nq // 2), np.uint32)
    G0, _ = make_growing(seg.arrays()["term_key"], 0, seed=1)
    gs0 = vb.GrowingSegment(gix, **G0)
    f = vb.DocFilter(gix, keeps)
    f.set_growing(gs0)
    st = vb.Stream(gix, 2, nq, len(terms), k)
    st.set_growing(gs0)
    st.set_filter(f)
    st.submit(terms, off, q_filter=sel)
    st.submit(terms, off)
    same(vb.search_batch_masked(gix, terms, off, k, f, sel), st.collect(), "empty growing segment, filtered")
    same(vb.search_batch(gix, terms, off, k), st.collect(), "empty growing segment, plain")
    # the empty index (everything deleted and compacted): no hit, whatever is attached
    eix = vb.GpuIndex(vb.DeviceSegment.maintain(gix, np.ones(seg.n_docs, bool), None))
    est = vb.Stream(eix, 2, nq, len(terms), k)
    ef = vb.DocFilter(eix, np.zeros((1, 0), bool))
    G, _ = make_growing(seg.arrays()["term_key"], 100, seed=3)
    egs = vb.GrowingSegment(eix, **G)
    ef.set_growing(egs, np.ones((1, 100), bool))
    for gs_, f_ in ((None, None), (egs, None), (None, ef), (egs, ef)):
        est.set_growing(gs_)
        est.set_filter(f_)
        est.submit(terms, off, q_filter=np.zeros(nq, np.uint32) if f_ is not None else None)
        hits, nh = est.collect()
        assert nh.tolist() == [0] * nq


def test_setters():
    """attach, detach and swap between submits; every refused call returns its code, leaves in_flight as it was, and the next valid
    submit is correct"""
    c, seg, gix, _ = _base()
    nq, k = 20, 10
    terms, off = make_queries(c, nq, 3, seed=5)
    n_grow = GT + 70
    key = seg.arrays()["term_key"]
    G, _ = make_growing(key, n_grow + 50, seed=8, pool=terms, pool_p=0.5)
    GA = docs(G, 0, n_grow)
    GB, _ = make_growing(key, 3000, seed=9, pool=terms, pool_p=0.5)
    gsA, gsB = vb.GrowingSegment(gix, **GA), vb.GrowingSegment(gix, **GB)
    rng = np.random.default_rng(2)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, rng.random(seg.n_docs) < 0.2])
    gkA = np.stack([rng.random(n_grow + 50) < 0.5, rng.random(n_grow + 50) < 0.2])
    gkB = np.stack([rng.random(3000) < 0.5, rng.random(3000) < 0.2])
    fA, fB = vb.DocFilter(gix, keeps), vb.DocFilter(gix, keeps[::-1].copy())
    fA.set_growing(gsA, gkA[:, :n_grow])
    fB.set_growing(gsB, gkB)
    sel = np.array([0, 1, NONE, 1] * (nq // 4), np.uint32)
    st = vb.Stream(gix, 3, nq, len(terms), k)
    # three batches in flight, each with what it was submitted with: (A, fA), (B, fB), nothing
    st.set_growing(gsA)
    st.set_filter(fA)
    st.submit(terms, off, q_filter=sel)
    st.set_growing(gsB)
    st.set_filter(fB)
    st.submit(terms, off, q_filter=sel)
    st.set_growing(None)
    st.set_filter(None)
    st.submit(terms, off)
    same(vb.search_batch_growing_masked(gix, gsA, terms, off, k, fA, sel), st.collect(), "submitted with A")
    same(vb.search_batch_growing_masked(gix, gsB, terms, off, k, fB, sel), st.collect(), "submitted with B")
    same(vb.search_batch(gix, terms, off, k), st.collect(), "submitted with nothing")
    # submit_filtered without a filter
    st.submit(terms, off)
    _raise(INVALID, st.submit, terms, off, q_filter=sel)
    assert st.in_flight == 1
    # a plain submit on a filtered ring filters nothing and still merges the segment
    st.set_growing(gsA)
    st.set_filter(fA)
    st.submit(terms, off)
    same(vb.search_batch(gix, terms, off, k), st.collect(), "before the refused submit")
    same(vb.search_batch_growing(gix, gsA, terms, off, k), st.collect(), "plain submit on a filtered ring")
    # a selector beyond the filter's bitmaps
    _raise(INVALID, st.submit, terms, off, q_filter=np.full(nq, 2, np.uint32))
    # a segment and a filter of another index: refused by the setter, the ring keeps what it had
    gix2 = vb.GpuIndex(seg)
    gs_other = vb.GrowingSegment(gix2, **GA)
    f_other = vb.DocFilter(gix2, keeps)
    _raise(INVALID, st.set_growing, gs_other)
    _raise(INVALID, st.set_filter, f_other)
    assert st.in_flight == 0 and st.growing is gsA and st.doc_filter is fA
    st.submit(terms, off, q_filter=sel)
    same(vb.search_batch_growing_masked(gix, gsA, terms, off, k, fA, sel), st.collect(), "after the foreign handles")
    # bitmaps of another upload; a filter without growing bitmaps
    st.set_filter(fB)
    st.submit(terms, off)  # (in flight across the refused submits)
    _raise(INVALID, st.submit, terms, off, q_filter=sel)
    f_plain = vb.DocFilter(gix, keeps)
    st.set_filter(f_plain)
    _raise(UNSUPPORTED, st.submit, terms, off, q_filter=sel)
    assert st.in_flight == 1
    st.submit(terms, off, q_filter=np.full(nq, NONE, np.uint32))  # (no selector names a bitmap: nothing to pair)
    st.set_filter(fA)
    st.submit(terms, off, q_filter=sel)
    for what in ("in flight across the refusals", "all selectors NONE"):
        same(vb.search_batch_growing(gix, gsA, terms, off, k), st.collect(), what)
    same(vb.search_batch_growing_masked(gix, gsA, terms, off, k, fA, sel), st.collect(), "after the refusals")
    # stale bitmaps after an append: refused until they are extended; a plain submit is served meanwhile
    st.submit(terms, off, q_filter=sel)
    gsA.append(**docs(G, n_grow, n_grow + 50))
    _raise(INVALID, st.submit, terms, off, q_filter=sel)
    assert st.in_flight == 1
    st.submit(terms, off)
    fA.extend_growing(gsA, gkA[:, n_grow:])
    st.submit(terms, off, q_filter=sel)
    fresh_old, fresh_new = vb.GrowingSegment(gix, **GA), vb.GrowingSegment(gix, **G)
    ff = vb.DocFilter(gix, keeps)
    ff.set_growing(fresh_old, gkA[:, :n_grow])
    same(vb.search_batch_growing_masked(gix, fresh_old, terms, off, k, ff, sel), st.collect(), "submitted before the append")
    same(vb.search_batch_growing(gix, fresh_new, terms, off, k), st.collect(), "plain, after the append")
    ff.set_growing(fresh_new, gkA)
    same(vb.search_batch_growing_masked(gix, fresh_new, terms, off, k, ff, sel), st.collect(), "after the extend")
    # a full ring and a query set set_queries refuses leave the ring as it was
    for _ in range(3):
        st.submit(terms, off, q_filter=sel)
    _raise(INVALID, st.submit, terms, off, q_filter=sel)
    assert st.in_flight == 3
    for _ in range(3):
        same(vb.search_batch_growing_masked(gix, fresh_new, terms, off, k, ff, sel), st.collect(), "full ring")
    _raise(INVALID, st.submit, terms[::-1].copy(), off, q_filter=sel)
    assert st.in_flight == 0
    st.submit(terms, off, q_filter=sel)
    same(vb.search_batch_growing_masked(gix, fresh_new, terms, off, k, ff, sel), st.collect(), "after a refused query set")


def test_full_size_c3():
    """C3: 10 M documents generated on the device, 100 000 growing documents, a keep-9/10 filter, 1024 five-term queries through a
    depth-3 ring: every record equals the one-batch call's, the sealed part on the window route"""
    from bench import make_queries as bench_queries
    dseg = vb.DeviceSegment.synth(10_000_000, 30_000, mean_len=100, len_mode=1, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    nq, k = 1024, 10
    terms, off = bench_queries(dseg, 30_000, nq, 5, seed=3, zipf_s=0.0)
    hseg = dseg.download()
    n_grow = 100_000
    G, _ = make_growing(hseg.arrays()["term_key"], n_grow, seed=11, mean_elems=60)
    del hseg
    gs = vb.GrowingSegment(gix, **G)
    f = vb.DocFilter(gix, np.arange(dseg.n_docs) % 10 != 7)
    f.set_growing(gs, np.arange(n_grow) % 10 != 3)
    sel = np.zeros(nq, np.uint32)
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_queries(terms, off)
    assert b.debug_route() == 3, f"route {b.debug_route()}"
    ref = vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    assert int((ref[0]["doc_id"] > 0xFFFFFFFF - n_grow).sum()) > 0
    st = vb.Stream(gix, 3, nq, len(terms), k)
    st.set_growing(gs)
    st.set_filter(f)
    for _ in range(3):
        st.submit(terms, off, q_filter=sel)
    for i in range(5):
        got = st.collect()
        assert np.array_equal(ref[1], got[1]) and ref[0].tobytes() == got[0].tobytes(), f"batch {i}"
        if i < 2:
            st.submit(terms, off, q_filter=sel)
