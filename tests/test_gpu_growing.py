"""The growing (unsealed) segment on the device (vbm25_growing_upload, vbm25_search_batch_growing, vbm25_batch_set_growing): per query
the records are byte for byte vbm25_merge_hits(the sealed records of vbm25_search_batch, vbm25_growing_search(the query's keys), k) --
the host composition the shim ran before -- on every sealed route, for k from 1 to beyond 1024, growing segments of zero to several
tiles (growing.h: GT = 8192 documents), deleted documents, keys the sealed segment lacks and score ties inside the growing segment and
across it and the sealed one.  -m gpu only."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from growing_data import make_growing
from parity import assert_same_ranking

pytestmark = pytest.mark.gpu
GT = 8192  # documents per tile of growing_scan_kernel


def _sealed(n_docs, vocab, seed, mean_len=40):
    c = make_corpus(n_docs, vocab, seed=seed, length="lognormal", mean_len=mean_len)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    return c, seg


def host_composition(seg, gix, terms, off, k, G):
    """what the shim computed: per query vbm25_merge_hits(sealed records of vbm25_search_batch, vbm25_growing_search)"""
    hits, nh = vb.search_batch(gix, terms, off, k)
    key = seg.arrays()["term_key"].reshape(-1, 16)
    n_terms = len(key)
    out = []
    for q in range(len(off) - 1):
        t = terms[off[q]:off[q + 1]]
        t = t[t < n_terms]
        grow = vb.growing_search(seg, vb.Query([key[r].tobytes() for r in t]), k, **G)
        out.append(vb.merge_hits(hits[q, :nh[q]], grow, k))
    return out


def assert_records(want, hits, nh, what):
    assert len(nh) == len(want)
    for q, w in enumerate(want):
        assert nh[q] == len(w), f"{what} q{q}: {nh[q]} records, want {len(w)}"
        assert hits[q, :nh[q]].tobytes() == w.tobytes(), f"{what} q{q}: records differ"


def check_both(seg, gix, gs, terms, off, k, G, what, tuning_route=None):
    want = host_composition(seg, gix, terms, off, k, G)
    hits, nh = vb.search_batch_growing(gix, gs, terms, off, k)
    assert_records(want, hits, nh, f"{what} one-shot")
    b = vb.Batch(gix, len(off) - 1, max(1, len(terms)), k)
    b.set_growing(gs)
    b.set_queries(terms, off)
    if tuning_route is not None:
        assert b.debug_route() == tuning_route, f"{what}: route {b.debug_route()}"
    b.run()
    h2, n2 = b.fetch()
    assert_records(want, h2, n2, f"{what} batch")
    return want


def _queries(c, seg, seed):
    """1 .. 8 terms, 20 terms, an empty query, unknown tokens (ids >= n_terms at the end of a query)"""
    n_terms = seg.meta()["n_terms"]
    rows = []
    for nterms in (1, 2, 3, 5, 8, 20):
        t, o = make_queries(c, 3, nterms, seed=seed + nterms)
        rows += [t[o[q]:o[q + 1]] for q in range(3)]
    rows.append(np.zeros(0, np.uint32))
    rows.append(np.r_[rows[3], np.uint32(n_terms + 7), np.uint32(0xFFFFFFFF)].astype(np.uint32))
    rows = [np.unique(r[r < n_terms]).tolist() + [x for x in r.tolist() if x >= n_terms] for r in rows]
    terms = np.array([x for r in rows for x in r], np.uint32)
    off = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint32)
    return terms, off


_C = {}


def _base():
    if "A" not in _C:
        c, seg = _sealed(20_000, 1500, seed=3)
        _C["A"] = (c, seg, vb.GpuIndex(seg))
    return _C["A"]


@pytest.mark.parametrize("k", [1, 10, 100, 256, 1000, 1500])
def test_records_equal_the_host_composition(k):
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=k)
    G, _ = make_growing(seg.arrays()["term_key"], 2 * GT + 777, seed=k, pool=terms[terms < seg.n_terms])
    gs = vb.GrowingSegment(gix, **G)
    assert gs.device_bytes > 0
    want = check_both(seg, gix, gs, terms, off, k, G, f"k={k}")
    assert sum(int((w["doc_id"] > 0xFFFFFFFF - (2 * GT + 777)).sum()) for w in want) > 0  # growing documents reached the records


@pytest.mark.parametrize("n_grow", [0, 1, GT - 1, GT, GT + 1, 3 * GT + 5])
@pytest.mark.parametrize("k", [10, 1025])
def test_tile_boundaries(n_grow, k):
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=n_grow)
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=n_grow + 1, pool=terms[terms < seg.n_terms], pool_p=0.5)
    gs = vb.GrowingSegment(gix, **G)
    check_both(seg, gix, gs, terms, off, k, G, f"n_grow={n_grow} k={k}")


def test_no_deleted_array_and_all_unknown_keys():
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=5)
    G, _ = make_growing(seg.arrays()["term_key"], 5000, seed=9, deleted=None, pool=terms[terms < seg.n_terms])
    assert G["g_deleted"] is None
    check_both(seg, gix, vb.GrowingSegment(gix, **G), terms, off, 100, G, "deleted=NULL")
    # documents of keys the sealed segment lacks only: no growing hit, the sealed records unchanged
    G2, _ = make_growing(seg.arrays()["term_key"][:0], 300, seed=2, n_unknown=40)
    gs2 = vb.GrowingSegment(gix, **G2)
    hits, nh = vb.search_batch_growing(gix, gs2, terms, off, 10)
    sh, snh = vb.search_batch(gix, terms, off, 10)
    assert np.array_equal(nh, snh) and all(hits[q, :nh[q]].tobytes() == sh[q, :nh[q]].tobytes() for q in range(len(nh)))


def test_score_ties_inside_and_across_segments():
    """Growing copies of sealed documents score exactly what the sealed ones do (same terms, tfs and fieldnorm, summed in term
    order): the sealed hit must come first.  Duplicates inside the growing segment rank by growing index."""
    c, seg, gix = _base()
    a = seg.arrays()
    key = a["term_key"].reshape(-1, 16)
    rng = np.random.default_rng(4)
    term_start, post_doc, post_tf = c["term_start"], c["post_doc"], c["post_tf"]
    rank_of = np.repeat(np.arange(len(term_start) - 1), np.diff(term_start.astype(np.int64)))
    docs = rng.choice(seg.n_docs, 40, replace=False)
    starts, keys, tfs, fns, pls = [0], [], [], [], []
    for rep in range(3):  # three growing copies of each chosen sealed document, spread over two tiles
        for d in docs:
            sel = np.nonzero(post_doc == d)[0]
            r = rank_of[sel]
            o = np.argsort(r)
            keys.append(key[r[o]].reshape(-1))
            tfs.append(post_tf[sel][o])
            starts.append(starts[-1] + len(sel))
            fns.append(a["doc_fieldnorm"][d])
            pls.append([rep, int(d) & 0xFFFF, 7])
        pad = GT - len(fns) if rep == 0 else 0  # (empty documents: the copies of the second round lie in tile 1)
        starts += [starts[-1]] * pad
        fns += [0] * pad
        pls += [[0, 0, 0]] * pad
    G = dict(g_start=np.array(starts, np.uint64), g_key=np.concatenate(keys), g_tf=np.concatenate(tfs).astype(np.uint32),
             g_fieldnorm=np.array(fns, np.uint8), g_payload=np.array(pls, np.uint16), g_deleted=None)
    gs = vb.GrowingSegment(gix, **G)
    # queries made of a chosen document's own terms: its sealed hit and its three copies tie
    rows = []
    for d in docs[:24]:
        r = np.sort(rank_of[post_doc == d])
        rows.append(r[:min(len(r), 1 + len(rows) % 5)])
    terms = np.concatenate(rows).astype(np.uint32)
    off = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint32)
    for k in (1, 4, 10, 1500):
        want = check_both(seg, gix, gs, terms, off, k, G, f"ties k={k}")
    tied = sum(int((np.diff(w["score"]) == 0).sum()) for w in want)
    assert tied > 0


ROUTES = [  # (case, tuning, k, nq, expected route: vbm25_batch_debug_route)
    ("fused_one_launch", {}, 10, 4, 1),
    ("plan_range", dict(fused=0, arith=0, win=0), 10, 64, 0),
    ("range_arith", dict(fused=0, win=0), 100, 64, 2),
    ("win", dict(fused=0, win_force=1), 10, 64, 3),
    ("win_giveups", dict(fused=0, win_force=1), 10, 64, 3),
    ("dense_all", dict(dense_x1000=0), 10, 64, 0),
    ("scan_many_k300", {}, 300, 64, 0),
    ("bigk", {}, 2000, 16, 4),
    ("nq_1", {}, 10, 1, 1),
]


@pytest.mark.parametrize("case,tune,k,nq,route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_sealed_route(tuning, case, tune, k, nq, route):
    if case == "win_giveups":  # thick lists: windows with more second arrivals than an item holds are given up
        c, seg = _sealed(200_000, 3000, seed=2, mean_len=60)
    else:
        c, seg = _sealed(60_000, 4000, seed=8)
    tuning(**tune)
    gix = vb.GpuIndex(seg)
    terms, off = make_queries(c, nq, 4, seed=nq + k)
    G, _ = make_growing(seg.arrays()["term_key"], GT + 100, seed=1, pool=terms, pool_p=0.4)
    gs = vb.GrowingSegment(gix, **G)
    check_both(seg, gix, gs, terms, off, k, G, case, tuning_route=route)


def test_empty_sealed_index():
    meta = dict(n_docs=0, n_terms=0, n_blocks=0, sum_len=0, k1=1.2, b=0.75)
    arrays = {k: np.zeros(0, dtype=dt) for k, dt in vb.api._DESC_ARRAYS}
    arrays["term_first_block"] = np.zeros(1, dtype=np.uint32)
    arrays["blk_off8"] = np.zeros(1, dtype=np.uint32)
    desc, keep = vb.api.desc_from_arrays(meta, arrays)
    gix = vb.GpuIndex(desc)
    G, _ = make_growing(np.zeros((0, 16), np.uint8), 100, seed=3)
    gs = vb.GrowingSegment(gix, **G)
    for k in (10, 2000):
        hits, nh = vb.search_batch_growing(gix, gs, np.array([0, 5], np.uint32), np.array([0, 1, 2], np.uint32), k)
        assert nh.tolist() == [0, 0]
        b = vb.Batch(gix, 2, 2, k)
        b.set_growing(gs)
        b.set_queries(np.array([0, 5], np.uint32), np.array([0, 1, 2], np.uint32))
        b.run()
        assert b.fetch()[1].tolist() == [0, 0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_the_oracle(seed):
    c, seg = _sealed(30_000 * seed, 800 * seed, seed=seed)
    gix = vb.GpuIndex(seg)
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    terms, off = make_queries(c, 24, 1 + seed, seed=seed)
    G, g_term = make_growing(seg.arrays()["term_key"], 3000 * seed, seed=seed, pool=terms)
    gs = vb.GrowingSegment(gix, **G)
    k = 20
    hits, nh = vb.search_batch_growing(gix, gs, terms, off, k)
    ext, next_ = vb.search_batch_growing(gix, gs, terms, off, k + 300)
    g_del = G["g_deleted"]
    for q in range(len(off) - 1):
        t = terms[off[q]:off[q + 1]]
        ref = oix.search_wand_growing(t, k, G["g_start"], g_term, G["g_tf"], G["g_fieldnorm"], G["g_payload"], g_del)
        assert_same_ranking(ref, hits[q, :nh[q]], ref_ext=ext[q, :next_[q]], what=f"seed {seed} q{q}")


def test_batch_behaviour():
    c, seg, gix = _base()
    terms, off = make_queries(c, 32, 3, seed=1)
    nq = len(off) - 1
    G, _ = make_growing(seg.arrays()["term_key"], 4000, seed=5, pool=terms, pool_p=0.5)
    gs = vb.GrowingSegment(gix, **G)
    want = host_composition(seg, gix, terms, off, 10, G)
    sealed, snh = vb.search_batch(gix, terms, off, 10)
    b = vb.Batch(gix, nq, len(terms), 10)
    b.set_growing(gs)
    b.set_queries(terms, off)
    b.set_timing(True)
    b.run()
    ms, n = b.kernel_ms()
    assert n == 1 and ms > 0
    # vbm25_batch_device_results points at the merged records
    import ctypes
    hp, cp = b.device_results()
    b.run()
    dev_hits = np.zeros((nq, 10), dtype=vb.HIT_DTYPE)
    dev_n = np.zeros(nq, dtype=np.uint32)
    hip = ctypes.CDLL("libamdhip64.so")  # (the runtime libvbm25 runs on; hipMemcpy orders behind the run on the null stream)
    assert hip.hipMemcpy(ctypes.c_void_p(dev_hits.ctypes.data), ctypes.c_void_p(hp), ctypes.c_size_t(dev_hits.nbytes), 2) == 0
    assert hip.hipMemcpy(ctypes.c_void_p(dev_n.ctypes.data), ctypes.c_void_p(cp), ctypes.c_size_t(dev_n.nbytes), 2) == 0
    assert_records(want, dev_hits, dev_n, "device_results")
    # a re-run does not merge the growing hits twice
    b.run()
    assert_records(want, *b.fetch(), "re-run")
    # detached: vbm25_search_batch's records exactly
    b.set_growing(None)
    b.run()
    h, n = b.fetch()
    assert np.array_equal(n, snh) and all(h[q, :n[q]].tobytes() == sealed[q, :n[q]].tobytes() for q in range(nq))
    # a larger re-upload shows at the next run
    G2, _ = make_growing(seg.arrays()["term_key"], 3 * GT, seed=6, pool=terms, pool_p=0.5)
    gs2 = vb.GrowingSegment(gix, **G2)
    assert gs2.device_bytes > gs.device_bytes
    b.set_growing(gs2)
    b.run()
    assert_records(host_composition(seg, gix, terms, off, 10, G2), *b.fetch(), "re-upload")
    # a filter and a growing segment: UNSUPPORTED from whichever setter comes second
    f = vb.DocFilter(gix, np.ones(seg.n_docs, dtype=bool))
    with pytest.raises(vb.Vbm25Error) as e:
        b.set_filter(f, np.zeros(nq, np.uint32))
    assert e.value.code == -4
    b.set_growing(None)
    b.set_filter(f, np.zeros(nq, np.uint32))
    with pytest.raises(vb.Vbm25Error) as e:
        b.set_growing(gs)
    assert e.value.code == -4
    b.set_filter(None)
    b.set_growing(gs)
    # a growing segment of another index
    gix2 = vb.GpuIndex(seg)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.search_batch_growing(gix2, gs, terms, off, 10)
    assert e.value.code == -1
    b.set_growing(None)


def test_upload_rejects_bad_segments():
    c, seg, gix = _base()
    G, _ = make_growing(seg.arrays()["term_key"], 50, seed=7)
    bad = dict(G)
    g = int(np.argmax(np.diff(G["g_start"].astype(np.int64)) >= 2))
    e0 = int(G["g_start"][g])
    keys = G["g_key"].reshape(-1, 16).copy()
    keys[[e0, e0 + 1]] = keys[[e0 + 1, e0]]  # keys of document g out of order
    bad["g_key"] = keys.reshape(-1)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.GrowingSegment(gix, **bad)
    assert e.value.code == -1 and "ascending" in str(e.value)
    bad = dict(G)
    st = G["g_start"].copy()
    st[5] = st[6] + 1  # not monotone
    bad["g_start"] = st
    with pytest.raises(vb.Vbm25Error) as e:
        vb.GrowingSegment(gix, **bad)
    assert e.value.code == -1


def test_full_size_c3():
    """C3's 10 M-document device index plus 100 000 growing documents, 1024 five-term queries: a 64-query sample equals the host
    composition, and the one-shot and resident paths give the same records."""
    from bench import make_queries as bench_queries
    dseg = vb.DeviceSegment.synth(10_000_000, 30_000, mean_len=100, len_mode=1, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    terms, off = bench_queries(dseg, 30_000, 1024, 5, seed=3, zipf_s=0.0)
    hseg = dseg.download()
    G, _ = make_growing(hseg.arrays()["term_key"], 100_000, seed=11, mean_elems=60)
    gs = vb.GrowingSegment(gix, **G)
    hits, nh = vb.search_batch_growing(gix, gs, terms, off, 10)
    b = vb.Batch(gix, 1024, len(terms), 10)
    b.set_growing(gs)
    b.set_queries(terms, off)
    b.run()
    h2, n2 = b.fetch()
    assert np.array_equal(nh, n2) and hits.tobytes() == h2.tobytes()
    sample = np.sort(np.random.default_rng(0).choice(1024, 64, replace=False))
    st = np.concatenate([terms[off[q]:off[q + 1]] for q in sample]).astype(np.uint32)
    so = np.r_[0, np.cumsum([off[q + 1] - off[q] for q in sample])].astype(np.uint32)
    want = host_composition(hseg, gix, st, so, 10, G)
    for i, q in enumerate(sample):  # (row views: a fancy-indexed copy of a structured array leaves its padding bytes undefined)
        assert nh[q] == len(want[i]) and hits[q, :nh[q]].tobytes() == want[i].tobytes(), f"C3 q{q}: records differ"
