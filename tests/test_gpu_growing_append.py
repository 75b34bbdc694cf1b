"""The device growing segment changed in place (vbm25_device_growing_append / _delete / _docs).  After every step the appended
segment's records are compared byte for byte with two yardsticks, never with itself: a FRESH GrowingSegment of the concatenated
documents (g_deleted set for the deleted ones) and the host composition merge_hits(search_batch, growing_search) of
tests/test_gpu_growing.py -- one-shot and through a resident Batch that was attached before the first append and never re-attached.
-m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_queries
from growing_data import make_growing
from lifecycle_data import Expect, check
from test_gpu_growing import ROUTES, _queries, _sealed, assert_records, check_both, host_composition
from test_gpu_growing_filter import expected as filtered_expected

pytestmark = pytest.mark.gpu
GT = 8192  # documents per tile of growing_scan_kernel
NONE = vb.NO_FILTER
INVALID = -1


def docs(G, a, b, rebase=True):
    """documents [a, b) of G as a CSR of their own; rebase=False keeps G's element arrays whole and lets start begin at G's offset"""
    s = G["g_start"].astype(np.int64)
    e0, e1 = (int(s[a]), int(s[b])) if rebase else (0, len(G["g_tf"]))
    return dict(g_start=(s[a:b + 1] - e0).astype(np.uint64), g_key=G["g_key"].reshape(-1, 16)[e0:e1].reshape(-1), g_tf=G["g_tf"][e0:e1],
                g_fieldnorm=G["g_fieldnorm"][a:b], g_payload=G["g_payload"][a:b],
                g_deleted=None if G["g_deleted"] is None else G["g_deleted"][a:b])


def concat(A, B):
    B = docs(B, 0, len(B["g_start"]) - 1)
    na, nb = len(A["g_start"]) - 1, len(B["g_start"]) - 1
    dele = None
    if A["g_deleted"] is not None or B["g_deleted"] is not None:
        dele = np.r_[A["g_deleted"] if A["g_deleted"] is not None else np.zeros(na, np.uint8),
                     B["g_deleted"] if B["g_deleted"] is not None else np.zeros(nb, np.uint8)].astype(np.uint8)
    return dict(g_start=np.r_[A["g_start"], B["g_start"][1:] + A["g_start"][-1]].astype(np.uint64),
                g_key=np.r_[A["g_key"].reshape(-1), B["g_key"].reshape(-1)], g_tf=np.r_[A["g_tf"], B["g_tf"]].astype(np.uint32),
                g_fieldnorm=np.r_[A["g_fieldnorm"], B["g_fieldnorm"]].astype(np.uint8),
                g_payload=np.concatenate([A["g_payload"].reshape(-1, 3), B["g_payload"].reshape(-1, 3)]).astype(np.uint16), g_deleted=dele)


def with_deleted(G, gone):
    out = dict(G)
    d = np.zeros(len(G["g_start"]) - 1, np.uint8) if G["g_deleted"] is None else G["g_deleted"].copy()
    d[np.asarray(gone, np.int64)] = 1
    out["g_deleted"] = d
    return out


def same(hits, nh, h2, n2, what):
    assert np.array_equal(nh, n2), f"{what}: counts differ"
    for q in range(len(nh)):
        assert hits[q, :nh[q]].tobytes() == h2[q, :nh[q]].tobytes(), f"{what} q{q}: records differ"


def check_step(seg, gix, gs, batches, terms, off, Gnow, what, ks=None):
    """the appended segment `gs` against a fresh upload of Gnow and the host composition, one-shot and through the resident batches
    {k: Batch} (attached before the first append)"""
    n = len(Gnow["g_start"]) - 1
    assert gs.n_docs == n, f"{what}: n_docs {gs.n_docs}, want {n}"
    fresh = vb.GrowingSegment(gix, **Gnow)
    for k in (ks if ks is not None else sorted(batches)):
        want = host_composition(seg, gix, terms, off, k, Gnow)
        fh, fn = vb.search_batch_growing(gix, fresh, terms, off, k)
        hits, nh = vb.search_batch_growing(gix, gs, terms, off, k)
        assert_records(want, hits, nh, f"{what} k={k} one-shot against the host composition")
        same(fh, fn, hits, nh, f"{what} k={k} one-shot against a fresh upload")
        if k in batches:
            batches[k].run()
            h2, n2 = batches[k].fetch()
            assert_records(want, h2, n2, f"{what} k={k} resident batch against the host composition")
            same(fh, fn, h2, n2, f"{what} k={k} resident batch against a fresh upload")


def attach(gix, gs, terms, off, ks):
    out = {}
    for k in ks:
        b = vb.Batch(gix, len(off) - 1, max(1, len(terms)), k)
        b.set_growing(gs)
        b.set_queries(terms, off)
        out[k] = b
    return out


_C = {}


def _base():
    if "A" not in _C:
        c, seg = _sealed(20_000, 1500, seed=3)
        _C["A"] = (c, seg, vb.GpuIndex(seg))
    return _C["A"]


@pytest.mark.parametrize("k", [1, 10, 100, 256, 1000, 1500])
def test_append_sequence_across_tile_boundaries(k):
    """5000 documents, then deltas of 1, 7, one that lands exactly on GT, +1, and 3 GT + 5 in one call: tile tables appear with the
    second tile and terms lose them again as n_tiles grows"""
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=k)
    total = 4 * GT + 6
    G, _ = make_growing(seg.arrays()["term_key"], total, seed=k + 40, pool=terms[terms < seg.n_terms])
    n = 5000
    gs = vb.GrowingSegment(gix, **docs(G, 0, n))
    batches = attach(gix, gs, terms, off, [k])
    check_step(seg, gix, gs, batches, terms, off, docs(G, 0, n), f"k={k} upload")
    for step, m in enumerate([1, 7, GT - n - 8, 1, 3 * GT + 5]):
        gs.append(**docs(G, n, n + m, rebase=bool(step % 2)))  # (a start array that begins anywhere, as upload takes it)
        n += m
        check_step(seg, gix, gs, batches, terms, off, docs(G, 0, n), f"k={k} after {n} documents")
    assert n == total


def test_upload_of_nothing_empty_and_unknown_deltas():
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=5)
    key = seg.arrays()["term_key"]
    G, _ = make_growing(key, 900, seed=9, deleted=None, pool=terms[terms < seg.n_terms])  # no deleted array
    assert G["g_deleted"] is None
    gs = vb.GrowingSegment(gix, **docs(G, 0, 0))
    assert gs.n_docs == 0
    batches = attach(gix, gs, terms, off, [10, 1500])
    gs.append(**docs(G, 0, 300))
    check_step(seg, gix, gs, batches, terms, off, docs(G, 0, 300), "append to an empty upload")
    before = gs.device_bytes
    gs.append(**docs(G, 300, 300))  # an empty delta: VBM25_OK, nothing changes
    assert gs.n_docs == 300 and gs.device_bytes == before
    check_step(seg, gix, gs, batches, terms, off, docs(G, 0, 300), "empty delta")
    U, _ = make_growing(key[:0], 120, seed=2, n_unknown=40)  # keys the sealed segment lacks only; this delta has a deleted array
    gs.append(**U)
    now = concat(docs(G, 0, 300), U)
    check_step(seg, gix, gs, batches, terms, off, now, "delta of unknown keys")
    gs.append(**docs(G, 300, 900))
    now = concat(now, docs(G, 300, 900))
    check_step(seg, gix, gs, batches, terms, off, now, "delta without a deleted array behind one with")
    D, _ = make_growing(key, 500, seed=11, deleted=0.3, pool=terms[terms < seg.n_terms])
    gs.append(**D)
    check_step(seg, gix, gs, batches, terms, off, concat(now, D), "delta with deleted documents")


def test_two_hundred_single_document_appends():
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=6)
    G, _ = make_growing(seg.arrays()["term_key"], GT + 100, seed=21, pool=terms[terms < seg.n_terms], pool_p=0.5)
    n = GT - 100  # (the run crosses into the second tile)
    gs = vb.GrowingSegment(gix, **docs(G, 0, n))
    batches = attach(gix, gs, terms, off, [10])
    for i in range(200):
        gs.append(**docs(G, n, n + 1))
        n += 1
        if i + 1 in (50, 100, 150, 200):
            check_step(seg, gix, gs, batches, terms, off, docs(G, 0, n), f"{i + 1} single appends", ks=[10, 1025] if i == 199 else None)


def _copies(c, seg, chosen, rep):
    """growing copies of sealed documents: same terms, tfs and fieldnorm, so the same score bits"""
    a = seg.arrays()
    key = a["term_key"].reshape(-1, 16)
    term_start, post_doc, post_tf = c["term_start"], c["post_doc"], c["post_tf"]
    rank_of = np.repeat(np.arange(len(term_start) - 1), np.diff(term_start.astype(np.int64)))
    starts, keys, tfs, fns, pls = [0], [], [], [], []
    for d in chosen:
        sel = np.nonzero(post_doc == d)[0]
        r = rank_of[sel]
        o = np.argsort(r)
        keys.append(key[r[o]].reshape(-1))
        tfs.append(post_tf[sel][o])
        starts.append(starts[-1] + len(sel))
        fns.append(a["doc_fieldnorm"][d])
        pls.append([rep, int(d) & 0xFFFF, 7])
    G = dict(g_start=np.array(starts, np.uint64), g_key=np.concatenate(keys), g_tf=np.concatenate(tfs).astype(np.uint32),
             g_fieldnorm=np.array(fns, np.uint8), g_payload=np.array(pls, np.uint16), g_deleted=None)
    rows = []
    for d in chosen[:24]:
        r = np.sort(rank_of[post_doc == d])
        rows.append(r[:min(len(r), 1 + len(rows) % 5)])
    return G, rows


def test_ties_of_appended_documents():
    """An appended document identical to an earlier growing one ranks behind it (order by g); both tie the sealed document they
    copy, which comes first -- also at rank k."""
    c, seg, gix = _base()
    chosen = np.random.default_rng(4).choice(seg.n_docs, 40, replace=False)
    G0, rows = _copies(c, seg, chosen, 0)
    G1, _ = _copies(c, seg, chosen, 1)
    terms = np.concatenate(rows).astype(np.uint32)
    off = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint32)
    G0 = concat(G0, _empty_docs(GT - 40))  # (the appended copies lie in the second tile)
    gs = vb.GrowingSegment(gix, **G0)
    ks = [1, 2, 4, 10, 1500]
    batches = attach(gix, gs, terms, off, ks)
    gs.append(**G1)
    now = concat(G0, G1)
    check_step(seg, gix, gs, batches, terms, off, now, "ties")
    want = host_composition(seg, gix, terms, off, 10, now)
    assert sum(int((np.diff(w["score"]) == 0).sum()) for w in want) > 0
    assert ties_cut_at_rank_k(host_composition(seg, gix, terms, off, 3, now)) == (True, True)


def _empty_docs(n):
    return dict(g_start=np.zeros(n + 1, np.uint64), g_key=np.zeros(0, np.uint8), g_tf=np.zeros(0, np.uint32),
                g_fieldnorm=np.zeros(n, np.uint8), g_payload=np.zeros((n, 3), np.uint16), g_deleted=None)


def ties_cut_at_rank_k(top3):
    """from the top-3 records: (some query's sealed hit ties a growing copy exactly where k = 1 cuts, some query's uploaded copy ties
    its appended copy exactly where k = 2 cuts) -- so the k = 1 and k = 2 comparisons above decide such ties"""
    grow = [w["doc_id"] > 0xFFFFFFFF - (GT + 40) for w in top3]
    at1 = any(len(w) >= 2 and w["score"][0] == w["score"][1] and not g[0] and g[1] for w, g in zip(top3, grow))
    at2 = any(len(w) == 3 and w["score"][1] == w["score"][2] and g[1] and g[2] for w, g in zip(top3, grow))
    return at1, at2


def test_bigk_batch_sized_for_the_small_segment():
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=8)
    G, _ = make_growing(seg.arrays()["term_key"], 2 * GT + 50, seed=31, pool=terms[terms < seg.n_terms])
    gs = vb.GrowingSegment(gix, **docs(G, 0, 100))
    batches = attach(gix, gs, terms, off, [1500, 1025])
    batches[1500].run()  # (scratch in use at the small size)
    gs.append(**docs(G, 100, 2 * GT + 50))
    check_step(seg, gix, gs, batches, terms, off, G, "k > 1024 after the segment outgrew the batch's scratch")
    assert sum(int((w["doc_id"] > 0xFFFFFFFF - (2 * GT + 50)).sum()) for w in host_composition(seg, gix, terms, off, 1500, G)) > 1024


@pytest.mark.parametrize("k", [10, 1500])
def test_deletes(k):
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=k + 1)
    G, _ = make_growing(seg.arrays()["term_key"], 3 * GT + 200, seed=17, pool=terms[terms < seg.n_terms], pool_p=0.5)
    n = 2 * GT + 100
    now = docs(G, 0, n)
    gs = vb.GrowingSegment(gix, **now)
    batches = attach(gix, gs, terms, off, [k])
    rng = np.random.default_rng(k)
    gone = rng.choice(n, 700, replace=False)
    gs.delete(gone)
    now = with_deleted(now, gone)
    check_step(seg, gix, gs, batches, terms, off, now, "random subset")
    tile = np.arange(GT, 2 * GT)
    gs.delete(tile)  # every document of one tile, many of them deleted already
    now = with_deleted(now, tile)
    check_step(seg, gix, gs, batches, terms, off, now, "a whole tile")
    again = np.r_[gone[:50], gone[:50], np.uint32(3), np.uint32(3)]
    gs.delete(again)  # repeated and already deleted indices
    now = with_deleted(now, again)
    check_step(seg, gix, gs, batches, terms, off, now, "repeats")
    gs.append(**docs(G, n, 3 * GT + 200))  # delete -> append -> delete: the deleted stay deleted
    now = concat(now, docs(G, n, 3 * GT + 200))
    check_step(seg, gix, gs, batches, terms, off, now, "append after deletes")
    late = rng.choice(3 * GT + 200, 900, replace=False)
    gs.delete(late)
    now = with_deleted(now, late)
    check_step(seg, gix, gs, batches, terms, off, now, "delete after the append")
    gs.delete(np.zeros(0, np.uint32))
    live = int(np.nonzero(now["g_deleted"] == 0)[0][0])
    with pytest.raises(vb.Vbm25Error) as e:
        gs.delete(np.array([live, gs.n_docs], np.uint32))  # nothing changes: the live document stays
    assert e.value.code == INVALID
    check_step(seg, gix, gs, batches, terms, off, now, "after a refused delete")


def test_failed_appends_leave_the_segment_as_it_was():
    c, seg, gix = _base()
    terms, off = _queries(c, seg, seed=12)
    G, _ = make_growing(seg.arrays()["term_key"], 700, seed=7, pool=terms[terms < seg.n_terms])
    now = docs(G, 0, 600)
    gs = vb.GrowingSegment(gix, **now)
    batches = attach(gix, gs, terms, off, [10, 1500])
    gs.append(**docs(G, 600, 640))  # (spares and stage exist: a failure would have something to spoil)
    now = docs(G, 0, 640)
    delta = docs(G, 640, 700)
    bad_keys = dict(delta)
    s = delta["g_start"].astype(np.int64)
    assert s[3] - s[2] >= 2
    keys = delta["g_key"].reshape(-1, 16).copy()
    keys[[s[2], s[2] + 1]] = keys[[s[2] + 1, s[2]]]  # the third document's keys out of order
    bad_keys["g_key"] = keys.reshape(-1)
    not_monotone = dict(delta)
    st = delta["g_start"].copy()
    st[5] = st[6] + 1
    not_monotone["g_start"] = st
    beyond = dict(delta)
    st = delta["g_start"].copy()
    st[-1] += 3  # reaches past n_elements
    beyond["g_start"] = st
    before = gs.device_bytes
    for name, bad in (("unsorted keys", bad_keys), ("start not monotone", not_monotone), ("start beyond n_elements", beyond)):
        with pytest.raises(vb.Vbm25Error) as e:
            gs.append(**bad)
        assert e.value.code == INVALID, name
        assert gs.n_docs == 640 and gs.device_bytes == before, name
        check_step(seg, gix, gs, batches, terms, off, now, f"after a failed append ({name})")
    gs.append(**delta)
    check_step(seg, gix, gs, batches, terms, off, docs(G, 0, 700), "the good delta afterwards")


def test_filters_are_stale_after_an_append_until_set_again():
    c, seg = _sealed(60_000, 4000, seed=8)
    gix = vb.GpuIndex(seg)
    ex = Expect(seg)
    nq, k = 30, 10
    terms, off = make_queries(c, nq, 4, seed=77)
    n0, n1 = GT + 300, 3 * GT + 40
    G, _ = make_growing(seg.arrays()["term_key"], n1, seed=5, pool=terms, pool_p=0.4)
    now = docs(G, 0, n0)
    gs = vb.GrowingSegment(gix, **now)
    rng = np.random.default_rng(1)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, np.arange(seg.n_docs) % 3 == 0, np.zeros(seg.n_docs, bool)])
    sel = np.array([[NONE, 0, 1, 2][q % 4] for q in range(nq)], np.uint32)

    def gkeeps_for(n):
        half = rng.random(n) < 0.5
        only_appended = np.arange(n) >= n0  # clustered: the tile skip meets the appended tiles
        return np.stack([half, only_appended, np.zeros(n, bool)])

    f = vb.DocFilter(gix, keeps)
    gk = gkeeps_for(n0)
    f.set_growing(gs, gk)
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_filter(f, sel)
    b.set_growing(gs)
    b.set_queries(terms, off)
    b.run()
    check(filtered_expected(ex, terms, off, k, now, keeps, gk, sel), *b.fetch(), "filtered before the append")
    # a delete leaves the bitmaps valid
    gone = rng.choice(n0, 400, replace=False)
    gs.delete(gone)
    now = with_deleted(now, gone)
    b.run()
    check(filtered_expected(ex, terms, off, k, now, keeps, gk, sel), *b.fetch(), "filtered after a delete")
    h, n = vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    check(filtered_expected(ex, terms, off, k, now, keeps, gk, sel), h, n, "one-shot filtered after a delete")
    # an append makes them stale: INVALID from the run and from the one-shot call, both counts in the message
    gs.append(**docs(G, n0, n1))
    now = concat(now, docs(G, n0, n1))
    with pytest.raises(vb.Vbm25Error) as e:
        b.run()
    assert e.value.code == INVALID and str(n0) in str(e.value) and str(n1) in str(e.value)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    assert e.value.code == INVALID and str(n0) in str(e.value) and str(n1) in str(e.value)
    b2 = vb.Batch(gix, nq, len(terms), k)
    b2.set_growing(gs)
    with pytest.raises(vb.Vbm25Error) as e:
        b2.set_filter(f, sel)
    assert e.value.code == INVALID
    # the batch stays usable: without the filter it gives the unfiltered records
    b.set_filter(None)
    b.run()
    assert_records(host_composition(seg, gix, terms, off, k, now), *b.fetch(), "filter detached after the refused run")
    # bitmaps of the new size
    gk = gkeeps_for(n1)
    f.set_growing(gs, gk)
    b.set_filter(f, sel)
    b.run()
    want = filtered_expected(ex, terms, off, k, now, keeps, gk, sel)
    check(want, *b.fetch(), "filtered after set_growing")
    h, n = vb.search_batch_growing_masked(gix, gs, terms, off, k, f, sel)
    check(want, h, n, "one-shot filtered after set_growing")
    appended = [w[(w["doc_id"] > 0xFFFFFFFF - n1)] for q, w in enumerate(want) if sel[q] == 1]
    assert sum(len(a) for a in appended) > 0 and all((0xFFFFFFFF - a["doc_id"] >= n0).all() for a in appended)
    assert all(int((w["doc_id"] > 0xFFFFFFFF - n1).sum()) == 0 for q, w in enumerate(want) if sel[q] == 2)  # keep-none
    bk = vb.Batch(gix, nq, len(terms), 1500)
    bk.set_filter(f, sel)
    bk.set_growing(gs)
    bk.set_queries(terms, off)
    bk.run()
    check(filtered_expected(ex, terms, off, 1500, now, keeps, gk, sel), *bk.fetch(), "filtered k=1500 after set_growing")


def test_append_to_a_segment_of_an_empty_sealed_index():
    """no sealed terms: no growing document can score, before or after an append, and the calls work on zero-length term arrays"""
    meta = dict(n_docs=0, n_terms=0, n_blocks=0, sum_len=0, k1=1.2, b=0.75)
    arrays = {k: np.zeros(0, dtype=dt) for k, dt in vb.api._DESC_ARRAYS}
    arrays["term_first_block"] = np.zeros(1, dtype=np.uint32)
    arrays["blk_off8"] = np.zeros(1, dtype=np.uint32)
    desc, keep = vb.api.desc_from_arrays(meta, arrays)
    gix = vb.GpuIndex(desc)
    G, _ = make_growing(np.zeros((0, 16), np.uint8), 150, seed=3)
    gs = vb.GrowingSegment(gix, **docs(G, 0, 100))
    gs.append(**docs(G, 100, 150))
    gs.delete(np.array([3, 120], np.uint32))
    assert gs.n_docs == 150
    for k in (10, 2000):
        hits, nh = vb.search_batch_growing(gix, gs, np.array([0, 5], np.uint32), np.array([0, 1, 2], np.uint32), k)
        assert nh.tolist() == [0, 0]


@pytest.mark.parametrize("case,tune,k,nq,route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_sealed_route_after_an_append(tuning, case, tune, k, nq, route):
    if case == "win_giveups":
        c, seg = _sealed(200_000, 3000, seed=2, mean_len=60)
    else:
        c, seg = _sealed(60_000, 4000, seed=8)
    tuning(**tune)
    gix = vb.GpuIndex(seg)
    terms, off = make_queries(c, nq, 4, seed=nq + k)
    G, _ = make_growing(seg.arrays()["term_key"], GT + 100, seed=1, pool=terms, pool_p=0.4)
    gs = vb.GrowingSegment(gix, **docs(G, 0, GT - 50))
    gs.append(**docs(G, GT - 50, GT + 100))
    check_both(seg, gix, gs, terms, off, k, G, case, tuning_route=route)
    fresh = vb.GrowingSegment(gix, **G)
    same(*vb.search_batch_growing(gix, fresh, terms, off, k), *vb.search_batch_growing(gix, gs, terms, off, k), f"{case} against a fresh upload")


def test_capacity_grows_geometrically():
    """1024 single-document appends onto 16 documents (one tile throughout: no tile tables, three buffer groups grow): what the
    segment has allocated never shrinks and changes fewer than 128 times.  Linear growth would change it about 1024 times; any
    geometric policy with a factor of 1.25 or more over three buffer groups stays below 3 log_1.25(1024) = 93."""
    c, seg, gix = _base()
    G, _ = make_growing(seg.arrays()["term_key"], 16 + 1024, seed=3)
    gs = vb.GrowingSegment(gix, **docs(G, 0, 16))
    sizes = [gs.device_bytes]
    for i in range(1024):
        gs.append(**docs(G, 16 + i, 17 + i))
        sizes.append(gs.device_bytes)
    assert gs.n_docs == 1040
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), "device_bytes decreased"
    assert len(set(sizes)) < 128, f"{len(set(sizes))} distinct sizes"
    terms, off = _queries(c, seg, seed=2)
    check_step(seg, gix, gs, {}, terms, off, G, "after 1024 single appends", ks=[10])


def test_full_size_c3():
    """C3's 10 M-document device index, 100 000 growing documents uploaded, three appends of 1 000 and a delete of 500: the whole
    1024-query batch equals a fresh upload's, a 64-query sample the host composition."""
    from bench import make_queries as bench_queries
    dseg = vb.DeviceSegment.synth(10_000_000, 30_000, mean_len=100, len_mode=1, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    terms, off = bench_queries(dseg, 30_000, 1024, 5, seed=3, zipf_s=0.0)
    hseg = dseg.download()
    G, _ = make_growing(hseg.arrays()["term_key"], 103_000, seed=11, mean_elems=60)
    gs = vb.GrowingSegment(gix, **docs(G, 0, 100_000))
    b = vb.Batch(gix, 1024, len(terms), 10)
    b.set_growing(gs)
    b.set_queries(terms, off)
    b.run()
    for i in range(3):
        gs.append(**docs(G, 100_000 + 1000 * i, 101_000 + 1000 * i))
    gone = np.random.default_rng(5).choice(103_000, 500, replace=False)
    gs.delete(gone)
    now = with_deleted(G, gone)
    assert gs.n_docs == 103_000
    fresh = vb.GrowingSegment(gix, **now)
    fh, fn = vb.search_batch_growing(gix, fresh, terms, off, 10)
    hits, nh = vb.search_batch_growing(gix, gs, terms, off, 10)
    same(fh, fn, hits, nh, "C3 one-shot against a fresh upload")
    b.run()
    h2, n2 = b.fetch()
    same(fh, fn, h2, n2, "C3 resident batch against a fresh upload")
    sample = np.sort(np.random.default_rng(0).choice(1024, 64, replace=False))
    st = np.concatenate([terms[off[q]:off[q + 1]] for q in sample]).astype(np.uint32)
    so = np.r_[0, np.cumsum([off[q + 1] - off[q] for q in sample])].astype(np.uint32)
    want = host_composition(hseg, gix, st, so, 10, now)
    for i, q in enumerate(sample):
        assert nh[q] == len(want[i]) and hits[q, :nh[q]].tobytes() == want[i].tobytes(), f"C3 q{q}: records differ"
