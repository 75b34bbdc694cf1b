"""TID sets on the device (csrc/tid.hip): vbm25_tid_set_*, vbm25_filter_set_tids, vbm25_device_growing_delete_tids and
vbm25_device_vacuum_bulkdelete.  The yardsticks are numpy (np.unique, np.isin on packed keys, DocFilter.pack) and the routes that
existed before: DocFilter.update with host-made words, GrowingSegment.delete with indices, DeviceVacuum.from_pages of pages the table
model patched as bulkdelete.rs does.  The new route is never compared against itself.  -m gpu only."""
import numpy as np
import pytest
import torch

import vectorchord_bm25_amd as vb
import table_model as T
from vectorchord_bm25_amd._lib import check
from corpus import make_queries
from growing_data import make_growing
from test_gpu_growing import _sealed
from test_gpu_growing_append import docs, same, with_deleted
from test_table_model import SEED32

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
NONE = vb.NO_FILTER
KEY = np.frombuffer(b"1".ljust(16, b"\0"), np.uint8).reshape(1, 16)
_C = {}


def cached(name, make):
    if name not in _C:
        _C[name] = make()
    return _C[name]


def keys_of(p):
    return vb.TidSet.keys(p)


def pack(bits):
    return vb.DocFilter.pack(np.asarray(bits, bool), len(bits))[0]


def tiny_index(payload):
    """an index of len(payload) documents with these payloads: one term, which every document holds once"""
    payload = np.asarray(payload, np.uint16).reshape(-1, 3)
    n = len(payload)
    if n == 0:
        meta = dict(n_docs=0, n_terms=0, n_blocks=0, sum_len=0, k1=1.2, b=0.75)
        arrays = {k: np.zeros(0, dtype=dt) for k, dt in vb.api._DESC_ARRAYS}
        arrays["term_first_block"] = np.zeros(1, dtype=np.uint32)
        arrays["blk_off8"] = np.zeros(1, dtype=np.uint32)
        desc, keep = vb.api.desc_from_arrays(meta, arrays)
        gix = vb.GpuIndex(desc)
        gix.keep = keep
        return gix
    seg = vb.Segment.build(1.2, 0.75, np.ones(n, np.uint32), payload, KEY, np.array([0, n], np.uint64), np.arange(n, dtype=np.uint32),
                           np.ones(n, np.uint32))
    return vb.GpuIndex(seg)


def random_payloads(n, seed, narrow=False):
    """payloads that collide in two of three fields (narrow: every field of few values, so whole payloads repeat too)"""
    rng = np.random.default_rng(seed)
    hi = (3, 3, 40) if narrow else (4, 5, 65536)
    return np.stack([rng.integers(0, h, n) for h in hi], axis=1).astype(np.uint16)


def assert_match(ts, gix_or_grow, payload, what, growing=False):
    words, n_match = ts.match_growing(gix_or_grow) if growing else ts.match(gix_or_grow)
    want = np.isin(keys_of(payload), keys_of(ts.read()))
    assert words.dtype == np.uint64 and np.array_equal(words, pack(want)), f"{what}: words differ at {np.flatnonzero(words != pack(want))[:8]}"
    assert n_match == int(want.sum()), f"{what}: n_match {n_match}, numpy {int(want.sum())}"
    return want


# ---- the set

@pytest.mark.parametrize("n", [0, 1, 2, 64, 65, 100_000])
def test_read_is_numpy_unique(n):
    rng = np.random.default_rng(n)
    pool = random_payloads(max(1, n // 8), n + 1)   # heavy repeats
    tids = pool[rng.integers(0, len(pool), n)]
    if n >= 2:
        tids[0], tids[-1] = (0, 0, 0), (65535, 65535, 65535)
    u = np.unique(keys_of(tids))
    for name, arr in (("as drawn", tids), ("sorted", tids[np.argsort(keys_of(tids), kind="stable")]),
                      ("reversed", tids[np.argsort(keys_of(tids), kind="stable")[::-1]]), ("all equal", np.repeat(tids[:1], n, axis=0))):
        with vb.TidSet(arr) as ts:
            want = np.unique(keys_of(arr))
            got = ts.read()
            assert ts.n_unique == len(want) and got.shape == (len(want), 3) and got.dtype == np.uint16, (n, name)
            assert np.array_equal(keys_of(got), want), (n, name)
            assert ts.device == 0 and ts.device_bytes() >= 8 * len(want)
    assert n < 2 or (u[0] == 0 and u[-1] == (1 << 48) - 1)


# ---- match against numpy

def sets_for(payload, rng):
    """(name, tids) over the documents' payloads: empty, one member, all, none present, every second; document 0 only, n - 1 only"""
    n = len(payload)
    absent = np.array([[7, 7, 7], [65535, 0, 1], [0, 65535, 65535]], np.uint16)
    absent = absent[~np.isin(keys_of(absent), keys_of(payload))]
    out = [("empty", np.zeros((0, 3), np.uint16)), ("none present", absent)]
    if n:
        out += [("one member", payload[[int(rng.integers(n))]]), ("all", payload), ("every second", payload[::2]),
                ("document 0", payload[:1]), ("document n - 1", payload[-1:]),
                ("every third and strangers", np.concatenate([payload[::3], absent]))]
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_match_small_indexes(n):
    rng = np.random.default_rng(n)
    payload = random_payloads(n, 100 + n)
    if n >= 65:
        payload[64] = payload[3]   # two documents share a payload: both bits
    gix = tiny_index(payload)
    for name, tids in sets_for(payload, rng):
        with vb.TidSet(tids) as ts:
            want = assert_match(ts, gix, payload, f"n={n} {name}")
            if name == "all":
                assert want.all()
            if name == "document 0" and n >= 65:
                assert want[0] and want.sum() == int((keys_of(payload) == keys_of(payload[:1])[0]).sum())
            if n >= 65 and name == "one member":
                with vb.TidSet(payload[[3]]) as two:
                    w = assert_match(two, gix, payload, "shared payload")
                    assert w[3] and w[64]
            # either output pointer may be NULL
            L = vb.lib()
            buf = np.zeros(max(1, (n + 63) // 64), np.uint64)
            assert L.vbm25_tid_set_match_index(ts.h, gix.h, buf.ctypes.data, None) == 0 and np.array_equal(buf[:(n + 63) // 64], pack(want))
            assert L.vbm25_tid_set_match_index(ts.h, gix.h, None, None) == 0


def big():
    def make():
        payload = random_payloads(70_000, 5)
        payload[69_999] = payload[0]
        return payload, tiny_index(payload)
    return cached("big", make)


@pytest.mark.parametrize("grid", [1, 3])
def test_match_70000_documents_grid_stride(tuning, grid):
    """1094 words under 1 and 3 workgroups of four waves: hundreds of grid-stride passes, the last word of 48 documents"""
    payload, gix = big()
    tuning(tid_grid=grid)
    rng = np.random.default_rng(grid)
    for name, tids in sets_for(payload, rng):
        with vb.TidSet(tids) as ts:
            assert_match(ts, gix, payload, f"grid={grid} {name}")


@pytest.mark.parametrize("tid_dir", [0, 2, None])
@pytest.mark.parametrize("n_set", [3, 4, 5, 5000])
def test_both_stages_of_the_search(tuning, tid_dir, n_set):
    """directories of 1, 4 and the default's entries against sets of 3, 4, 5 and 5000: the directory alone (set <= directory), one
    run of the whole set (tid_dir 0) and strides of 2 and 1250 that the HBM stage finishes"""
    payload, gix = big()
    if tid_dir is not None:
        tuning(tid_dir=tid_dir)
    rng = np.random.default_rng(n_set)
    members = payload[rng.choice(len(payload), n_set - n_set // 3, replace=False)]
    near = members[:n_set // 3].copy()
    near[:, 2] ^= 1   # strangers next to members
    with vb.TidSet(np.concatenate([members, near])) as ts:
        want = assert_match(ts, gix, payload, f"tid_dir={tid_dir} n_set={n_set}")
        assert want.sum() >= len(members)


def growing_case(n):
    def make():
        c, seg = cached("sealed", lambda: _sealed(3000, 300, seed=3))
        gix = cached("sealed gix", lambda: vb.GpuIndex(seg))
        G, _ = make_growing(seg.arrays()["term_key"], n + 40, seed=n + 1)
        G["g_payload"] = G["g_payload"].reshape(-1, 3).copy()
        if n + 40 > 10:
            G["g_payload"][7] = G["g_payload"][2]
        return c, seg, gix, G
    return cached(("growing", n), make)


@pytest.mark.parametrize("n", [0, 1, 64, 65, 1000])
def test_match_growing_and_after_an_append(n):
    c, seg, gix, G = growing_case(n)
    now = docs(G, 0, n)
    if n:
        now = with_deleted(now, np.arange(0, n, 3))   # deleted documents are matched like any other
    gs = vb.GrowingSegment(gix, **now)
    allp = G["g_payload"].reshape(-1, 3)
    rng = np.random.default_rng(n)
    with vb.TidSet(allp[::2]) as ts, vb.TidSet(np.zeros((0, 3), np.uint16)) as empty:
        w0 = assert_match(ts, gs, allp[:n], f"n_grow={n}", growing=True)
        assert_match(empty, gs, allp[:n], f"n_grow={n} empty set", growing=True)
        if n:
            gs.delete(np.array([n - 1], np.uint32))
            assert_match(ts, gs, allp[:n], f"n_grow={n} after a delete", growing=True)
        gs.append(**docs(G, n, n + 40))
        w1 = assert_match(ts, gs, allp, f"n_grow={n} + 40", growing=True)
        assert w1.sum() > w0.sum() and np.array_equal(w1[:n], w0)


# ---- DocFilter.set_tids

def filter_case():
    def make():
        c, seg, gix, G = growing_case(1000)
        n_g = 65
        now = with_deleted(docs(G, 0, n_g), [4, 40])
        gs = vb.GrowingSegment(gix, **now)
        sp, gp = c["doc_payload"].reshape(-1, 3), G["g_payload"].reshape(-1, 3)
        rng = np.random.default_rng(11)
        tids = np.concatenate([sp[rng.random(len(sp)) < 0.4], gp[:n_g][rng.random(n_g) < 0.5], np.array([[9, 9, 9]], np.uint16)])
        return c, seg, gix, G, now, gs, sp, gp[:n_g], tids
    return cached("filter", make)


@pytest.mark.parametrize("invert", [False, True])
def test_set_tids_equals_update_with_numpy_words(invert):
    c, seg, gix, G, now, gs, sp, gp, tids = filter_case()
    n, n_g = len(sp), len(gp)
    rng = np.random.default_rng(3)
    start = rng.random((3, n)) < 0.5
    gstart = rng.random((3, n_g)) < 0.5
    got, want = vb.DocFilter(gix, start), vb.DocFilter(gix, start)
    got.set_growing(gs, gstart)
    want.set_growing(gs, gstart)
    with vb.TidSet(tids) as ts:
        ks = np.isin(keys_of(sp), keys_of(tids)) != invert
        kg = np.isin(keys_of(gp), keys_of(tids)) != invert
        got.set_tids(1, ts, invert, gs)
        want.update(1, ks)
        want.update_growing(1, kg)
        for i in range(3):   # bitmap 1 word for word, the others untouched
            assert np.array_equal(got.read(i), want.read(i)) and np.array_equal(got.read(i, growing=True), want.read(i, growing=True)), i
        assert np.array_equal(got.read(0), pack(start[0])) and np.array_equal(got.read(2, growing=True), pack(gstart[2]))
        assert np.array_equal(got.read(1), pack(ks)) and np.array_equal(got.read(1, growing=True), pack(kg))
        # gs == None: the growing bitmaps are untouched
        got.set_tids(2, ts, invert)
        assert np.array_equal(got.read(2), pack(ks)) and np.array_equal(got.read(2, growing=True), pack(gstart[2]))


def test_set_tids_tail_bits_at_65_documents():
    payload = random_payloads(65, 9)
    gix = tiny_index(payload)
    c, seg, sgix, G = growing_case(65)
    G65 = docs(G, 0, 65)
    f = vb.DocFilter(gix, np.ones((1, 65), bool))
    with vb.TidSet(payload[:5]) as ts:
        f.set_tids(0, ts, invert=True)
        w = f.read(0)
        assert len(w) == 2 and int(w[1]) == 1 and np.array_equal(w, pack(~np.isin(keys_of(payload), keys_of(payload[:5]))))
    gs = vb.GrowingSegment(sgix, **G65)
    f2 = vb.DocFilter(sgix, np.zeros((1, sgix.n_docs), bool))
    f2.set_growing(gs)
    gp = G65["g_payload"].reshape(-1, 3)
    with vb.TidSet(gp[10:20]) as ts:
        f2.set_tids(0, ts, True, gs)
        w = f2.read(0, growing=True)
        assert len(w) == 2 and int(w[1]) == 1 and np.array_equal(w, pack(~np.isin(keys_of(gp), keys_of(gp[10:20]))))
        assert int(f2.read(0)[-1]) >> (sgix.n_docs % 64) == 0


def search_case():
    """60 000 sealed documents (the corpus on which the forced window route is taken) and 300 growing ones over the queries' terms"""
    def make():
        c, seg = _sealed(60_000, 4000, seed=8)
        gix = vb.GpuIndex(seg)
        terms, off = make_queries(c, 48, 4, seed=5)
        G, _ = make_growing(seg.arrays()["term_key"], 300, seed=9, pool=terms, pool_p=0.5)
        gs = vb.GrowingSegment(gix, **G)
        sp, gp = c["doc_payload"].reshape(-1, 3), G["g_payload"].reshape(-1, 3)
        rng = np.random.default_rng(11)
        tids = np.concatenate([sp[rng.random(len(sp)) < 0.4], gp[rng.random(len(gp)) < 0.5], np.array([[9, 9, 9]], np.uint16)])
        return c, seg, gix, G, gs, sp, gp, tids, terms, off
    return cached("search", make)


@pytest.mark.parametrize("case,tune,route", [("win", dict(fused=0, win_force=1), 3), ("general", dict(fused=0, arith=0, win=0), 0)])
def test_filtered_search_with_device_made_bitmaps(tuning, case, tune, route):
    """a resident Batch filtered by bitmaps made from TID sets on the device returns, record for record, what
    search_batch_growing_masked returns with the host-made bitmaps"""
    c, seg, gix, G, gs, sp, gp, tids, terms, off = search_case()
    ks = np.stack([np.isin(keys_of(sp), keys_of(tids)), ~np.isin(keys_of(sp), keys_of(tids))])
    kg = np.stack([np.isin(keys_of(gp), keys_of(tids)), ~np.isin(keys_of(gp), keys_of(tids))])
    host = vb.DocFilter(gix, ks)
    host.set_growing(gs, kg)
    dev = vb.DocFilter(gix, np.zeros((2, len(sp)), bool))
    dev.set_growing(gs)
    with vb.TidSet(tids) as ts:
        dev.set_tids(0, ts, False, gs)
        dev.set_tids(1, ts, True, gs)
    sel = np.array([(0, 1, NONE)[q % 3] for q in range(48)], np.uint32)
    want, n_want = vb.search_batch_growing_masked(gix, gs, terms, off, 10, host, sel)
    tuning(**tune)
    b = vb.Batch(gix, 48, len(terms), 10)
    b.set_growing(gs)
    b.set_filter(dev, sel)
    b.set_queries(terms, off)
    assert b.debug_route() == route, (case, b.debug_route())
    b.run()
    hits, nh = b.fetch()
    same(want, n_want, hits, nh, case)
    assert int(nh.sum()) > 100


def test_set_tids_refusals_leave_the_bitmaps():
    c, seg, gix, G = growing_case(1000)
    n = gix.n_docs
    gs = vb.GrowingSegment(gix, **docs(G, 0, 100))
    other = vb.GrowingSegment(gix, **docs(G, 0, 100))
    rng = np.random.default_rng(2)
    start, gstart = rng.random((2, n)) < 0.5, rng.random((2, 100)) < 0.5
    f = vb.DocFilter(gix, start)

    def unchanged(growing=True):
        assert all(np.array_equal(f.read(i), pack(start[i])) for i in range(2))
        assert not growing or all(np.array_equal(f.read(i, growing=True), pack(gstart[i])) for i in range(2))

    def refused(code, text, *args):
        with pytest.raises(vb.Vbm25Error) as e:
            f.set_tids(*args)
        assert e.value.code == code and text in str(e.value), str(e.value)

    with vb.TidSet(c["doc_payload"].reshape(-1, 3)[::2]) as ts:
        refused(UNSUPPORTED, "no growing bitmaps", 0, ts, False, gs)
        unchanged(growing=False)
        f.set_growing(gs, gstart)
        refused(INVALID, "another upload", 0, ts, False, other)
        refused(INVALID, "bitmap 2 of a filter of 2", 2, ts)
        refused(INVALID, "bitmap 7 of a filter of 2", 7, ts, True, gs)
        unchanged()
        gs.append(**docs(G, 100, 130))
        refused(INVALID, "appended to since", 1, ts, False, gs)   # stale growing bitmaps
        unchanged()
        f.extend_growing(gs)
        f.set_tids(1, ts, False, gs)   # ... and accepted once they are extended
        assert np.array_equal(f.read(1, growing=True), pack(np.isin(keys_of(G["g_payload"].reshape(-1, 3)[:130]), keys_of(ts.read()))))
        if torch.cuda.device_count() < 2:
            print("one device: the refusal of a set on another device than the filter's is not checked")
            return
        with vb.TidSet(ts.read(), device=1) as far:
            refused(INVALID, "the TID set is on device 1", 0, far)


# ---- GrowingSegment.delete_tids

@pytest.mark.parametrize("k", [1, 10, 1500])
def test_delete_tids_equals_delete_of_the_indices_numpy_finds(k):
    c, seg, gix, G = growing_case(1000)
    terms, off = make_queries(c, 16, 3, seed=k)
    pool = terms[terms < seg.n_terms]
    G2, _ = make_growing(seg.arrays()["term_key"], 1040, seed=21, pool=pool, pool_p=0.5)
    gp = G2["g_payload"].reshape(-1, 3).copy()
    gp[9] = gp[5]   # two rows of one TID go together
    G2["g_payload"] = gp
    first = with_deleted(docs(G2, 0, 1000), [1, 2, 3])
    a, b = vb.GrowingSegment(gix, **first), vb.GrowingSegment(gix, **first)

    def step(tids, what, expect=None):
        with vb.TidSet(tids) as ts:
            n = a.delete_tids(ts)
        found = np.flatnonzero(np.isin(keys_of(gp[:b.n_docs]), keys_of(tids)))
        b.delete(found.astype(np.uint32))
        assert n == len(found) and (expect is None or n == expect), (what, n, len(found))
        same(*vb.search_batch_growing(gix, b, terms, off, k), *vb.search_batch_growing(gix, a, terms, off, k), f"k={k} {what}")

    before = vb.search_batch_growing(gix, a, terms, off, k)
    step(np.array([[1, 1, 1]], np.uint16), "a set that matches nothing", 0)
    same(*before, *vb.search_batch_growing(gix, a, terms, off, k), "nothing matched: nothing changed")
    step(gp[[1, 2, 3]], "documents already deleted", 3)
    same(*before, *vb.search_batch_growing(gix, a, terms, off, k), "already deleted: nothing changed")
    rng = np.random.default_rng(k)
    step(np.concatenate([gp[rng.choice(1000, 300, replace=False)], gp[[5]]]), "300 documents and a shared TID")
    for s in (a, b):
        s.append(**docs(G2, 1000, 1040))
    step(np.zeros((0, 3), np.uint16), "a later append keeps them deleted", 0)
    step(gp[1000:1010], "the appended documents", 10)


# ---- DeviceVacuum.bulkdelete

def table():
    """(the model, copies of its pages, the index read from them): 700 sealed rows on two pages of the documents tape and 100 growing
    rows, five and three of them deleted in the pages already.  A fresh model per call: a test patches its pages."""
    rows, universe = cached("rows", lambda: T.random_rows(700, 120, 5, mean_len=20))
    m = T.Table(rows, 1.2, 0.75, SEED32)
    rng = np.random.default_rng(4)
    for i in range(100):
        keys = [universe[j] for j in rng.choice(len(universe), 5, replace=False)]
        if i % 10 == 0:
            keys[0] = T.new_key(i)
        m.insert((7, i // 50, i % 50 + 1), {key: int(tf) for key, tf in zip(keys, rng.integers(1, 5, 5))})
    for d in (0, 63, 64, 300, 699):
        m.delete_sealed(d)
    for g in (0, 50, 99):
        m.delete_growing(g)
    before = [np.array(p, copy=True) for p in m.page_list()]
    return m, before, vb.GpuIndex(vb.DeviceSegment.from_pages(before))


def bulkdelete_case(sealed_ids, growing_ids, extra=()):
    """the model deletes these rows by payload as bulkdelete.rs does; returns (handle after bulkdelete, handle of the patched pages,
    the counts returned, the model's counts of rows that were live, the index, the model, the pages before)"""
    m, before, gix = table()
    tids = [m.sealed[d][0] for d in sealed_ids] + [m.growing[g][0] for g in growing_ids] + list(extra)
    live_s = sum(not m.sealed_deleted[d] for d in set(sealed_ids))
    live_g = sum(not m.growing_deleted[g] for g in set(growing_ids))
    for d in sealed_ids:
        m.delete_sealed(d)
    for g in growing_ids:
        m.delete_growing(g)
    after = [np.array(p, copy=True) for p in m.page_list()]
    got = vb.DeviceVacuum.from_pages(gix, before)
    with vb.TidSet(np.array(tids, np.uint16).reshape(-1, 3)) as ts:
        counts = got.bulkdelete(gix, ts)
    return got, vb.DeviceVacuum.from_pages(gix, after), counts, (live_s, live_g), gix, m, before


def info(dv):
    ns, nsd, ng, ngd, ne = [np.zeros(1, np.uint32) for _ in range(4)] + [np.zeros(1, np.uint64)]
    check(vb.lib().vbm25_device_vacuum_info(dv.h, ns.ctypes.data, nsd.ctypes.data, ng.ctypes.data, ngd.ctypes.data, ne.ctypes.data))
    return int(ns[0]), int(nsd[0]), int(ng[0]), int(ngd[0]), int(ne[0])


def assert_same_handle(got, want, what):
    for a, b in zip(got.read(), want.read()):
        assert a.tobytes() == b.tobytes(), f"{what}: read() differs"
    assert info(got) == info(want), (what, info(got), info(want))
    assert (got.n_sealed_deleted, got.n_grow_deleted) == (want.n_sealed_deleted, want.n_grow_deleted), what


def test_bulkdelete_equals_the_patched_pages():
    rng = np.random.default_rng(8)
    sealed_ids = sorted(set(rng.choice(700, 150, replace=False).tolist() + [0, 63, 1, 65, 698]))   # 0 and 63 were deleted already
    growing_ids = sorted(set(rng.choice(100, 30, replace=False).tolist() + [0, 1, 98]))            # 0 was
    got, want, counts, live, gix, m, before = bulkdelete_case(sealed_ids, growing_ids, extra=[(60000, 1, 1)])
    dead_s, dead_g = len(set(sealed_ids) & {0, 63, 64, 300, 699}), len(set(growing_ids) & {0, 50, 99})
    assert dead_s >= 2 and dead_g >= 1 and counts == live == (len(sealed_ids) - dead_s, len(growing_ids) - dead_g)
    assert_same_handle(got, want, "bulkdelete")
    seg_got, rel_got = vb.DeviceSegment.maintain_device(gix, got, return_relabel=True)
    seg_want, rel_want = vb.DeviceSegment.maintain_device(gix, want, return_relabel=True)
    assert rel_got.tobytes() == rel_want.tobytes()
    a, b = seg_got.download(), seg_want.download()
    assert a.meta() == b.meta() and all(a.arrays()[k].tobytes() == v.tobytes() for k, v in b.arrays().items())
    # a two-bitmap filter carried across
    keeps = np.random.default_rng(1).random((2, 700)) < 0.5
    gkeeps = np.random.default_rng(2).random((2, 100)) < 0.5
    f = vb.DocFilter(gix, keeps)
    grow = vb.GrowingSegment.from_pages(gix, before)
    f.set_growing(grow, gkeeps)
    nix = vb.GpuIndex(seg_got)
    fa, fb = f.remap_device(nix, got), f.remap_device(nix, want)
    for i in (0, 1):
        assert np.array_equal(fa.read(i), fb.read(i)), i


@pytest.mark.parametrize("case", ["old deletions only", "the empty set", "absent TIDs"])
def test_bulkdelete_that_changes_nothing(case):
    sealed_ids, growing_ids, extra = {"old deletions only": ([0, 63, 64, 300, 699], [0, 50, 99], []), "the empty set": ([], [], []),
                                      "absent TIDs": ([], [], [(60000, 2, 2), (7, 9, 60), (65535, 65535, 65535)])}[case]
    got, want, counts, live, gix, m, before = bulkdelete_case(sealed_ids, growing_ids, extra)
    fresh = vb.DeviceVacuum.from_pages(gix, before)
    assert counts == (0, 0) == live
    assert_same_handle(got, fresh, case)
    assert_same_handle(got, want, case)


def test_bulkdelete_of_everything_and_of_another_index():
    got, want, counts, live, gix, m, before = bulkdelete_case(list(range(700)), list(range(100)))
    assert counts == live == (695, 97)
    assert_same_handle(got, want, "everything")
    seg = vb.DeviceSegment.maintain_device(gix, got)
    assert (seg.n_docs, seg.n_terms, seg.n_blocks) == (0, 0, 0)
    # an index of another document count: refused, the handle unchanged
    dv = vb.DeviceVacuum.from_pages(gix, before)
    words, g_del = dv.read()
    other = tiny_index(random_payloads(65, 1))
    with vb.TidSet(np.array([m.sealed[5][0]], np.uint16)) as ts:
        with pytest.raises(vb.Vbm25Error) as e:
            dv.bulkdelete(other, ts)
        assert e.value.code == INVALID and "the index holds 65" in str(e.value)
        assert dv.read()[0].tobytes() == words.tobytes() and dv.read()[1].tobytes() == g_del.tobytes() and info(dv)[1] == 5
        assert dv.bulkdelete(gix, ts) == (1, 0) and info(dv)[1] == 6
