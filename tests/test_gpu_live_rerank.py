"""The rerank stack on a live table, on the GPU (csrc/live.hip, csrc/reranker.hip): DocTerms.append_documents / append against a fresh
Documents.bind of the concatenation -- arrays by np.array_equal, scores bit for bit, rows byte for byte -- on documents-bound and
index-bound handles; Reranker.sync against a fresh reranker on the fresh handle at both sort paths and every directory shape; the
snapshot rule on a ring; what the calls allocate; every refusal with code and message; a growing segment and an index-bound handle fed
the same deltas.  The documents and queries are those of tests/test_gpu_evaluate_documents.py.  -m gpu only."""
import math

import numpy as np
import pytest

import cast_model as cm
import test_gpu_evaluate_documents as ev
import vectorchord_bm25_amd as vb
from test_gpu_rerank import lists_csr
from test_gpu_reranker import same

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
GROWTH = 2  # the factor include/vbm25.h documents for every capacity of an append and a sync
CUTS = (0, 1, 63, 64, 65, 299, 300)
CAPS = dict(max_queries=16, max_lexemes=1024, max_bytes=1 << 16, max_candidates=40000, max_k=1024)
N = 300


def unique_payloads(n, seed):
    """n distinct ctids, shuffled"""
    rng = np.random.default_rng(seed)
    flat = rng.choice(1 << 24, n, replace=False).astype(np.uint64) * 977 + 13
    return np.stack([(flat >> 32) & 0xFFFF, (flat >> 16) & 0xFFFF, flat & 0xFFFF], axis=1).astype(np.uint16)


def corpus():
    """test_gpu_evaluate_documents' scored documents (0 .. 5000 lexemes; only unknown keys, unknown keys first, last and interleaved)
    filled up to 300"""
    docs = ev.scored_docs()
    docs += cm.corpus(ev.KNOWN[:30] + ev.UNKNOWN[:4], N - len(docs), seed=12)
    assert len(docs) == N
    return docs


def cast(docs, pay):
    return vb.Documents.cast(docs, pay, seed=cm.SEED)


def fieldnorms(dt):
    import ctypes as C
    f = vb.lib().vbm25_debug_doc_terms_fieldnorm
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 3
    out, flag = np.zeros(max(dt.n_docs, 1), np.uint8), C.c_uint32()
    assert f(dt.h, out.ctypes.data, C.byref(flag)) == 0
    return out[:dt.n_docs], flag.value


@pytest.fixture(scope="module")
def world():
    return ev.World(ev.KNOWN)


@pytest.fixture(scope="module")
def live(world):
    """the corpus, its payloads, the fresh handle with its arrays and its cross-product scores (computed once, left unchanged)"""
    docs, pay = corpus(), unique_payloads(N, 1)
    all_docs = cast(docs, pay)
    fresh = all_docs.bind(world.resolver)
    queries = ev.query_batch()[:16]
    ids, off = world.resolve(queries)
    m = dict(world=world, docs=docs, pay=pay, all=all_docs, fresh=fresh, arrays=fresh.download(), fn=fieldnorms(fresh)[0], queries=queries,
             ids=ids, off=off, cross=fresh.evaluate(ids, off))
    assert m["cross"].any()
    return m


def assert_prefix(dt, m, n, what, index_bound=False):
    """the handle's n documents are the fresh handle's first n: arrays, fieldnorm codes and the cross product's bits"""
    start, term, tf = dt.download()
    f_start, f_term, f_tf = m["arrays"]
    nk = int(f_start[n])
    assert dt.n_docs == n and dt.n_known == nk, what
    assert np.array_equal(start, f_start[:n + 1]) and np.array_equal(term, f_term[:nk]) and np.array_equal(tf, f_tf[:nk]), what
    fn, flag = fieldnorms(dt)
    assert np.array_equal(fn, m["fn"][:n]) and flag == int(index_bound), what
    if n:
        got = dt.evaluate(m["ids"], m["off"])
        assert np.array_equal(ev.bits(got), ev.bits(m["cross"][:, :n])), f"{what}: scores differ"


# ---- 1. the handle against a fresh bind


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("cut", CUTS)
def test_append_documents_equals_the_fresh_bind(live, cut, grid):
    m = live
    vb.set_tuning("eval_grid", grid)
    try:
        dt = cast(m["docs"][:cut], m["pay"][:cut]).bind(m["world"].resolver)
        assert dt.base_docs == cut
        second = cut + (N - cut) // 3  # (two deltas: the second lands behind an appended one, in the room to spare or past it)
        for a, b in ((cut, second), (second, N)):
            dt.append_documents(cast(m["docs"][a:b], m["pay"][a:b]), m["world"].resolver)
            assert_prefix(dt, m, b, f"cut {cut}, grid {grid}, up to {b}")
        assert dt.base_docs == cut and dt.device_bytes() >= 8 * (N + 1) + 8 * dt.n_known + N + 6 * (N - cut)
    finally:
        vb.reset_tuning()


def test_single_document_appends_and_what_a_sync_allocates(live):
    """200 appends of one document behind a base of 100, a sync after each: the handle equals the fresh one's prefix after every append,
    the directory follows, and the reranker allocates in no more rounds than doubling from its starting capacity allows"""
    m = live
    res = m["world"].resolver
    dt = cast(m["docs"][:100], m["pay"][:100]).bind(res)
    with dt.reranker(res, 2, **CAPS, documents=cast(m["docs"][:100], m["pay"][:100])) as r:
        made, moved = r.allocations(), 0
        for n in range(100, N):
            dt.append_documents(cast(m["docs"][n:n + 1], m["pay"][n:n + 1]), res)
            assert_prefix(dt, m, n + 1, f"after document {n}")
            assert r.directory_docs == n
            r.sync()
            assert r.directory_docs == n + 1
            moved += r.allocations() != made
            made = r.allocations()
        # the sorted arrays start at 100 entries and at least double: ceil(log2(300 / 100)) growth steps; the first sync also makes
        # what no later one makes again (the spare directory, the events, the delta's scratch) -- and is itself a growth step
        bound = math.ceil(math.log(N / 100) / math.log(GROWTH))
        assert 1 <= moved <= bound, (moved, bound)
        with m["fresh"].reranker(res, 2, **CAPS, documents=m["all"]) as want:
            q_cand, tids = lists_csr([np.arange(N)] * 4)
            tids = m["pay"][tids.astype(np.int64)]
            r.submit(m["queries"][5:9], 10, q_cand, cand_tid=tids)
            want.submit(m["queries"][5:9], 10, q_cand, cand_tid=tids)
            same(r.collect(), want.collect(), "after 200 syncs")


@pytest.fixture(scope="module")
def sealed_worlds(live):
    """per cut: the index built from the first `cut` documents on the device, its resolver, the fresh bind of all documents to it"""
    made = {}

    def get(cut):
        if cut not in made:
            m = live
            gix = vb.GpuIndex(vb.DeviceSegment.from_documents(cast(m["docs"][:cut], m["pay"][:cut]), 1.2, 0.75))
            res = vb.Resolver(gix, 1, 64, 4096, 1 << 18, seed=cm.SEED)
            fresh = m["all"].bind(res)
            res.submit(m["queries"])
            ids, off = res.collect()
            made[cut] = dict(m, gix=gix, resolver=res, fresh=fresh, arrays=fresh.download(), fn=fieldnorms(fresh)[0], ids=ids, off=off,
                             cross=fresh.evaluate(ids, off))
        return made[cut]
    return get


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("cut", [c for c in CUTS if c])  # (an index needs a sealed document)
def test_append_to_an_index_bound_handle(sealed_worlds, cut, grid):
    w = sealed_worlds(cut)
    vb.set_tuning("eval_grid", grid)
    try:
        dt = w["gix"].bind()
        assert_prefix(dt, w, cut, f"the bind of {cut}", index_bound=True)
        second = cut + (N - cut) // 2
        for a, b in ((cut, second), (second, N)):
            dt.append_documents(cast(w["docs"][a:b], w["pay"][a:b]), w["resolver"])
            assert_prefix(dt, w, b, f"index of {cut}, grid {grid}, up to {b}", index_bound=True)
        assert dt.base_docs == cut
    finally:
        vb.reset_tuning()


@pytest.mark.parametrize("grid", [1, 3])
def test_append_from_the_host_csr_with_deleted_documents(live, grid):
    """the CSR Documents.download() gives, some documents flagged: those have empty runs, their followers the right indices"""
    m = live
    res = m["world"].resolver
    cut = 64
    dl = m["all"].download()
    deleted = np.zeros(N, np.uint8)
    deleted[[cut, cut + 1, 100, ev.EDGE["5000 elements"], N - 1]] = 1
    live_docs = [([] if deleted[i] else d) for i, d in enumerate(m["docs"])]
    want = cast(live_docs, m["pay"]).bind(res).download()
    vb.set_tuning("eval_grid", grid)
    try:
        dt = cast(m["docs"][:cut], m["pay"][:cut]).bind(res)
        for a, b in ((cut, 200), (200, N)):  # (neither CSR's start begins at 0: a window into the whole arrays)
            dt.append(dl["g_start"][a:b + 1], dl["g_key"], dl["g_tf"], dl["g_fieldnorm"][a:b], dl["g_payload"][a:b], res, g_deleted=deleted[a:b])
        got = dt.download()
        for g, w, name in zip(got, want, ("start", "term", "tf")):
            assert np.array_equal(g, w), name
        assert dt.n_docs == N and np.array_equal(fieldnorms(dt)[0], m["fn"])  # (a deleted document keeps the code it came with)
        for d in np.flatnonzero(deleted):
            assert got[0][d] == got[0][d + 1]
        with dt.reranker(res, 1, **CAPS, documents=cast(m["docs"][:cut], m["pay"][:cut])) as r:  # (create on a grown handle: the tail's ctids)
            assert r.directory_docs == N
            r.submit(m["queries"][5:6], 5, np.array([0, 2], np.uint64), cand_tid=m["pay"][[N - 2, 3]])
            ranks, n = r.collect()
            assert n[0] == 2 and sorted(ranks["doc"][0, :2].tolist()) == [3, N - 2]
    finally:
        vb.reset_tuning()


# ---- 2. scores


def test_scores_and_topk_on_old_and_new_documents(live):
    m = live
    res = m["world"].resolver
    dt = cast(m["docs"][:120], m["pay"][:120]).bind(res)
    with dt.scorer() as early, m["fresh"].scorer() as want:  # (`early` is made before the handle grows)
        for a, b in ((120, 121), (121, 250), (250, N)):
            dt.append_documents(cast(m["docs"][a:b], m["pay"][a:b]), res)
        q_cand, cand_doc = ev.candidate_lists(len(m["queries"]), N)  # (lists of 0, 1, 63, 64, 65 and all documents: old and new mixed)
        assert (cand_doc >= 120).any() and (cand_doc < 120).any()
        for scorer in (early, dt.scorer()):
            assert np.array_equal(ev.bits(dt.evaluate(m["ids"], m["off"], q_cand, cand_doc)), ev.bits(m["fresh"].evaluate(m["ids"], m["off"], q_cand, cand_doc)))
            assert np.array_equal(ev.bits(scorer.evaluate(m["ids"], m["off"])), ev.bits(m["cross"]))
            for k in (1, 10, 1024):
                same(scorer.topk(m["ids"], m["off"], k, q_cand, cand_doc), want.topk(m["ids"], m["off"], k, q_cand, cand_doc), f"lists k={k}")
                same(scorer.topk(m["ids"], m["off"], k), want.topk(m["ids"], m["off"], k), f"cross k={k}")


# ---- 3. the directory


def tiny_docs(n, seed):
    return cm.corpus(ev.KNOWN[:40], n, seed=seed, mean=3)


def by_ctid(r, queries, q_cand, tids, k=10):
    r.submit(queries, k, q_cand, cand_tid=tids)
    return r.collect()


@pytest.mark.parametrize("n_base,n_delta,sort_max,tid_dir", [
    (1, 1, None, None), (1, 1, 0, None), (1, 63, None, None), (1, 63, 0, None), (2, 64, 0, None), (200, 65, None, 2), (200, 65, 64, 0), (5000 - 3000, 3000, None, None),
    (5000 - 3000, 3000, 0, None), (3, 2, None, 2), (3, 2, 0, 0), (4, 4093, None, None), (4, 4093, 1, 2), (1000, 64, 63, None), (1000, 64, 64, None)])
def test_sync_equals_a_fresh_directory(world, n_base, n_delta, sort_max, tid_dir):
    """handles of 1 .. 5000 documents, deltas of 1, 63, 64, 65 and 3000 rows under live_sort_max forcing each sort, tid_dir 0, 2 and the
    default, sets of 3 -> 5 and 4 -> 4097 (the stride changes across the sync).  Every ctid is asked for, with ones nobody carries."""
    n = n_base + n_delta
    docs, pay = tiny_docs(n, n), unique_payloads(n, n)
    res = world.resolver
    queries = [[ev.KNOWN[0], ev.KNOWN[3]], [ev.KNOWN[1]], [ev.KNOWN[2], ev.KNOWN[7], ev.UNKNOWN[0]]]
    rng = np.random.default_rng(n)
    lists = [rng.permutation(n), np.arange(n)[::-1], n_base + rng.integers(0, n_delta, 100)]  # (the last one: new rows only)
    q_cand, cand = lists_csr(lists)
    tids = pay[cand.astype(np.int64)].copy()
    tids[::17, 2] ^= 0x5555  # (ctids nobody carries, among the others)
    caps = dict(CAPS, max_candidates=2 * n + 100)
    try:
        if tid_dir is not None:
            vb.set_tuning("tid_dir", tid_dir)
        if sort_max is not None:
            vb.set_tuning("live_sort_max", sort_max)
        base = cast(docs[:n_base], pay[:n_base])
        dt = base.bind(res)
        with dt.reranker(res, 1, **caps, documents=base) as r:
            dt.append_documents(cast(docs[n_base:], pay[n_base:]), res)
            # not yet synced: the new rows' ctids are skipped and every pos is kept -- the rows of a reranker on the base alone
            before = by_ctid(r, queries, q_cand, tids)
            with base.bind(res).reranker(res, 1, **caps, documents=base) as old:
                same(before, by_ctid(old, queries, q_cand, tids), "before the sync")
            assert r.directory_docs == n_base and before[1][2] == 0
            made = r.allocations()
            r.sync()
            assert r.directory_docs == n and r.allocations() > made
            all_docs = cast(docs, pay)
            with all_docs.bind(res).reranker(res, 1, **caps, documents=all_docs) as want:
                expect = by_ctid(want, queries, q_cand, tids)
                same(by_ctid(r, queries, q_cand, tids), expect, f"{n_base} + {n_delta}")
                assert expect[1][2] == min(10, int((tids[int(q_cand[2]):] == pay[cand[int(q_cand[2]):].astype(np.int64)]).all(axis=1).sum())) > 0
            made = r.allocations()
            r.sync()  # (nothing new)
            assert r.allocations() == made
    finally:
        vb.reset_tuning()


def test_deltas_beyond_the_lds_sort_grow_the_scratch(world):
    """deltas of 4100 and then 9000 rows on one reranker: both past the LDS sort's 4096, the second past the scratch the first made"""
    n = 10 + 4100 + 9000
    docs, pay = tiny_docs(n, 5), unique_payloads(n, 6)
    res = world.resolver
    rng = np.random.default_rng(8)
    q_cand, cand = lists_csr([rng.permutation(n)[:3000], np.arange(n - 2000, n)])
    tids = pay[cand.astype(np.int64)]
    queries = [[ev.KNOWN[0], ev.KNOWN[3]], [ev.KNOWN[1]]]
    base = cast(docs[:10], pay[:10])
    dt = base.bind(res)
    with dt.reranker(res, 1, **CAPS, documents=base) as r:
        for a, b in ((10, 4110), (4110, n)):
            dt.append_documents(cast(docs[a:b], pay[a:b]), res)
            made = r.allocations()
            r.sync()
            assert r.directory_docs == b and r.allocations() > made
        all_docs = cast(docs, pay)
        with all_docs.bind(res).reranker(res, 1, **CAPS, documents=all_docs) as want:
            same(by_ctid(r, queries, q_cand, tids), by_ctid(want, queries, q_cand, tids), "after two large deltas")


@pytest.mark.parametrize("sort_max", [None, 0])
def test_shared_and_extreme_ctids(world, sort_max):
    """a new row with an old row's ctid (the old one wins), two new rows with one ctid (the lower index wins), (0, 0, 0) and
    (0xFFFF, 0xFFFF, 0xFFFF) arriving in a delta, ctids of rows not yet synced skipped with their pos kept and found after the sync"""
    res = world.resolver
    docs = [[(ev.KNOWN[0], 1 + i % 3), (ev.KNOWN[1 + i % 5], 1)] for i in range(12)]
    pay = unique_payloads(12, 77)
    pay[8] = pay[2]            # new row 8 shares old row 2's ctid
    pay[10] = pay[9]           # new rows 9 and 10 share one
    pay[7] = (0, 0, 0)
    pay[11] = (0xFFFF, 0xFFFF, 0xFFFF)
    ask = np.array([pay[2], pay[9], pay[7], pay[11], pay[6], pay[0], (1, 2, 3)], np.uint16)
    q_cand = np.array([0, len(ask)], np.uint64)
    query = [[ev.KNOWN[0]]]
    try:
        if sort_max is not None:
            vb.set_tuning("live_sort_max", sort_max)
        base = cast(docs[:6], pay[:6])
        dt = base.bind(res)
        with dt.reranker(res, 1, **CAPS, documents=base) as r:
            dt.append_documents(cast(docs[6:], pay[6:]), res)
            ranks, n = by_ctid(r, query, q_cand, ask)
            assert n[0] == 2 and sorted(zip(ranks["pos"][0, :2].tolist(), ranks["doc"][0, :2].tolist())) == [(0, 2), (5, 0)]
            r.sync()
            ranks, n = by_ctid(r, query, q_cand, ask)
            assert n[0] == 6 and sorted(zip(ranks["pos"][0, :6].tolist(), ranks["doc"][0, :6].tolist())) == [(0, 2), (1, 9), (2, 7), (3, 11), (4, 6), (5, 0)]
            all_docs = cast(docs, pay)
            with all_docs.bind(res).reranker(res, 1, **CAPS, documents=all_docs) as want:
                same((ranks, n), by_ctid(want, query, q_cand, ask), "shared ctids")
    finally:
        vb.reset_tuning()


# ---- 4. the snapshot rule


def test_a_batch_submitted_before_the_sync_keeps_the_old_directory(live):
    m = live
    res = m["world"].resolver
    base = cast(m["docs"][:150], m["pay"][:150])
    dt = base.bind(res)
    q_cand, cand = lists_csr([np.arange(N), np.arange(N)[::-1], np.arange(100, 200)])
    tids = m["pay"][cand.astype(np.int64)]
    queries = m["queries"][5:8]
    with dt.reranker(res, 3, **CAPS, documents=base) as r, base.bind(res).reranker(res, 1, **CAPS, documents=base) as old, \
            m["fresh"].reranker(res, 1, **CAPS, documents=m["all"]) as new:
        r.submit(queries, 10, q_cand, cand_tid=tids)                      # A
        dt.append_documents(cast(m["docs"][150:], m["pay"][150:]), res)
        r.sync()
        r.submit(queries, 10, q_cand, cand_tid=tids)                      # B
        assert r.in_flight() == 2
        same(r.collect(), by_ctid(old, queries, q_cand, tids), "A: the directory of before the append")
        same(r.collect(), by_ctid(new, queries, q_cand, tids), "B: the directory of after the sync")
        # 20 rounds after the sync allocate nothing; neither does a sync the room to spare covers
        made, held = r.allocations(), r.device_bytes()
        want = by_ctid(new, queries, q_cand, tids)
        for _ in range(20):
            same(by_ctid(r, queries, q_cand, tids), want, "after the sync")
        assert (r.allocations(), r.device_bytes()) == (made, held)


def test_a_sync_inside_the_room_to_spare_allocates_nothing(live):
    m = live
    res = m["world"].resolver
    base = cast(m["docs"][:100], m["pay"][:100])
    dt = base.bind(res)
    with dt.reranker(res, 1, **CAPS, documents=base) as r:
        dt.append_documents(cast(m["docs"][100:110], m["pay"][100:110]), res)
        r.sync()  # (grows: 100 -> 200 entries)
        made, held = r.allocations(), r.device_bytes()
        try:
            for a, b in ((110, 111), (111, 180), (180, 200)):
                if a == 180:
                    vb.set_tuning("live_sort_max", 0)  # (the first delta of this reranker through the radix sort: its scratch is there already)
                dt.append_documents(cast(m["docs"][a:b], m["pay"][a:b]), res)
                r.sync()
                assert (r.allocations(), r.device_bytes(), r.directory_docs) == (made, held, b)
        finally:
            vb.reset_tuning()
        dt.append_documents(cast(m["docs"][200:201], m["pay"][200:201]), res)
        r.sync()
        assert r.allocations() > made and r.directory_docs == 201


# ---- 5. refusals


def refused(code, text, call, *args):
    with pytest.raises(vb.Vbm25Error) as e:
        call(*args)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_refusals_leave_everything_as_it_was(live, sealed_worlds):
    m = live
    res = m["world"].resolver
    L = vb.lib()
    base = cast(m["docs"][:50], m["pay"][:50])
    dt = base.bind(res)
    delta, bare = cast(m["docs"][50:60], m["pay"][50:60]), cast(m["docs"][50:60], None)
    q_cand, tids = np.array([0, 50], np.uint64), m["pay"][:50]
    with dt.reranker(res, 1, **CAPS, documents=base) as r, dt.reranker(res, 1, **CAPS) as no_ctids:
        rows = by_ctid(r, m["queries"][5:6], q_cand, tids)

        def unchanged(n=50):
            assert_prefix(dt, m, n, "after a refusal")
            same(by_ctid(r, m["queries"][5:6], q_cand, tids), rows, "after a refusal")

        for args in ((None, delta.h, res.h), (dt.h, None, res.h), (dt.h, delta.h, None)):
            assert L.vbm25_doc_terms_append_documents(*args) == INVALID and L.vbm25_last_error() == b"NULL argument"
            assert L.vbm25_doc_terms_append(*args) == INVALID and L.vbm25_last_error() == b"NULL argument"
        assert L.vbm25_reranker_sync(None) == INVALID and L.vbm25_last_error() == b"NULL argument"
        assert L.vbm25_doc_terms_base_docs(None) == 0 and L.vbm25_reranker_directory_docs(None) == 0
        other = sealed_worlds(63)
        refused(INVALID, "the documents are bound to another index than the resolver's", dt.append_documents, delta, other["resolver"])
        unchanged()
        # a caster slot submitted again since its collect
        with vb.Caster(0, 1, 16, 256, 1 << 12, seed=cm.SEED) as caster:
            caster.submit(m["docs"][50:52], m["pay"][50:52])
            stale = caster.collect()
            caster.submit(m["docs"][52:54], m["pay"][52:54])
            refused(INVALID, "the delta belongs to a caster slot that was submitted again", dt.append_documents, stale, res)
            unchanged()
            caster.collect()
        # the CSR's validation is upload's
        dl = delta.download()
        bad = dl["g_key"].reshape(-1, 16).copy()
        s = dl["g_start"].astype(np.int64)
        d = int(np.flatnonzero(np.diff(s) >= 2)[0])
        bad[[s[d], s[d] + 1]] = bad[[s[d] + 1, s[d]]]
        refused(INVALID, f"growing document {d}: keys must be strictly ascending", dt.append, dl["g_start"], bad, dl["g_tf"], dl["g_fieldnorm"],
                dl["g_payload"], res)
        wrong = dl["g_start"].copy()
        wrong[3] = wrong[4] + 1
        refused(INVALID, "start not monotone at document 3", dt.append, wrong, dl["g_key"], dl["g_tf"], dl["g_fieldnorm"], dl["g_payload"], res)
        unchanged()
        # an empty delta
        dt.append_documents(cast([], np.zeros((0, 3), np.uint16)), res)
        unchanged()
        # sync
        refused(INVALID, "sync on a reranker created without payloads", no_ctids.sync)
        # the first append decides about payloads
        dt.append_documents(delta, res)
        refused(INVALID, "the delta carries no payloads and the documents appended so far carry them", dt.append_documents, bare, res)
        assert_prefix(dt, m, 60, "after the payload refusal")
    plain = base.bind(res)
    with plain.reranker(res, 1, **CAPS, documents=base) as r:
        rows = by_ctid(r, m["queries"][5:6], q_cand, tids)
        plain.append_documents(bare, res)  # (a documents-bound handle may grow without payloads ...)
        refused(INVALID, "the delta carries payloads and the documents appended so far carry none", plain.append_documents, delta, res)
        refused(INVALID, "the 10 documents appended to the bound documents carry no payloads", r.sync)  # (... but no ctid names them)
        assert r.directory_docs == 50
        same(by_ctid(r, m["queries"][5:6], q_cand, tids), rows, "after the refused sync")
        refused(INVALID, "the 10 documents appended to the bound documents carry no payloads", plain.reranker, res, 1, *CAPS.values(), base)
        assert_prefix(plain, m, 60, "grown without payloads")
    # an index-bound handle needs the ctids
    w = sealed_worlds(63)
    bound = w["gix"].bind()
    refused(INVALID, "the delta carries no payloads: documents appended to an index-bound handle need their ctids", bound.append_documents,
            cast(m["docs"][63:70], None), w["resolver"])
    assert_prefix(bound, w, 63, "after the refusal", index_bound=True)


def test_create_on_a_grown_handle_equals_create_then_sync(live, sealed_worlds):
    w = sealed_worlds(65)
    res = w["resolver"]
    dt = w["gix"].bind()
    q_cand, cand = lists_csr([np.arange(N)[::-1], np.arange(0, N, 3)])
    tids = w["pay"][cand.astype(np.int64)]
    with dt.reranker(res, 1, **CAPS, from_index=True) as early:
        dt.append_documents(cast(w["docs"][65:], w["pay"][65:]), res)
        early.sync()
        with dt.reranker(res, 1, **CAPS, from_index=True) as late:
            assert late.directory_docs == early.directory_docs == N
            got = by_ctid(late, w["queries"][5:7], q_cand, tids)
            same(got, by_ctid(early, w["queries"][5:7], q_cand, tids), "create_from_index on the grown handle")
            with w["fresh"].reranker(res, 1, **CAPS, documents=w["all"]) as want:
                same(got, by_ctid(want, w["queries"][5:7], q_cand, tids), "the fresh handle")
            assert (got[0]["doc"][0, :got[1][0]] >= 65).any()
        refused(INVALID, "the documents given for the ctid lookup are 300, the bound documents 65", dt.reranker, res, 1, *CAPS.values(), w["all"])


# ---- 6. the live table, end to end


def test_growing_hits_are_reranked_on_the_index_bound_handle(live, sealed_worlds):
    """a growing segment and an index-bound handle fed the same three deltas: a growing hit's doc_id 0xFFFFFFFF - g is document
    n_sealed + g of the handle, and its rerank score is vb.evaluate on the downloaded documents"""
    n_sealed = 64
    w = sealed_worlds(n_sealed)
    res, gix = w["resolver"], w["gix"]
    dt = gix.bind()
    first = cast(w["docs"][64:65], w["pay"][64:65])
    gs = vb.GrowingSegment.from_dict(gix, first.download())
    dt.append_documents(first, res)
    for a, b in ((65, 150), (150, N)):
        delta = cast(w["docs"][a:b], w["pay"][a:b])
        gs.append_documents(delta)
        dt.append_documents(delta, res)
    queries = w["queries"][5:13]
    res.submit(queries)
    ids, off = res.collect()
    hits, n_hits = vb.search_batch_growing(gix, gs, ids, off, 20)
    lists, pairs = [], []
    for q in range(len(queries)):
        ids_q = hits["doc_id"][q, :n_hits[q]].astype(np.int64)
        growing = ids_q >= n_sealed + (1 << 31)  # (sealed ids are small, growing ones count down from 0xFFFFFFFF)
        docs_q = np.where(growing, n_sealed + (0xFFFFFFFF - ids_q), ids_q)
        assert (docs_q < N).all()
        lists.append(docs_q)
        pairs += [(q, int(d)) for d in docs_q]
    assert any((l >= n_sealed).any() for l in lists) and any((l < n_sealed).any() for l in lists)
    q_cand, cand_doc = lists_csr(lists)
    with dt.reranker(res, 1, **CAPS, from_index=True) as r:
        r.submit(queries, 20, q_cand, cand_doc=cand_doc)
        ranks, n = r.collect()
    # vb.evaluate's statistics are the sealed segment's: the host copy of the index's segment
    w2 = ev.World.__new__(ev.World)
    w2.seg = cm.build_segment(cm.cast(w["docs"][:n_sealed], w["pay"][:n_sealed]), 1.2, 0.75)
    w2.vocab = [bytes(k) for k in w2.seg.arrays()["term_key"].reshape(-1, 16)]
    want = w2.reference(w["all"].download(), ids, off, pairs)
    at = 0
    for q in range(len(queries)):
        assert n[q] == len(lists[q])
        got = np.zeros(len(lists[q]))
        got[ranks["pos"][q, :n[q]]] = ranks["score"][q, :n[q]]
        assert np.array_equal(ev.bits(got), ev.bits(want[at:at + len(lists[q])])), f"query {q}"
        assert np.array_equal(ranks["doc"][q, :n[q]], lists[q][ranks["pos"][q, :n[q]]])
        at += len(lists[q])
