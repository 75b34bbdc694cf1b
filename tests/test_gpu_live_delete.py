"""Deletes on a bound handle, on the GPU (csrc/live.hip, csrc/rerank.hip, csrc/reranker.hip): DocTerms.delete / delete_tids against
numpy -- the bitmap's words, np.isin on packed keys -- and what a dead document does to Scorer.topk and to a Reranker, against a model
made of code the deletes do not touch: a top-k is a stable descending sort of DocTerms.evaluate's scores over the candidates numpy
leaves eligible, cut at k, with pos kept; a ctid's document is the lowest live index numpy finds for that payload.  The snapshot rule,
appends after deletes, what the calls allocate, the calls that stay as they are, every refusal with code and message.  -m gpu only."""
import numpy as np
import pytest

import cast_model as cm
import test_gpu_evaluate_documents as ev
import vectorchord_bm25_amd as vb
from test_gpu_live_rerank import CAPS, N, cast, corpus, refused, tiny_docs, unique_payloads
from test_gpu_reranker import same

pytestmark = pytest.mark.gpu
INVALID = -1
NO = -1  # the model's "no document"


def words_of(mask):
    """the filters' packing: document d at bit d & 63 of word d >> 6"""
    padded = np.zeros((len(mask) + 63) // 64 * 64, bool)
    padded[:len(mask)] = mask
    return np.packbits(padded, bitorder="little").view(np.uint64)


def model_rows(cross, lists, dead, k):
    """per query: the eligible entries (a document, and a live one) by descending score, stable, cut at k; pos is the list index"""
    ranks, n = np.zeros((len(lists), k), vb.RANK_DTYPE), np.zeros(len(lists), np.uint32)
    for q, docs in enumerate(lists):
        docs = np.asarray(docs, np.int64)
        ok = docs >= 0
        ok[ok] &= ~dead[docs[ok]]
        pos = np.flatnonzero(ok)
        s = cross[q, docs[pos]]
        order = np.argsort(-s, kind="stable")[:k]
        ranks["score"][q, :len(order)], ranks["pos"][q, :len(order)], ranks["doc"][q, :len(order)] = s[order], pos[order], docs[pos[order]]
        n[q] = len(order)
    return ranks, n


def ctid_docs(pay, n_dir, tids, dead):
    """the lowest live document among the first n_dir that carries each ctid, NO without one"""
    keys, out = vb.TidSet.keys(pay[:n_dir]), []
    for key in vb.TidSet.keys(tids):
        at = np.flatnonzero(keys == key)
        at = at[~dead[at]]
        out.append(int(at[0]) if len(at) else NO)
    return np.array(out, np.int64)


def csr(lists):
    q_cand = np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.uint64)
    return q_cand, (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(np.uint32)


@pytest.fixture(scope="module")
def world():
    return ev.World(ev.KNOWN)


@pytest.fixture(scope="module")
def live(world):
    """300 documents with distinct ctids, their queries, and the cross product's scores from DocTerms.evaluate (computed once)"""
    docs, pay = corpus(), unique_payloads(N, 1)
    all_docs = cast(docs, pay)
    fresh = all_docs.bind(world.resolver)
    queries = ev.query_batch()[:16]
    ids, off = world.resolve(queries)
    cross = fresh.evaluate(ids, off)
    cross.setflags(write=False)
    assert cross.any()
    return dict(world=world, docs=docs, pay=pay, all=all_docs, queries=queries, ids=ids, off=off, cross=cross)


def sub_queries(m, lo, hi):
    """queries lo .. hi of the batch: (lexemes, ids, off, their rows of the cross product)"""
    off = m["off"].astype(np.int64)
    return m["queries"][lo:hi], m["ids"][off[lo]:off[hi]], (off[lo:hi + 1] - off[lo]).astype(np.uint32), m["cross"][lo:hi]


# ---- 1. the bitmap's words


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 300])
def test_delete_writes_the_words_numpy_packs(live, n):
    m = live
    dt = cast(m["docs"][:n], m["pay"][:n]).bind(m["world"].resolver)
    held = dt.device_bytes()
    dead = np.zeros(n, bool)
    assert dt.dead_docs == 0 and not dt.read_dead().any() and len(dt.read_dead()) == (n + 63) // 64
    patterns = [[], [0], [n - 1], [d for d in (63, 64) if d < n], list(range(0, n, 2)), [0, 0, n - 1, n // 2, n // 2, 0], list(range(n)) + [0]]
    for p in patterns:
        fresh = np.zeros(n, bool)
        fresh[p] = True
        want_new = int((fresh & ~dead).sum())
        assert dt.delete(np.array(p, np.uint32)) == want_new, p
        dead |= fresh
        assert np.array_equal(dt.read_dead(), words_of(dead)) and dt.dead_docs == int(dead.sum()), p
        assert dt.delete(p) == 0 and np.array_equal(dt.read_dead(), words_of(dead)) and dt.dead_docs == int(dead.sum()), f"{p} again"
        if not dead.any():
            assert dt.device_bytes() == held  # (a delete of nothing allocates nothing)
    assert dead.all() and dt.device_bytes() == held + 8 * ((n + 63) // 64)
    if n % 64:
        assert int(dt.read_dead()[-1]) >> (n % 64) == 0  # (nothing beyond n_docs)


# ---- 2. delete_tids against np.isin on packed keys

M = 500
_sealed = {}


def tid_corpus():
    if "docs" not in _sealed:
        _sealed["docs"] = tiny_docs(M, 31)
    return _sealed["docs"]


def tid_payloads(base, tail):
    """distinct ctids, but: (0, 0, 0) and (0xFFFF, 0xFFFF, 0xFFFF) are among them, the last sealed document shares the first one's, and
    so does the last appended one.  The first `base` ctids depend on `base` alone: the index over them is built once."""
    n = base + tail
    pay = unique_payloads(M, 9)[:n].copy()
    if n > 3:
        pay[1], pay[2] = (0, 0, 0), (0xFFFF, 0xFFFF, 0xFFFF)
    if base > 3:
        pay[base - 1] = pay[0]
    if tail and n > 1:
        pay[n - 1] = pay[0]
    return pay


def sealed_index(base, pay):
    if base not in _sealed:
        gix = vb.GpuIndex(vb.DeviceSegment.from_documents(cast(tid_corpus()[:base], pay[:base]), 1.2, 0.75))
        _sealed[base] = gix, vb.Resolver(gix, 1, 64, 4096, 1 << 18, seed=cm.SEED)
    return _sealed[base]


def grown_handle(world, base, tail, index_bound, pay):
    """-> (the handle of base + tail documents, the Documents delete_tids takes for it)"""
    docs = tid_corpus()
    if index_bound:
        gix, res = sealed_index(base, pay)
        dt, payloads = gix.bind(), None
    else:
        res = world.resolver
        first = cast(docs[:base], pay[:base])
        dt, payloads = first.bind(res), first if base else None
    if tail:
        dt.append_documents(cast(docs[base:base + tail], pay[base:base + tail]), res)
    assert (dt.base_docs, dt.n_docs) == (base, base + tail)
    return dt, payloads


@pytest.mark.parametrize("tail", [0, 1, 58, 59, 200])
@pytest.mark.parametrize("base", [0, 1, 59, 64, 70, 300])
def test_delete_tids_equals_isin_on_the_packed_keys(world, base, tail):
    n = base + tail
    pay = tid_payloads(base, tail)
    keys = vb.TidSet.keys(pay)
    absent = unique_payloads(M, 10)[:40] ^ np.uint16(0x8001)
    absent = absent[~np.isin(vb.TidSet.keys(absent), keys)]
    rng = np.random.default_rng(n)
    sets = [np.zeros((0, 3), np.uint16), absent, pay[n // 2:n // 2 + 1], pay[:1], np.array([(0, 0, 0), (0xFFFF, 0xFFFF, 0xFFFF)], np.uint16),
            np.concatenate([pay[rng.random(n) < 0.3], absent[:5]]), pay, pay]
    try:
        for index_bound in (False, True):
            if index_bound and not base:
                continue
            for grid, tid_dir in ((1, 0), (3, 2), (1, None), (3, None)):
                vb.reset_tuning()
                vb.set_tuning("tid_grid", grid)
                if tid_dir is not None:
                    vb.set_tuning("tid_dir", tid_dir)
                dt, payloads = grown_handle(world, base, tail, index_bound, pay)
                held, dead = dt.device_bytes(), np.zeros(n, bool)
                for i, tids in enumerate(sets):
                    what = f"base {base} tail {tail} index_bound {index_bound} grid {grid} dir {tid_dir} set {i}"
                    with vb.TidSet(tids) as s:
                        hit = np.isin(keys, vb.TidSet.keys(tids)) if len(tids) else np.zeros(n, bool)
                        assert dt.delete_tids(s, payloads) == int((hit & ~dead).sum()), what
                    if i == 3 and n > 1 and (tail or base > 3):
                        assert hit.sum() >= 2 and hit[0] and hit[n - 1 if tail else base - 1]  # (one ctid, several documents: all die)
                    dead |= hit
                    assert np.array_equal(dt.read_dead(), words_of(dead)) and dt.dead_docs == int(dead.sum()), what
                    if not dead.any():
                        assert dt.device_bytes() == held, what  # (an empty set, a set that matches nothing: no bitmap)
                assert dead.all()
    finally:
        vb.reset_tuning()


# ---- 3. the top-k


def dead_lists(m, dead, k):
    """candidate lists around the dead documents `dead` (a mask over the N documents), for six queries"""
    rng = np.random.default_rng(k)
    d, l = np.flatnonzero(dead), np.flatnonzero(~dead)
    mixed = rng.permutation(N)
    return [np.r_[d[:5], l[:40]],                      # dead documents first
            np.r_[l[:40], d[:5]],                      # ... last
            mixed,                                     # ... interleaved
            d[:1],                                     # ... alone
            np.r_[d[0], l[3], d[0], l[3], l[3], d[1], d[0]],  # ... repeated, among repeated live ones
            d[rng.integers(0, len(d), 70)],            # every candidate dead
            rng.integers(0, N, 2 * k + 1)]             # 2 k + 1 entries, repeats among them


@pytest.mark.parametrize("part,grid", [(None, None), (64, 1), (64, 3)])
def test_topk_leaves_dead_documents_out(live, part, grid):
    """Scorer.topk and the ring (submit, submit_ids; cand_doc lists, ctid lists, the cross product) byte for byte against the model, at
    k 1, 10 and 1024; with rerank_part 64 the dead entries fall into several parts and the merge kernel runs"""
    m = live
    res = m["world"].resolver
    queries, ids, off, cross = sub_queries(m, 5, 12)
    dead = np.zeros(N, bool)
    dead[[0, 1, 63, 64, 65, 128, N - 1]] = True
    dead[np.random.default_rng(3).random(N) < 0.25] = True
    try:
        if part:
            vb.set_tuning("rerank_part", part)
            vb.set_tuning("eval_grid", grid)
        dt = m["all"].bind(res)
        with dt.scorer() as early, dt.reranker(res, 2, **CAPS, documents=m["all"]) as r:
            none = np.zeros(N, bool)
            lists = dead_lists(m, dead, 10)
            q_cand, cand = csr(lists)
            same(early.topk(ids, off, 10, q_cand, cand), model_rows(cross, lists, none, 10), "before the delete")
            made = r.allocations()
            assert dt.delete(np.flatnonzero(dead)) == int(dead.sum())
            for k in (1, 10, 1024):
                lists = dead_lists(m, dead, k)
                q_cand, cand = csr(lists)
                want = model_rows(cross, lists, dead, k)
                assert want[1][5] == 0 and not want[0][5].view(np.uint8).any()  # (every candidate dead: no rank, an all-zero row)
                assert want[1][3] == 0 and want[1][4] == min(k, 3)
                with dt.scorer() as late:
                    for name, sc in (("a scorer made before the delete", early), ("a scorer made after it", late)):
                        same(sc.topk(ids, off, k, q_cand, cand), want, f"{name}, k={k}")
                        same(sc.topk(ids, off, k), model_rows(cross, [np.arange(N)] * len(lists), dead, k), f"{name}, the cross product, k={k}")
                r.submit(queries, k, q_cand, cand_doc=cand)
                r.submit_ids(ids, off, k, q_cand, cand_doc=cand)
                same(r.collect(), want, f"submit, k={k}")
                same(r.collect(), want, f"submit_ids, k={k}")
                r.submit(queries, k, q_cand, cand_tid=m["pay"][cand.astype(np.int64)])  # (distinct ctids: a dead row's ctid names nobody)
                r.submit_ids(ids, off, k)
                same(r.collect(), want, f"ctid lists, k={k}")
                same(r.collect(), model_rows(cross, [np.arange(N)] * len(lists), dead, k), f"the ring's cross product, k={k}")
            assert r.allocations() == made
    finally:
        vb.reset_tuning()


def test_a_tie_across_the_kth_place_with_a_tied_document_dead(live):
    m = live
    res = m["world"].resolver
    queries, ids, off, cross = sub_queries(m, 5, 12)
    lists, ks, kill = [], [], []
    for q in range(len(queries)):
        vals, counts = np.unique(cross[q], return_counts=True)
        tie = vals[counts >= 3].max()
        tied = np.flatnonzero(cross[q] == tie)[:4]
        above = np.flatnonzero(cross[q] > tie)[:20]
        lists.append(np.r_[tied[:2], above, tied[2:]])
        ks.append(len(above) + 2)  # (with everyone live the k-th place is the second tied entry; the first one dies)
        kill.append(int(tied[0]))
    q_cand, cand = csr(lists)
    dt = m["all"].bind(res)
    dead = np.zeros(N, bool)
    dead[kill] = True
    dt.delete(kill)
    with dt.scorer() as sc, dt.reranker(res, 1, **CAPS) as r:
        for k in sorted(set(ks)):
            want = model_rows(cross, lists, dead, k)
            same(sc.topk(ids, off, k, q_cand, cand), want, f"k={k}")
            r.submit(queries, k, q_cand, cand_doc=cand)
            same(r.collect(), want, f"the ring, k={k}")
        for q, k in enumerate(ks):
            got = sc.topk(ids, off, k, q_cand, cand)
            row = got[0][q, :got[1][q]]
            assert kill[q] not in row["doc"] and got[1][q] == min(k, int((~dead[lists[q]]).sum()))
            if not dead[lists[q][1]]:  # (the second tied entry keeps its place in front of the tied ones behind it)
                assert lists[q][1] in row["doc"]


# ---- 4. the ctid lookup


@pytest.mark.parametrize("tid_dir", [0, 2, None])
def test_a_ctid_names_its_lowest_live_document(world, tid_dir):
    """two documents with one ctid, the lower dead; both dead; three with one ctid and only the middle one live; and the reuse: a
    sealed row deleted, its ctid appended again -- no row until the sync, the new row after it"""
    res = world.resolver
    n0 = 40
    docs = [[(ev.KNOWN[0], 1 + i % 3), (ev.KNOWN[1 + i % 5], 1)] for i in range(n0 + 2)]
    pay = unique_payloads(n0 + 2, 21)
    pay[7] = pay[3]                      # 3 and 7 share
    pay[12] = pay[10]                    # 10 and 12 share
    pay[30] = pay[25] = pay[20]          # 20, 25 and 30 share
    pay[n0] = pay[5]                     # the rows appended later reuse the ctids of 5 and of 3 / 7
    pay[n0 + 1] = pay[3]
    ask = np.array([pay[3], pay[10], pay[20], pay[5], pay[0], (1, 2, 3), pay[3]], np.uint16)
    q_cand = np.array([0, len(ask)], np.uint64)
    query, ids, off = [[ev.KNOWN[0]]], *world.resolve([[ev.KNOWN[0]]])
    try:
        if tid_dir is not None:
            vb.set_tuning("tid_dir", tid_dir)
        base = cast(docs[:n0], pay[:n0])
        dt = base.bind(res)
        cross = cast(docs, pay).bind(res).evaluate(ids, off)
        with dt.reranker(res, 1, **CAPS, documents=base) as r:
            dead = np.zeros(n0 + 2, bool)

            def check(n_dir, what):
                r.submit(query, 10, q_cand, cand_tid=ask)
                got = r.collect()
                same(got, model_rows(cross, [ctid_docs(pay, n_dir, ask, dead)], dead, 10), what)
                return dict(zip(got[0]["pos"][0, :got[1][0]].tolist(), got[0]["doc"][0, :got[1][0]].tolist()))

            assert check(n0, "nobody dead") == {0: 3, 1: 10, 2: 20, 3: 5, 4: 0, 6: 3}
            for kill in ([3], [10, 12], [20, 30], [5]):
                dt.delete(kill)
                dead[kill] = True
            # the lower of two dead: the upper; both dead: no row, pos kept; of three the middle one; the deleted sealed row 5: no row
            assert check(n0, "after the deletes") == {0: 7, 2: 25, 4: 0, 6: 7}
            dt.delete([7])
            dead[7] = True
            assert check(n0, "3 and 7 dead") == {2: 25, 4: 0}
            made = r.allocations()
            dt.append_documents(cast(docs[n0:], pay[n0:]), res)
            assert check(n0, "the ctids inserted again, not yet synced") == {2: 25, 4: 0}
            r.sync()
            assert check(n0 + 2, "synced: the ctids name the new rows") == {0: n0 + 1, 2: 25, 3: n0, 4: 0, 6: n0 + 1}
            assert r.allocations() > made  # (the sync grew; the deletes moved nothing: see test_what_the_deletes_allocate)
    finally:
        vb.reset_tuning()


# ---- 5. the snapshot rule


def test_a_batch_submitted_before_the_delete_keeps_the_old_bits(live):
    m = live
    res = m["world"].resolver
    queries, ids, off, cross = sub_queries(m, 5, 8)
    lists = [np.arange(N), np.arange(N)[::-1], np.arange(100, 200)]
    q_cand, cand = csr(lists)
    tids = m["pay"][cand.astype(np.int64)]
    dt = m["all"].bind(res)
    first, second = np.zeros(N, bool), np.zeros(N, bool)
    first[::3] = True
    second[::3] = second[1::2] = True
    with dt.reranker(res, 3, **CAPS, documents=m["all"]) as r:
        r.submit(queries, 10, q_cand, cand_tid=tids)            # A: nobody dead, no bitmap yet
        dt.delete(np.flatnonzero(first))
        r.submit(queries, 10, q_cand, cand_doc=cand)            # B
        r.submit(queries, 10, q_cand, cand_tid=tids)            # C
        assert r.in_flight() == 3
        same(r.collect(), model_rows(cross, lists, np.zeros(N, bool), 10), "A: the rows of before the delete")
        r.submit_ids(ids, off, 10, q_cand, cand_doc=cand)       # D: enqueued before the second delete, collected after it
        dt.delete(np.flatnonzero(second))
        same(r.collect(), model_rows(cross, lists, first, 10), "B")
        same(r.collect(), model_rows(cross, lists, first, 10), "C")
        r.submit(queries, 10, q_cand, cand_tid=tids)            # E
        same(r.collect(), model_rows(cross, lists, first, 10), "D: the bits of before the second delete")
        same(r.collect(), model_rows(cross, lists, second, 10), "E: the next batch sees the new bits")


# ---- 6. appends after deletes


def test_appends_carry_the_bitmap_along(live):
    """200 single-document appends behind a base of 20, a delete after every tenth: the fieldnorm array doubles 20 -> 40 -> ... -> 320
    with the bitmap behind it; old bits are kept, new documents are live, rows are exact after each step"""
    m = live
    res = m["world"].resolver
    queries, ids, off, cross = sub_queries(m, 5, 9)
    n = 20
    base = cast(m["docs"][:n], m["pay"][:n])
    dt = base.bind(res)
    dead = np.zeros(N, bool)
    rng = np.random.default_rng(4)
    with dt.scorer() as sc, dt.reranker(res, 1, **CAPS, documents=base) as r:
        for step in range(200):
            dt.append_documents(cast(m["docs"][n:n + 1], m["pay"][n:n + 1]), res)
            n += 1
            if step % 10 == 9:  # (the first one at 30 documents: the bitmap is there when the capacity of 40 is outgrown, then 80, 160)
                kill = np.r_[n - 1, step % 20, rng.integers(0, n, 2)]  # (the newest document, one of the base, two others; dead or not)
                assert dt.delete(kill) == int((~dead[np.unique(kill)]).sum())
                dead[kill] = True
            assert np.array_equal(dt.read_dead(), words_of(dead[:n])) and dt.dead_docs == int(dead.sum()), step
            same(sc.topk(ids, off, 10), model_rows(cross[:, :n], [np.arange(n)] * len(queries), dead, 10), f"after append {step}")
        assert n == 220 and dead[:20].any() and dead[160:].any()
        r.sync()
        ask = np.arange(n)[::-1]
        r.submit(queries[:1], 1024, np.array([0, n], np.uint64), cand_tid=m["pay"][ask])
        same(r.collect(), model_rows(cross[:1, :n], [ctid_docs(m["pay"], n, m["pay"][ask], dead)], dead, 1024), "by ctid at the end")


# ---- 7. what the calls allocate, and what stays as it is


def test_what_the_deletes_allocate(live):
    m = live
    res = m["world"].resolver
    queries, ids, off, cross = sub_queries(m, 5, 8)
    dt = m["all"].bind(res)
    held = dt.device_bytes()
    with dt.reranker(res, 1, **CAPS, documents=m["all"]) as r, dt.scorer() as sc:
        made, r_held = r.allocations(), r.device_bytes()
        # deletes of nothing: no bitmap
        assert dt.delete([]) == 0
        with vb.TidSet(np.zeros((0, 3), np.uint16)) as empty, vb.TidSet(m["pay"] ^ np.uint16(0x4001)) as nobody:
            assert not np.isin(vb.TidSet.keys(m["pay"] ^ np.uint16(0x4001)), vb.TidSet.keys(m["pay"])).any()
            assert dt.delete_tids(empty, m["all"]) == 0 and dt.delete_tids(nobody, m["all"]) == 0
        assert dt.device_bytes() == held and dt.dead_docs == 0 and not dt.read_dead().any()
        # the first delete that names a document makes it: one bit a document of the fieldnorm array's capacity
        assert dt.delete([5]) == 1
        assert dt.device_bytes() == held + 8 * ((N + 63) // 64)
        with vb.TidSet(m["pay"][10:20]) as s:
            assert dt.delete_tids(s, m["all"]) == 10
        assert dt.device_bytes() == held + 8 * ((N + 63) // 64)
        dead = np.zeros(N, bool)
        dead[[5] + list(range(10, 20))] = True
        want = model_rows(cross, [np.arange(N)] * 3, dead, 10)
        same(sc.topk(ids, off, 10), want, "first")
        sc_held = sc.device_bytes()
        assert dt.delete([5, 11]) == 0
        same(sc.topk(ids, off, 10), want, "after the repeat")
        assert sc.device_bytes() == sc_held
        r.submit(queries, 10)
        same(r.collect(), want, "the ring")
        assert (r.allocations(), r.device_bytes()) == (made, r_held)


def test_evaluate_and_download_do_not_see_the_deletes(live):
    m = live
    res = m["world"].resolver
    dt = m["all"].bind(res)
    q_cand, cand = ev.candidate_lists(len(m["queries"]), N)
    with dt.scorer() as sc:
        before = (dt.evaluate(m["ids"], m["off"]), dt.evaluate(m["ids"], m["off"], q_cand, cand), sc.evaluate(m["ids"], m["off"]),
                  sc.evaluate(m["ids"], m["off"], q_cand, cand), *dt.download())
        assert dt.delete(np.arange(0, N, 2)) == N // 2
        after = (dt.evaluate(m["ids"], m["off"]), dt.evaluate(m["ids"], m["off"], q_cand, cand), sc.evaluate(m["ids"], m["off"]),
                 sc.evaluate(m["ids"], m["off"], q_cand, cand), *dt.download())
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert np.array_equal(ev.bits(before[0]), ev.bits(m["cross"]))


# ---- 8. refusals


def test_refusals_leave_the_words_and_the_count(live):
    m = live
    res = m["world"].resolver
    L = vb.lib()
    base = cast(m["docs"][:50], m["pay"][:50])
    dt = base.bind(res)
    dt.delete([1, 49])
    words = dt.read_dead()

    def unchanged(h=dt, w=words, count=2):
        assert np.array_equal(h.read_dead(), w) and h.dead_docs == count

    import ctypes as C
    one = np.array([3], np.uint32)
    with vb.TidSet(m["pay"][:5]) as s:
        n_new = C.c_uint32(77)
        assert L.vbm25_doc_terms_delete(None, one.ctypes.data, 1, C.byref(n_new)) == INVALID and L.vbm25_last_error() == b"NULL argument"
        assert L.vbm25_doc_terms_delete(dt.h, None, 1, C.byref(n_new)) == INVALID and L.vbm25_last_error() == b"NULL argument"
        assert L.vbm25_doc_terms_delete_tids(None, s.h, base.h, C.byref(n_new)) == INVALID and L.vbm25_last_error() == b"NULL argument"
        assert L.vbm25_doc_terms_delete_tids(dt.h, None, base.h, C.byref(n_new)) == INVALID and L.vbm25_last_error() == b"NULL argument"
        assert L.vbm25_doc_terms_read_dead(dt.h, None) == INVALID and L.vbm25_last_error() == b"NULL argument"
        assert n_new.value == 77 and L.vbm25_doc_terms_dead_docs(None) == 0
        unchanged()
        refused(INVALID, "docs[2] is 50: outside the handle's 50 documents", dt.delete, [3, 4, 50, 5])
        unchanged()
        refused(INVALID, "payloads is NULL: the 50 documents the handle was bound with", dt.delete_tids, s)
        refused(INVALID, "the documents given for the ctid lookup are 300, the bound documents 50", dt.delete_tids, s, m["all"])
        refused(INVALID, "the documents given for the ctid lookup carry no payloads", dt.delete_tids, s, cast(m["docs"][:50], None))
        unchanged()
        # appended documents without payloads: no ctid names them
        dt.append_documents(cast(m["docs"][50:60], None), res)
        refused(INVALID, "the 10 documents appended to the bound documents carry no payloads", dt.delete_tids, s, base)
        unchanged()  # (60 documents are still one word)
        assert dt.delete([55]) == 1  # (by index such a document dies like any other)
        # an index-bound handle takes no payloads: its ctids are the index's
        gix = vb.GpuIndex(vb.DeviceSegment.from_documents(base, 1.2, 0.75))
        bound = gix.bind()
        refused(INVALID, "payloads are given and the handle is bound to an index", bound.delete_tids, s, base)
        assert bound.dead_docs == 0 and not bound.read_dead().any()
        assert bound.delete_tids(s) == 5 and bound.dead_docs == 5 and np.array_equal(bound.read_dead(), words_of(np.arange(50) < 5))
