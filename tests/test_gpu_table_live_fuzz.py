"""tests/test_gpu_table_ctid_fuzz.py's life on the live rerank stack (csrc/live.hip, the sync in csrc/reranker.hip): ONE index-bound
handle and ONE reranker ring on it for a whole epoch, where CtidLife binds the epoch's documents again after every insert.  LiveLife
keeps everything CtidLife asserts and adds, per epoch:
  attach   a second GpuIndex.bind() (`live`), a depth-3 ring on it (from_index) and a scorer, all made before the handle grows;
  INSERT   every collected cast handle (1 to 4 rows) is also appended to `live`: n_docs = n_sealed + growing rows, base_docs = n_sealed;
  RERANK   the ring is synced only here, so the delta is whatever piled up.  With rows pending the batch goes in twice, around the
           sync, both in flight: A is Table.rerank(side="live") over the rows the directory covered, B over all rows (a ctid names the
           lowest index of sealed + growing: a sealed row beats a growing one, dead or not).  Then B's eligible candidates by index
           (cand_doc) against Table.rerank_docs, on the ring and through the scorer; and once per epoch, with a growing row deleted,
           the records of vbm25_search_batch_growing mapped to indices (0xFFFFFFFF - g is n_sealed + g) and reranked the same way;
  REOPEN   `live`'s arrays and fieldnorm codes are Table.forward_live(); a restart -- a fresh bind plus vbm25_doc_terms_append of the
           growing CSR with its deleted flags -- is forward_live(drop_deleted=True), and a ring made on it answers the last rerank's
           lists like the live ring; the syncs that allocated stay within what doubling allows; a sync of nothing allocates nothing;
  VACUUM   everything above is dropped and made again on the index that was written and read back.
Every comparison is exact: bytes, counts, dtypes.  The model's live side was checked on the CPU first (tests/test_table_model.py).

An epoch without sealed documents has no ring (the refusal is asserted) but its handle still takes the appends.

The seeds are SEEDS_LIVE = (4, 29), not SEEDS_CTID = (1, 4): seed 1 never appends a handle without a known element.

Measured on an MI355X: test_random_life_live 3.3 to 3.9 s per seed and tuning (160 operations, 14 or 15 VACUUMs, 26 or 36 reranks of 8
queries on three rings and a scorer, ten syncs or more with a batch on either side, a restart at every reopen) next to 1.9 to 2.0 s of
test_random_life_by_ctid at seed 4 and 2.5 s at seed 1 in the same run; test_scripted_live_corners 0.5 s next to 0.4 s of
test_scripted_ctid_corners, test_live_life_across_a_tile 0.8 s next to 0.5 s of test_ctid_life_across_a_tile.  At most about twice the
parent: nothing was cut.  No timing is asserted."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import table_model as T
from test_gpu_table_ctid_fuzz import NO_DOCUMENTS, RING_CAPS, CtidLife, Q, assert_same_ranks, lists_csr
from test_gpu_table_fuzz import GT, NONE
from test_table_model import N_OPS, SEED32, SEEDS_LIVE, assert_coverage_ctid, assert_coverage_live, lexeme_universe, new_table_ctid

pytestmark = pytest.mark.gpu
GROWTH = 2   # the factor include/vbm25.h documents for every capacity of an append and a sync
TUNINGS = ({}, dict(live_sort_max=0, tid_dir=0, eval_grid=1), dict(live_sort_max=3, tid_dir=2, eval_grid=3))


def docs_csr(lists):
    return np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.uint64), np.concatenate([np.asarray(l, np.uint32) for l in lists] + [np.zeros(0, np.uint32)])


def fieldnorms(dt):
    f = vb.lib().vbm25_debug_doc_terms_fieldnorm
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 3
    out, flag = np.zeros(max(dt.n_docs, 1), np.uint8), C.c_uint32()
    assert f(dt.h, out.ctypes.data, C.byref(flag)) == 0
    return out[:dt.n_docs]


def assert_forward(dt, want, what):
    """a bound handle's four arrays against the model's, dtype included"""
    assert dt.n_docs == len(want[3]) and dt.n_known == len(want[1]), f"{what}: {dt.n_docs} documents, {dt.n_known} known elements"
    for got, w, name in zip(dt.download() + (fieldnorms(dt),), want, ("start", "term", "tf", "fieldnorm")):
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), f"{what}: {name}"


class LiveLife(CtidLife):
    def __init__(self, *args, **kwargs):
        self.n_ab = self.n_restart_rings = self.n_hit_routes = 0
        super().__init__(*args, **kwargs)

    def attach(self):
        super().attach()
        n_sealed = len(self.m.sealed)
        self.live = self.gix.bind()   # (a second handle: self.bound stays the frozen one the forward-index check reads)
        assert self.live.n_docs == self.live.base_docs == n_sealed
        if n_sealed:
            self.ring_live = self.live.reranker(self.resolver, 3, **RING_CAPS, from_index=True)
            self.scorer = self.live.scorer()   # (made before the handle grows: it sees the new documents)
        else:
            with pytest.raises(vb.Vbm25Error, match=NO_DOCUMENTS):
                self.live.reranker(self.resolver, 3, **RING_CAPS, from_index=True)
            self.ring_live = self.scorer = None
        self.restarted = self.last_rerank = None
        self.syncs_moved = 0   # the syncs of this epoch in which the ring allocated

    def keep(self, cast):
        super().keep(cast)
        n = self.live.n_docs
        self.live.append_documents(cast, self.resolver)
        self.m.live_append(self.live.n_docs - n)

    def insert_rows(self, docs, host_bits=False):
        super().insert_rows(docs, host_bits)
        assert self.live.n_docs == len(self.m.sealed) + len(self.m.growing) and self.live.base_docs == len(self.m.sealed)

    def by_doc(self, queries, lists, k, want, what):
        """lists of live document indices through the ring (cand_doc) and through the scorer made at attach"""
        q_cand, cand_doc = docs_csr(lists)
        self.ring_live.submit([q.lexemes for q in queries], k, q_cand, cand_doc=cand_doc)
        got = self.ring_live.collect()
        assert_same_ranks(got, want, f"{what}, the live ring by index")
        terms, off = self.csr(self.gix, queries)
        top = self.scorer.topk(terms, off, k, q_cand, cand_doc)
        assert top[0].tobytes() == got[0].tobytes() and top[1].tobytes() == got[1].tobytes(), f"{what}: the scorer made at attach and the ring"

    def rerank(self, queries, lists, k, count=True):
        m, ring = self.m, self.ring_live
        queries = [q if isinstance(q, Q) else Q(m, q) for q in queries]
        what = f"epoch {self.epoch} rerank k={k}"
        if ring is None:
            assert not len(m.sealed)
            return super().rerank(queries, lists, k, count)
        q_cand, cand_tid = lists_csr(lists)
        lexemes = [q.lexemes for q in queries]
        covered = ring.directory_docs
        pending = covered != self.live.n_docs
        if pending:
            ring.submit(lexemes, k, q_cand, cand_tid=cand_tid)   # A: against the old directory
            made = ring.allocations()
            ring.sync()
            self.syncs_moved += ring.allocations() != made
            assert ring.directory_docs == self.live.n_docs
        ring.submit(lexemes, k, q_cand, cand_tid=cand_tid)       # B
        assert ring.in_flight() == 1 + pending
        want = super().rerank(queries, lists, k, count)
        assert want["live_covered"] == covered and (want["live_before"] is not None) == pending, what
        if pending:
            assert_same_ranks(ring.collect(), want["live_before"], f"{what}, the live ring before the sync of {self.live.n_docs - covered} rows")
            self.n_ab += 1
        assert_same_ranks(ring.collect(), want["live"], f"{what}, the live ring")
        self.by_doc(queries, want["live_docs"], k, want["live_by_doc"], what)
        if want["hits"] is not None:   # the search's records, growing ones among them, as indices of the live handle
            terms, off = self.csr(self.gix, queries)
            hits, n_hits = vb.search_batch_growing(self.gix, self.grow, terms, off, T.HITS_K)
            n_sealed = len(m.sealed)
            for q, model_hits in enumerate(want["hits"]):
                ids = hits["doc_id"][q, :n_hits[q]].astype(np.int64)
                assert np.array_equal(np.where(ids >= n_sealed, n_sealed + (NONE - ids), ids), model_hits), f"{what}: the search's records, query {q}"
            self.by_doc(queries, want["hits"], k, want["hits_by_doc"], f"{what}, search hits")
            self.n_hit_routes += 1
        self.last_rerank = (queries, lists)
        return want

    def reopen(self):
        """The restart's ring against the live one: a deleted growing row has an empty run after a restart (vbm25_doc_terms_append
        drops the elements of a flagged document) and every element on the live handle (nothing deletes from a bound handle), so its
        score is 0.0 on the one and the model's on the other BY CONSTRUCTION: those entries are compared by pos and doc only.  The
        lists are cut to 1024 candidates and asked at k = 1024, so that no entry is cut on one ring and kept on the other."""
        super().reopen()
        m, ring = self.m, self.ring_live
        what = f"epoch {self.epoch} reopen"
        n_sealed = len(m.sealed)
        assert_forward(self.live, m.forward_live(), f"{what}: the live handle")
        G = m.growing_csr()
        self.restarted = self.gix.bind()
        self.restarted.append(G["g_start"], G["g_key"], G["g_tf"], G["g_fieldnorm"], G["g_payload"], self.resolver, g_deleted=G["g_deleted"])
        assert self.restarted.base_docs == n_sealed
        assert_forward(self.restarted, m.forward_live(drop_deleted=True), f"{what}: the restarted handle")
        if ring is None:
            return
        # the allocation contract: the sorted arrays start at n_sealed entries and at least double when outgrown, the first sync --
        # which also makes what no later one makes again -- counted as a growth step
        bound = max(1, math.ceil(math.log(self.live.n_docs / n_sealed) / math.log(GROWTH)))
        assert self.syncs_moved <= bound, f"{what}: {self.syncs_moved} syncs allocated, doubling from {n_sealed} to {self.live.n_docs} allows {bound}"
        if ring.directory_docs != self.live.n_docs:
            return
        made, held = ring.allocations(), ring.device_bytes()
        ring.sync()   # (nothing new)
        assert (ring.allocations(), ring.device_bytes(), ring.directory_docs) == (made, held, self.live.n_docs), what
        if self.last_rerank is None:
            return
        queries, lists = self.last_rerank
        q_cand, cand_tid = lists_csr([l[:1024] for l in lists])
        with self.restarted.reranker(self.resolver, 1, **RING_CAPS, from_index=True) as fresh:   # (at create, no sync)
            assert fresh.directory_docs == self.live.n_docs
            for r in (ring, fresh):
                r.submit([q.lexemes for q in queries], 1024, q_cand, cand_tid=cand_tid)
            (a, n_a), (b, n_b) = ring.collect(), fresh.collect()
        assert np.array_equal(n_a, n_b), what
        dead = np.r_[np.zeros(n_sealed, bool), np.array(m.growing_deleted, bool)]
        for q, n in enumerate(n_a):
            ra, rb = a[q, :n][np.argsort(a["pos"][q, :n])], b[q, :n][np.argsort(b["pos"][q, :n])]
            assert np.array_equal(ra["pos"], rb["pos"]) and np.array_equal(ra["doc"], rb["doc"]), f"{what}: query {q}, the restart resolves other rows"
            gone = dead[ra["doc"]]
            assert ra["score"][~gone].tobytes() == rb["score"][~gone].tobytes(), f"{what}: query {q}, the restart scores a live row differently"
            assert not rb["score"][gone].any(), f"{what}: query {q}, a deleted growing row scores after the restart"
        self.n_restart_rings += 1

    def vacuum(self, tids=()):
        old = (self.live, self.ring_live, self.restarted, self.scorer)
        super().vacuum(tids)
        del old


@pytest.mark.parametrize("tuning", TUNINGS, ids=lambda t: "-".join(f"{k}={v}" for k, v in t.items()) or "defaults")
@pytest.mark.parametrize("seed", SEEDS_LIVE)
def test_random_life_live(seed, tuning):
    t0 = time.time()
    try:
        for name, value in tuning.items():
            vb.set_tuning(name, value)
        m, universe = new_table_ctid(seed)
        life = LiveLife(m, universe)
        for op in m.ops_ctid(seed, N_OPS, universe):
            life.run(op)
        life.reopen()
    finally:
        vb.reset_tuning()
    assert_coverage_ctid(m, f"seed {seed}")
    assert_coverage_live(m, f"seed {seed}")
    assert life.n_reranks == m.cstats["reranks"] > 0
    assert life.n_ab >= m.cstats["ab_differ"] > 0 and life.n_restart_rings > 0 and life.n_hit_routes >= m.cstats["live_hits"] > 0
    print(f"seed {seed} {tuning}: {time.time() - t0:.1f} s, {life.n_ab} syncs, {life.n_restart_rings} restarts compared")


def test_scripted_live_corners():
    """test_scripted_ctid_corners' sequence on the live stack, its model assertions carried over (one INSERT of two rows without a
    known element is added, so the rows behind it have moved by two), with what the live side adds.  It pins the DOCUMENTED
    behaviour of a dead sealed row's ctid that is inserted again before the VACUUM: on the live ring the ctid still names the sealed
    row, as nothing deletes documents from a bound handle; after the VACUUM it names the one row that exists."""
    universe = lexeme_universe()
    lex = [t for t, _ in universe]
    rows, keys = T.random_rows(700, 300, 5, keys=[key for _, key in universe])
    shared = []
    for lo, hi in ((3, 400), (10, 690)):
        rows[hi] = (rows[lo][0],) + rows[hi][1:]
        shared.append(next(lex[keys.index(key)] for key in sorted(rows[hi][1]) if key not in rows[lo][1]))
    m = T.Table(rows, 1.2, 0.75, SEED32)
    life = LiveLife(m, universe)
    sel = [(NONE, 0, 1)[q % 3] for q in range(8)]
    ctid = [p for p, _, _ in rows]
    absent = [(0, 9, 0), (65535, 65535, 65535), (0, 0, 0)]

    def selects(queries, ks=(10, 300)):
        queries = (queries * 8)[:8]
        for front, k in [(f, k) for f in (0, 1, 2) for k in ks]:
            life.select(queries, sel, k, front)

    def reranks(queries, lists, ks=(1, 10, 65)):
        queries, lists = (queries * 8)[:8], (lists * 8)[:8]
        return [life.rerank(queries, lists, k) for k in ks]

    # a ctid of two sealed rows: the rerank names the lower one, a delete kills both
    want = reranks([[shared[0]], [shared[0], lex[1]]], [[ctid[400], ctid[5]], [ctid[5], ctid[3], ctid[3]]])[1]
    assert want["sealed"][0]["doc"][0, :2].tolist() == [5, 3] or want["sealed"][0]["doc"][0, :2].tolist() == [3, 5]
    assert 400 not in want["sealed"][0]["doc"] and want["sealed"][1].tolist() == [2, 3] * 4 and not want["growing"][1].any()
    assert want["live"][0].tobytes() == want["sealed"][0].tobytes() and want["live_before"] is None
    assert life.delete_tids([ctid[400]]) == (2, 0, 0) and m.sealed_deleted[[3, 400]].all()
    selects([[lex[0], lex[1]], [shared[0]]])
    # inserts: every lexeme unknown, no lexeme at all, one lexeme repeated to a tf above 1
    life.know(b"brand new", b"newer")
    life.insert_rows([((1, 2, 4), [(b"brand new", 1), (b"newer", 4)]), ((1, 2, 6), []),
                      ((1, 2, 9), [(lex[5], 1), (lex[200], 1), (lex[5], 2)])])
    assert m.growing[2][1] == {keys[5]: 3, keys[200]: 1}
    selects([[lex[5], lex[200]], [b"brand new", b"newer"], [b"newer", lex[5]]])
    want = reranks([[lex[5], lex[5], lex[200]], [b"brand new"]], [[(1, 2, 9), (1, 2, 4), ctid[20], (1, 2, 6)], [(1, 2, 6)] + absent])[2]
    assert want["growing"][0]["doc"][0, :3].tolist() == [2, 0, 1] and want["growing"][0]["score"][0, 0] > 0
    assert want["growing"][1].tolist() == [3, 1] * 4 and want["sealed"][1].tolist() == [1, 0] * 4
    assert want["live"][1].tolist() == [4, 1] * 4 and want["live"][0]["score"][0, :4][want["live"][0]["doc"][0, :4] == 702] > 0
    assert sorted(want["live"][0]["doc"][0, :4].tolist()) == [20, 700, 701, 702] and want["live_before"] is None   # (synced at k = 1)
    # a delta of a row without lexemes and a row of only unknown ones: no known element arrives, two documents do
    known = life.live.n_known
    life.insert_rows([((1, 2, 7), []), ((1, 2, 8), [(b"newer", 2)])])
    assert life.live.n_known == known and life.live.n_docs == 705 and m.cstats["unknown_handle"] == 1
    want = reranks([[lex[5], b"newer"]], [[(1, 2, 8), (1, 2, 7), (1, 2, 9), absent[0]]], ks=(10,))[0]
    assert want["live_before"][1].tolist() == [1] * 8 and want["live"][1].tolist() == [3] * 8
    assert want["live"][0]["doc"][0, :3].tolist() == [702, 704, 703] and want["live"][0]["score"][0, 1:3].tolist() == [0.0, 0.0]
    # a query of only unknown lexemes: every candidate scores 0.0 and keeps the list's order; the empty query likewise
    life.know(b"nowhere")
    want = reranks([[b"nowhere", T.NO_ROW_LEXEME], []], [[ctid[9], ctid[8], (1, 2, 9), ctid[7]]])[1]
    assert want["sealed"][0]["doc"][0, :3].tolist() == [9, 8, 7] and not want["sealed"][0]["score"].any()
    assert want["live"][0]["doc"][0, :4].tolist() == [9, 8, 702, 7] and not want["live"][0]["score"].any()
    selects([[b"nowhere"], [b"nowhere", lex[0]]])
    # k = 1024 with 1025 candidates: repeated ctids are entries like any other
    rng = np.random.default_rng(5)
    many = [ctid[int(d)] for d in rng.integers(0, 700, 1025)]
    want = reranks([[lex[0], lex[2], lex[7]]], [many, many[:1024], [(1, 2, 9)] * 1025], ks=(1024,))[0]
    assert want["sealed"][1].tolist() == [1024, 1024, 0] * 2 + [1024, 1024] and want["growing"][1][2] == 1024
    assert want["live"][1].tolist() == [1024] * 8 and (want["live"][0]["doc"][2] == 702).all()
    # a sealed row is deleted and its ctid inserted again: each ring resolves its own copy, THE LIVE RING THE SEALED ONE; after the
    # VACUUM only the new one exists
    assert ctid[7][2] % 3 and life.delete_tids([ctid[7], absent[0]]) == (1, 0, 0)
    life.insert_rows([(ctid[7], [(lex[0], 2), (lex[250], 1)])], host_bits=True)
    want = reranks([[lex[0], lex[250]]], [[ctid[7]], [absent[1], ctid[7], absent[2]]])[0]
    assert want["sealed"][0]["doc"][0, 0] == 7 and want["growing"][0]["doc"][0, 0] == 5 and want["growing"][0]["pos"][1, 0] == 1
    assert m.sealed_deleted[7] and want["live"][0]["doc"][:, 0].tolist() == [7] * 8 and want["live"][1].tolist() == [1] * 8
    assert want["live_before"][0].tobytes() == want["live"][0].tobytes()   # (a sync of exactly one row, which no ctid names)
    selects([[lex[0], lex[250]]])
    # a bulkdelete that kills the second pair of sealed rows with one ctid, a growing row and nothing for an absent ctid
    life.vacuum([ctid[10], (1, 2, 6), absent[0]])
    assert m.vacuums[-1] == (5, 1, 2) and len(m.sealed) == 700
    assert [p for p, _, _ in m.sealed].count(ctid[7]) == 1 and life.live.n_docs == life.live.base_docs == 700
    want = reranks([[lex[0], lex[250]]], [[ctid[7], ctid[10], ctid[690], ctid[11]]])[1]
    assert want["sealed"][1][0] == 2 and 699 in want["sealed"][0]["doc"][0, :2] and not want["growing"][1].any()
    assert want["live"][0].tobytes() == want["sealed"][0].tobytes() and m.sealed[699][0] == ctid[7]
    selects([[b"brand new", b"newer"], [lex[0], lex[250]]])
    # a bulkdelete of the empty set, one of only absent ctids
    life.vacuum([])
    life.vacuum(absent)
    assert m.vacuums[-2:] == [(0, 0, 0), (0, 0, 0)] and len(m.sealed) == 700
    selects([[lex[3], lex[40]]])
    # two growing rows of ONE delta with one ctid: the ctid names the lower
    life.insert_rows([((4, 4, 4), [(lex[1], 1)]), ((9, 9, 10), [(lex[3], 1)]), ((9, 9, 10), [(lex[3], 2), (lex[40], 1)])])
    want = reranks([[lex[3], lex[40]]], [[(9, 9, 10), (4, 4, 4), (9, 9, 10)]], ks=(10,))[0]
    assert want["live"][1].tolist() == [3] * 8 and sorted(want["live"][0]["doc"][0, :3].tolist()) == [700, 701, 701]
    assert want["live"][0]["score"][0, 0] == want["live"][0]["score"][0, 1] > 0 and not want["live_before"][1].any()
    # a bulkdelete of everything: the empty index binds to no documents and no ring can be made on it
    life.vacuum([p for p, _, _ in m.sealed] + [(4, 4, 4), (9, 9, 10)])
    assert len(m.sealed) == 0 and life.bound.n_docs == 0 and life.ring_ix is None
    assert life.live.n_docs == 0 == life.live.base_docs and life.ring_live is None
    life.rerank([[lex[1]]], [[(4, 4, 4)] + absent], 10)
    life.insert_rows([((5, 5, 6), [(lex[1], 2), (lex[2], 1)]), ((5, 5, 7), [(lex[2], 5)])])   # (appended to the handle of no document)
    assert life.live.n_docs == 2 and life.live.base_docs == 0 and life.live.n_known == 0
    assert_forward(life.live, m.forward_live(), "the handle of an index without sealed documents")
    assert m.forward_live()[0].tolist() == [0, 0, 0]   # (all runs empty: the vocabulary is empty)
    with pytest.raises(vb.Vbm25Error, match=NO_DOCUMENTS):
        life.live.reranker(life.resolver, 3, **RING_CAPS, from_index=True)
    life.rerank([[lex[1]]], [[(5, 5, 6)]], 10)
    selects([[lex[2]], [lex[1], lex[2]]])
    life.vacuum()
    assert len(m.sealed) == 2
    want = reranks([[lex[2]], [lex[1], lex[2]]], [[(5, 5, 7), (5, 5, 6)] + absent])[1]
    assert want["sealed"][1].tolist() == [2] * 8 and (want["sealed"][0]["score"][:, :2] > 0).all()
    assert want["live"][0].tobytes() == want["sealed"][0].tobytes() and life.live.n_docs == 2 == life.live.base_docs
    selects([[lex[2]], [lex[1], lex[2]]])
    life.reopen()


def test_live_life_across_a_tile():
    """test_ctid_life_across_a_tile's epoch on the live stack: appends of 1024 rows, a first sync of 5000 rows (past the LDS sort's
    4096) on a directory of 1000, a second of 3300 that the handle takes partly in its room to spare; reranks over ctids on both
    sides of n_sealed and of the tile, the cand_doc and search-hit routes after the ctid deletes"""
    t0 = time.time()
    universe = lexeme_universe()
    lex = [t for t, _ in universe]
    rows, _ = T.random_rows(1000, 300, 6, keys=[key for _, key in universe])
    m = T.Table(rows, 1.2, 0.75, SEED32)
    life = LiveLife(m, universe, cast_docs=1024, cast_lexemes=1 << 15, cast_bytes=1 << 20)
    rng = np.random.default_rng(6)

    def doc(i):
        row = [(lex[j], int(rng.integers(1, 5))) for j in rng.choice(300, int(rng.integers(3, 7)), replace=False)]
        if i % 50 == 0:
            life.know(b"n%06d" % i)
            row[0] = (b"n%06d" % i, 1)
        return (1 + i // 60000, i % 60000, 1 + i % 7), row + row[:1]   # (the first lexeme twice)

    def some_queries():
        return [[lex[j] for j in rng.choice(300, int(rng.integers(1, 4)))] for _ in range(8)]

    life.insert_rows([doc(i) for i in range(5000)])
    first = [[m.growing[int(g)][0] for g in [0, 4095, 4096, 4999] + [int(x) for x in rng.integers(0, 5000, 100)]] + [(0, 0, 0)]
             + [m.sealed[int(d)][0] for d in [0, 999] + [int(x) for x in rng.integers(0, 1000, 20)]] for _ in range(8)]
    want = life.rerank(some_queries(), first, 65)   # the first sync: 5000 rows, five appends
    assert want["live_covered"] == 1000 and life.ring_live.directory_docs == 6000 and life.syncs_moved == 1
    assert want["live_before"][0].tobytes() != want["live"][0].tobytes()
    life.insert_rows([doc(i) for i in range(5000, 8300)])   # (this append crosses the tile)
    assert life.grow.n_docs == 8300 > GT and life.live.n_docs == 9300 and life.ring_live.directory_docs == 6000
    g_ctid = [p for p, _, _ in m.growing]
    edge = [0, GT - 1, GT, 8299]
    gone = sorted(set(edge) | {int(g) for g in rng.choice(8300, 196, replace=False)})
    n_dead = life.delete_tids([g_ctid[g] for g in gone] + [m.sealed[d][0] for d in (0, 999)] + [(0, 0, 0)])
    assert n_dead == (2, len(gone), len(gone))
    sel = [(NONE, 0, 1)[q % 3] for q in range(8)]

    def work():
        for front in (0, 1, 2):
            queries = some_queries()
            life.select(queries, sel, 1025 if front == 0 else life.k, front)
            lists = [[g_ctid[g] for g in edge + [int(x) for x in rng.integers(GT - 100, GT + 100, 150)]] + [(0, 0, 0)]
                     + [m.sealed[int(d)][0] for d in rng.integers(0, len(m.sealed), 20)] for _ in range(8)]
            life.rerank(queries, lists, (10, 65, 1024)[front])

    work()   # (the second sync: 3300 rows)
    assert life.ring_live.directory_docs == 9300 and life.n_ab == 2 and life.n_hit_routes == 1 and m.cstats["live_hits"] == 1
    assert m.stats["both"] > 0 and m.cstats["rerank_both"] > 0 and m.cstats["live_both"] > 0
    life.reopen()
    assert life.n_restart_rings == 1
    more = [int(g) for g in rng.choice(8300, 100, replace=False)] + [GT - 2, GT + 1]
    life.vacuum([g_ctid[g] for g in more] + [m.sealed[int(d)][0] for d in rng.choice(1000, 50, replace=False)] + [(0, 0, 0)])
    assert m.vacuums[-1][0] >= 50 and m.vacuums[-1][1] >= len(gone) and m.vacuums[-1][2] > 100
    work()   # (the same ctids name sealed rows now, or nothing)
    life.reopen()
    print(f"{time.time() - t0:.1f} s")
