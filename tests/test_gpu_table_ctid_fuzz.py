"""tests/test_gpu_table_fuzz.py's life driven the way an integration drives it: by lexeme and ctid, through the device objects that
take them.  CtidLife carries, besides Life's handles, a Resolver, the index's own forward index (GpuIndex.bind) with a reranker ring
on it, one Caster for the whole life and the epoch's inserts as one Documents handle with a second reranker ring on its bind:
  SELECT   the CSR comes from Resolver.submit / collect of the lexemes and equals the model's ranks, then Life's three front ends;
  INSERT   batches of at most four rows through the caster, two in flight, each collected handle appended (append_documents) and kept
           (Documents.extend) before its slot is taken again; the growing bitmaps extended without bits, then set from ctid sets;
  DELETE   one TidSet of the statement's ctids: GrowingSegment.delete_tids; bitmap 0 = "the ctid is not among the epoch's dead ones",
           bitmap 1 = "the ctid is a live tenant row's", both halves by DocFilter.set_tids, read back against the model's predicates;
  RERANK   the same lexemes and ctid lists to both rings, byte for byte Table.rerank of the sealed and of the growing rows; once per
           epoch the forward index against Table.forward;
  VACUUM   DeviceVacuum.from_pages of the pages as they are, bulkdelete of "the dead TIDs the heap reports" -- the same TidSet also
           deletes from the long-lived growing segment and the bitmaps follow -- its counts and flags against a fresh read of the
           model's patched pages, and this handle is what Life.vacuum compacts, remaps and writes; the next epoch's Resolver, bind
           and rings are made from the index that was written and read back.
The model was checked on the CPU first (tests/test_table_model.py), so a mismatch here is a finding about the library.  Every
comparison is exact: bytes, counts, bitmaps.

A reranker refuses an index without sealed documents (the `<&>` operator has no average length there): in such an epoch the life
asserts that refusal for both rings and has no ring.

Measured on an MI355X: test_random_life_by_ctid 2.0 to 2.5 s per seed (160 operations, 14 to 15 VACUUMs, about 500 selects, 26 to 33
reranks of 8 queries on both rings), next to 1.4 to 1.9 s per seed of test_gpu_table_fuzz.py's test_random_life in the same runs;
test_scripted_ctid_corners 0.4 to 0.7 s, test_ctid_life_across_a_tile 0.5 to 0.8 s.  Nothing had to be cut."""
import time

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import table_model as T
import vectors_device_data as V
from test_gpu_table_fuzz import GT, NONE, Life, packed
from test_table_model import N_OPS, SEED32, SEEDS_CTID, assert_coverage_ctid, lexeme_universe, new_table_ctid

pytestmark = pytest.mark.gpu
QUERY_CAPS = (8, 64, 4096)   # a batch: queries, lexemes, lexeme bytes
RING_CAPS = dict(max_queries=8, max_lexemes=64, max_bytes=4096, max_candidates=16384, max_k=1024)
NO_DOCUMENTS = "evaluate on an index without sealed documents"


class Q(list):
    """a query as Life hands it around -- the model's sorted distinct keys -- with the lexemes the device is given"""

    def __init__(self, m, lexemes):
        super().__init__(m.keys_of(lexemes))
        self.lexemes = [bytes(t) for t in lexemes]


def tid_array(tids):
    return np.array([tuple(t) for t in tids], np.uint16).reshape(-1, 3)


def lists_csr(lists):
    return np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.uint64), tid_array([t for l in lists for t in l])


def assert_same_ranks(got, want, what):
    assert got[0].dtype == vb.RANK_DTYPE and got[0].shape == want[0].shape and got[1].dtype == np.uint32, what
    assert np.array_equal(got[1], want[1]), f"{what}: n_ranks {got[1]}, the model has {want[1]}"
    for q in range(len(want[1])):
        if got[0][q].tobytes() != want[0][q].tobytes():
            i = int(np.flatnonzero(got[0][q].view("V16") != want[0][q].view("V16"))[0])
            raise AssertionError(f"{what}: query {q} ({want[1][q]} ranks) differs first at entry {i}: {got[0][q, i]}, the model has {want[0][q, i]}")


class CtidLife(Life):
    def __init__(self, model, universe, cast_docs=4, cast_lexemes=4096, cast_bytes=1 << 18):
        model.key_of = {lexeme: key for lexeme, key in universe}
        model.key_of[T.NO_ROW_LEXEME] = T.NO_ROW_KEY
        self.lexeme_of = {key: lexeme for lexeme, key in universe}
        self.cast_docs = cast_docs
        self.caster = vb.Caster(0, 2, cast_docs, cast_lexemes, cast_bytes, seed=SEED32)
        self.n_reranks = 0
        super().__init__(model)
        self.last = ([Q(model, [self.lexeme_of[key]]) for key in model.vocab[:8]], self.last[1])

    def know(self, *lexemes):
        """lexemes of less than 16 bytes that no row has held: their keys are the bytes, zero padded (vector.rs:21-24)"""
        for t in lexemes:
            assert len(t) < 16 and b"\0" not in t
            self.m.key_of[t] = t.ljust(16, b"\0")

    def attach(self):
        super().attach()
        self.resolver = vb.Resolver(self.gix, 2, *QUERY_CAPS, seed=SEED32)
        self.bound = self.gix.bind()
        assert self.bound.n_docs == len(self.m.sealed)
        self.ring_ix = self.make_ring(self.bound, from_index=True)
        self.epoch_docs = vb.Documents.empty(payload=True)
        self.ring_docs, self.ring_docs_rows = None, -1
        self.dead = []            # every ctid a DELETE or a bulkdelete of this epoch has named
        self.host_bits = False    # (True: the bitmaps come from the model's bits, see set_bitmaps)
        self.forward_checked = False

    def make_ring(self, bound, **how):
        """a depth-2 reranker ring on `bound`, or None with the refusal asserted where the index has no sealed documents"""
        if len(self.m.sealed):
            return bound.reranker(self.resolver, 2, **RING_CAPS, **how)
        with pytest.raises(vb.Vbm25Error, match=NO_DOCUMENTS):
            bound.reranker(self.resolver, 2, **RING_CAPS, **how)
        return None

    # ---- SELECT: the CSR from the resolver

    def csr(self, gix, queries):
        r = self.resolver if gix is self.gix else vb.Resolver(gix, 1, *QUERY_CAPS, seed=SEED32)
        r.submit([q.lexemes for q in queries])
        terms, off = r.collect()
        want = [sorted(self.m.rank[key] for key in q if key in self.m.rank) for q in queries]   # (q: sorted distinct keys)
        assert terms.dtype == np.uint32 and off.dtype == np.uint32
        assert np.array_equal(off, np.r_[0, np.cumsum([len(t) for t in want])]), f"epoch {self.epoch}: the resolver's offsets"
        assert np.array_equal(terms, np.array([t for ids in want for t in ids], np.uint32)), f"epoch {self.epoch}: the resolver's term ids"
        return terms, off

    def select(self, queries, selectors, k, front, count=True):
        super().select([q if isinstance(q, Q) else Q(self.m, q) for q in queries], selectors, k, front, count)

    # ---- INSERT: through the caster

    def keep(self, cast):
        """one collected cast handle goes to everything that holds the epoch's inserts"""
        self.grow.append_documents(cast)
        self.epoch_docs.extend(cast)

    def insert_rows(self, docs, host_bits=False):
        """docs: [(payload, [(lexeme, count)])], one INSERT statement"""
        m, batch, pending = self.m, self.m.new_batch(), 0
        for payload, lexrow in docs:
            m.insert(payload, m.cast(lexrow), batch)

        def take():
            self.keep(self.caster.collect())   # (before the slot is taken again)

        for lo in range(0, len(docs), self.cast_docs):
            if pending == 2:
                take()
                pending -= 1
            part = docs[lo:lo + self.cast_docs]
            self.caster.submit([row for _, row in part], tid_array([p for p, _ in part]))
            pending += 1
        for _ in range(pending):
            take()
        assert self.grow.n_docs == self.epoch_docs.n_docs == len(m.growing)
        self.filt.extend_growing(self.grow)   # no bits: the new rows are hidden until the bitmaps are set
        self.host_bits |= host_bits
        self.set_bitmaps()

    # ---- DELETE by ctid, and the bitmaps from ctid sets

    def set_bitmaps(self):
        """both bitmaps, both halves, from ctid sets, and back against the model's predicates.  host_bits: from the model's bits
        instead, until the next VACUUM -- while a dead sealed row's ctid is carried by a live growing row again, which a heap does not
        do before the VACUUM, no set of ctids tells the two apart."""
        m = self.m
        if self.host_bits:
            for i in (0, 1):
                self.filt.update(i, self.keeps(0)[i])
                self.filt.update_growing(i, self.keeps(1)[i])
        else:
            with vb.TidSet(tid_array(self.dead)) as dead:
                self.filt.set_tids(0, dead, invert=True, growing=self.grow)
            tenant_s, tenant_g = m.tenant()
            live = [p for (p, _, _), keep in zip(m.sealed, tenant_s) if keep] + [p for (p, _, _), keep in zip(m.growing, tenant_g) if keep]
            with vb.TidSet(tid_array(live)) as tenant:
                self.filt.set_tids(1, tenant, False, self.grow)
        for i in (0, 1):
            assert np.array_equal(self.filt.read(i), packed(self.keeps(0)[i])), f"epoch {self.epoch}: sealed bitmap {i}"
            assert np.array_equal(self.filt.read(i, growing=True), packed(self.keeps(1)[i])), f"epoch {self.epoch}: growing bitmap {i}"

    def delete_tids(self, tids):
        n_sealed, n_grow, matched = self.m.delete_tids(tids, "delete")
        with vb.TidSet(tid_array(tids)) as ts:
            assert ts.n_unique == len({tuple(t) for t in tids})
            assert self.grow.delete_tids(ts) == matched, f"epoch {self.epoch}: delete_tids' count"
        self.dead += [tuple(t) for t in tids]
        self.set_bitmaps()
        return n_sealed, n_grow, matched

    # ---- RERANK: the index's ring and the epoch's documents' ring

    def rerank(self, queries, lists, k, count=True):
        m = self.m
        queries = [q if isinstance(q, Q) else Q(m, q) for q in queries]
        what = f"epoch {self.epoch} rerank k={k}"
        if self.ring_docs_rows != self.grow.n_docs:   # the growing segment changed since the last rerank
            if self.ring_docs is not None:
                self.ring_docs.close()
            self.docs_bound = self.epoch_docs.bind(self.resolver)
            assert self.docs_bound.n_docs == len(m.growing)
            self.ring_docs = self.make_ring(self.docs_bound, documents=self.epoch_docs)
            self.ring_docs_rows = self.grow.n_docs
        if not self.forward_checked:
            for got, want, name in zip(self.bound.download(), m.forward(), ("start", "term", "tf")):
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), f"epoch {self.epoch}: the forward index's {name}"
            self.forward_checked = True
        if not len(m.sealed):
            assert self.ring_ix is None and self.ring_docs is None
            return
        want = m.rerank_op(queries, lists, k, count=count)
        q_cand, cand_tid = lists_csr(lists)
        lexemes = [q.lexemes for q in queries]
        self.ring_ix.submit(lexemes, k, q_cand, cand_tid=cand_tid)
        self.ring_docs.submit(lexemes, k, q_cand, cand_tid=cand_tid)
        assert_same_ranks(self.ring_ix.collect(), want["sealed"], f"{what}, the index's ring")
        assert_same_ranks(self.ring_docs.collect(), want["growing"], f"{what}, the documents' ring")
        self.n_reranks += 1
        return want

    # ---- REOPEN, VACUUM

    def reopen(self):
        super().reopen()
        got, want = self.epoch_docs.download(), dict(self.m.growing_csr())
        want["g_deleted"] = np.zeros_like(want["g_deleted"])   # (cast documents carry no deleted flags)
        if got["g_payload"] is None:   # (a handle of no documents has no payload array to give)
            assert self.epoch_docs.n_docs == 0
            got["g_payload"] = np.zeros((0, 3), np.uint16)
        V.assert_same_csr(got, want, f"epoch {self.epoch}: the epoch's cast documents")

    def vacuum(self, tids=()):
        m = self.m
        dv = vb.DeviceVacuum.from_pages(self.gix, m.page_list())   # the pages as they are
        assert (dv.n_sealed, dv.n_sealed_deleted, dv.n_grow, dv.n_grow_deleted, dv.n_elements) == m.counts()
        n_sealed, n_grow, matched = m.delete_tids(tids, "bulkdelete")
        with vb.TidSet(tid_array(tids)) as ts:   # one set, three consumers
            assert dv.bulkdelete(self.gix, ts) == (n_sealed, n_grow), f"epoch {self.epoch}: bulkdelete's counts"
            assert self.grow.delete_tids(ts) == matched, f"epoch {self.epoch}: delete_tids' count"
            self.dead += [tuple(t) for t in tids]
            self.set_bitmaps()
        fresh = vb.DeviceVacuum.from_pages(self.gix, m.page_list())   # the model's pages, patched
        for got, want, name in zip(dv.read(), fresh.read(), ("sealed deleted words", "growing deleted flags")):
            assert got.dtype == want.dtype and np.array_equal(got, want), f"epoch {self.epoch}: bulkdelete's {name}"
        assert (dv.n_sealed, dv.n_sealed_deleted, dv.n_grow, dv.n_grow_deleted, dv.n_elements) == m.counts() == \
            (fresh.n_sealed, fresh.n_sealed_deleted, fresh.n_grow, fresh.n_grow_deleted, fresh.n_elements)
        old = (self.resolver, self.bound, self.ring_ix, self.epoch_docs, self.ring_docs)
        super().vacuum(dv=dv)
        del old

    def run(self, op):
        if op[0] == "insert":
            self.insert_rows(op[1])
        elif op[0] == "delete_tids":
            self.delete_tids(op[1])
        elif op[0] == "select":
            assert op[4] == 0 or op[3] == self.k
            self.select(*op[1:])
        elif op[0] == "rerank":
            self.rerank(*op[1:])
        elif op[0] == "reopen":
            self.reopen()
        else:
            self.vacuum(op[1])


@pytest.mark.parametrize("seed", SEEDS_CTID)
def test_random_life_by_ctid(seed):
    t0 = time.time()
    m, universe = new_table_ctid(seed)
    life = CtidLife(m, universe)
    for op in m.ops_ctid(seed, N_OPS, universe):
        life.run(op)
    life.reopen()
    assert_coverage_ctid(m, f"seed {seed}")
    assert life.n_reranks == m.cstats["reranks"] > 0
    print(f"seed {seed}: {time.time() - t0:.1f} s")


def test_scripted_ctid_corners():
    """what chance may not give, in one sequence; 700 rows: the documents tape crosses one page (680 tuples)"""
    universe = lexeme_universe()
    lex = [t for t, _ in universe]
    rows, keys = T.random_rows(700, 300, 5, keys=[key for _, key in universe])
    # two pairs of sealed rows share a ctid; the second of each holds a key the first lacks
    shared = []
    for lo, hi in ((3, 400), (10, 690)):
        rows[hi] = (rows[lo][0],) + rows[hi][1:]
        shared.append(next(lex[keys.index(key)] for key in sorted(rows[hi][1]) if key not in rows[lo][1]))
    m = T.Table(rows, 1.2, 0.75, SEED32)
    life = CtidLife(m, universe)
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
    # a query of only unknown lexemes: every candidate scores 0.0 and keeps the list's order; the empty query likewise
    life.know(b"nowhere")
    want = reranks([[b"nowhere", T.NO_ROW_LEXEME], []], [[ctid[9], ctid[8], (1, 2, 9), ctid[7]]])[1]
    assert want["sealed"][0]["doc"][0, :3].tolist() == [9, 8, 7] and not want["sealed"][0]["score"].any()
    selects([[b"nowhere"], [b"nowhere", lex[0]]])
    # k = 1024 with 1025 candidates: repeated ctids are entries like any other
    rng = np.random.default_rng(5)
    many = [ctid[int(d)] for d in rng.integers(0, 700, 1025)]
    want = reranks([[lex[0], lex[2], lex[7]]], [many, many[:1024], [(1, 2, 9)] * 1025], ks=(1024,))[0]
    assert want["sealed"][1].tolist() == [1024, 1024, 0] * 2 + [1024, 1024] and want["growing"][1][2] == 1024
    # a sealed row is deleted and its ctid inserted again: each ring resolves its own copy; after the VACUUM only the new one exists
    assert ctid[7][2] % 3 and life.delete_tids([ctid[7], absent[0]]) == (1, 0, 0)
    life.insert_rows([(ctid[7], [(lex[0], 2), (lex[250], 1)])], host_bits=True)
    want = reranks([[lex[0], lex[250]]], [[ctid[7]], [absent[1], ctid[7], absent[2]]])[0]
    assert want["sealed"][0]["doc"][0, 0] == 7 and want["growing"][0]["doc"][0, 0] == 3 and want["growing"][0]["pos"][1, 0] == 1
    selects([[lex[0], lex[250]]])
    # a bulkdelete that kills the second pair of sealed rows with one ctid, a growing row and nothing for an absent ctid
    life.vacuum([ctid[10], (1, 2, 6), absent[0]])
    assert m.vacuums[-1] == (5, 1, 2) and len(m.sealed) == 698
    assert [p for p, _, _ in m.sealed].count(ctid[7]) == 1
    want = reranks([[lex[0], lex[250]]], [[ctid[7], ctid[10], ctid[690], ctid[11]]])[1]
    assert want["sealed"][1][0] == 2 and 697 in want["sealed"][0]["doc"][0, :2] and not want["growing"][1].any()
    selects([[b"brand new", b"newer"], [lex[0], lex[250]]])
    # a bulkdelete of the empty set, one of only absent ctids
    life.vacuum([])
    life.vacuum(absent)
    assert m.vacuums[-2:] == [(0, 0, 0), (0, 0, 0)] and len(m.sealed) == 698
    selects([[lex[3], lex[40]]])
    # a bulkdelete of everything: the empty index binds to no documents and no ring can be made on it
    life.insert_rows([((4, 4, 4), [(lex[1], 1)])])
    life.vacuum([p for p, _, _ in m.sealed] + [(4, 4, 4)])
    assert len(m.sealed) == 0 and life.bound.n_docs == 0 and life.ring_ix is None
    life.rerank([[lex[1]]], [[(4, 4, 4)] + absent], 10)
    life.insert_rows([((5, 5, 6), [(lex[1], 2), (lex[2], 1)]), ((5, 5, 7), [(lex[2], 5)])])
    life.rerank([[lex[1]]], [[(5, 5, 6)]], 10)
    selects([[lex[2]], [lex[1], lex[2]]])
    life.vacuum()
    assert len(m.sealed) == 2
    want = reranks([[lex[2]], [lex[1], lex[2]]], [[(5, 5, 7), (5, 5, 6)] + absent])[1]
    assert want["sealed"][1].tolist() == [2] * 8 and (want["sealed"][0]["score"][:, :2] > 0).all()
    selects([[lex[2]], [lex[1], lex[2]]])
    life.reopen()


def test_ctid_life_across_a_tile():
    """one epoch of more than a growing tile (GT documents) appended through the caster; ctid deletes and bitmaps on both sides of the
    tile boundary, reranks over the documents' ring, a bulkdelete that spans both segments, VACUUM"""
    universe = lexeme_universe()
    lex = [t for t, _ in universe]
    rows, _ = T.random_rows(1000, 300, 6, keys=[key for _, key in universe])
    m = T.Table(rows, 1.2, 0.75, SEED32)
    life = CtidLife(m, universe, cast_docs=1024, cast_lexemes=1 << 15, cast_bytes=1 << 20)
    rng = np.random.default_rng(6)

    def doc(i):
        row = [(lex[j], int(rng.integers(1, 5))) for j in rng.choice(300, int(rng.integers(3, 7)), replace=False)]
        if i % 50 == 0:
            life.know(b"n%06d" % i)
            row[0] = (b"n%06d" % i, 1)
        return (1 + i // 60000, i % 60000, 1 + i % 7), row + row[:1]   # (the first lexeme twice)

    life.insert_rows([doc(i) for i in range(5000)])
    life.insert_rows([doc(i) for i in range(5000, 8300)])   # (this append crosses the tile)
    assert life.grow.n_docs == 8300 > GT
    g_ctid = [p for p, _, _ in m.growing]
    edge = [0, GT - 1, GT, 8299]
    gone = sorted(set(edge) | {int(g) for g in rng.choice(8300, 196, replace=False)})
    n_dead = life.delete_tids([g_ctid[g] for g in gone] + [m.sealed[d][0] for d in (0, 999)] + [(0, 0, 0)])
    assert n_dead == (2, len(gone), len(gone))
    sel = [(NONE, 0, 1)[q % 3] for q in range(8)]

    def work():
        for front in (0, 1, 2):
            queries = [[lex[j] for j in rng.choice(300, int(rng.integers(1, 4)))] for _ in range(8)]
            life.select(queries, sel, 1025 if front == 0 else life.k, front)
            lists = [[g_ctid[g] for g in edge + [int(x) for x in rng.integers(GT - 100, GT + 100, 150)]] + [(0, 0, 0)]
                     + [m.sealed[int(d)][0] for d in rng.integers(0, len(m.sealed), 20)] for _ in range(8)]
            life.rerank(queries, lists, (10, 65, 1024)[front])

    work()
    assert m.stats["both"] > 0 and m.cstats["rerank_both"] > 0
    life.reopen()
    more = [int(g) for g in rng.choice(8300, 100, replace=False)] + [GT - 2, GT + 1]
    life.vacuum([g_ctid[g] for g in more] + [m.sealed[int(d)][0] for d in rng.choice(1000, 50, replace=False)] + [(0, 0, 0)])
    assert m.vacuums[-1][0] >= 50 and m.vacuums[-1][1] >= len(gone) and m.vacuums[-1][2] > 100
    work()   # (the same ctids name sealed rows now, or nothing)
    life.reopen()
