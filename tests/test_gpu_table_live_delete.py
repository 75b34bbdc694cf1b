"""tests/test_gpu_table_live_fuzz.py's life with the deletes mirrored onto the rerank stack (vbm25_doc_terms_delete*, csrc/live.hip).
DeleteLife is LiveLife, unchanged, plus ONE more index-bound handle per epoch (`dlive`) with its own depth-3 ring and scorer:
  attach   the handle, ring and scorer are made before the handle grows; rows the model holds dead already die by index (delete);
  INSERT   every collected cast handle is appended to `dlive` as to `live`;
  DELETE   every delete_tids of the life reaches `dlive` as one TidSet (delete_tids); a VACUUM's bulkdelete set does before the
           compaction drops the handle.  After each, read_dead() is the model's deleted flags, sealed then growing, and the count
           returned is the number of rows that were alive;
  RERANK   the ring is synced where LiveLife syncs its own, with a batch on either side; each is held against the model's live side
           WITH THE DEAD ROWS LEFT OUT: a ctid names the lowest LIVE index of sealed + growing that carries it (of the rows the
           directory covers), scored and cut by the model's own _row_score and _top.  The model's eligible indices (dead ones among
           them) then go in as cand_doc: the dead ones take no rank and keep their pos, on the ring and through the scorer.
LiveLife's own handle is never deleted from, so every assertion of the parent driver holds as it did -- among them the pinned one that
a dead sealed row's ctid, inserted again, still names the sealed row THERE.  On `dlive` it names the new row: asserted below.
The driver classes and tests/table_model.py are imported unchanged; the scripted sequence and the random life are the parent's own
functions, run with this driver in LiveLife's place."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import test_gpu_table_live_fuzz as LF
from test_gpu_table_ctid_fuzz import RING_CAPS, Q, assert_same_ranks, lists_csr, tid_array
from test_table_model import SEEDS_LIVE

pytestmark = pytest.mark.gpu


def words_of(mask):
    padded = np.zeros((len(mask) + 63) // 64 * 64, bool)
    padded[:len(mask)] = mask
    return np.packbits(padded, bitorder="little").view(np.uint64)


class DeleteLife(LF.LiveLife):
    made = []

    def __init__(self, *args, **kwargs):
        self.n_left_out = self.n_mirrored = self.n_by_index = 0
        self.reused = set()   # (the dead index a ctid named before, the live index it names now)
        DeleteLife.made.append(self)
        super().__init__(*args, **kwargs)

    def flags(self):
        return np.r_[np.asarray(self.m.sealed_deleted, bool), np.asarray(self.m.growing_deleted, bool)]

    def assert_dead(self, what):
        want = self.flags()
        assert self.dlive.n_docs == len(want), what
        assert np.array_equal(self.dlive.read_dead(), words_of(want)) and self.dlive.dead_docs == int(want.sum()), f"{what}: the deletion bitmap"

    def attach(self):
        super().attach()
        self.dlive = self.gix.bind()
        held = self.dlive.device_bytes()
        if len(self.m.sealed):
            self.ring_d = self.dlive.reranker(self.resolver, 3, **RING_CAPS, from_index=True)
            self.scorer_d = self.dlive.scorer()
        else:
            self.ring_d = self.scorer_d = None
        # what a restart does: the rows that are dead already die by index
        gone = np.flatnonzero(self.flags()[:self.dlive.n_docs])
        assert self.dlive.delete(gone) == len(gone)
        self.n_by_index += len(gone)
        assert (self.dlive.device_bytes() == held) == (len(gone) == 0)

    def keep(self, cast):
        super().keep(cast)
        self.dlive.append_documents(cast, self.resolver)

    def mirror(self, tids, want):
        """`tids` to the live handle; `want`: the flags they leave behind"""
        before = self.dlive.dead_docs
        made = self.ring_d.allocations() if self.ring_d is not None else None
        with vb.TidSet(tid_array(tids)) as ts:
            assert self.dlive.delete_tids(ts) == int(want.sum()) - before, f"epoch {self.epoch}: the rows that were alive"
        assert made is None or self.ring_d.allocations() == made, f"epoch {self.epoch}: a delete moved the ring's allocations"
        assert np.array_equal(self.dlive.read_dead(), words_of(want)) and self.dlive.dead_docs == int(want.sum()), f"epoch {self.epoch}: the deletion bitmap"
        self.n_mirrored += 1

    def delete_tids(self, tids):
        out = super().delete_tids(tids)
        self.mirror(tids, self.flags())
        return out

    def vacuum(self, tids=()):
        named = {tuple(int(x) for x in t) for t in tids}
        rows = list(self.m.sealed) + list(self.m.growing)
        self.mirror(tids, self.flags() | np.array([tuple(int(x) for x in p) in named for p, _, _ in rows], bool))
        old = (self.dlive, self.ring_d, self.scorer_d)
        super().vacuum(tids)
        del old

    def score(self, qkeys, i):
        """the model's _row_score of live row i, kept for the rerank at hand: its three results ask for the same pairs"""
        at = (qkeys, i)
        if at not in self.scores:
            self.scores[at] = self.m._row_score(self.m.live_row(i), qkeys)
        return self.scores[at]

    def dead_out(self, queries, lists, k, dead, covered):
        """the model's live side over its first `covered` rows with the dead rows left out -> (ranks [nq, k], n_ranks)"""
        m = self.m
        where = {}
        for i in range(covered):
            if not dead[i]:
                where.setdefault(tuple(int(x) for x in m.live_row(i)[0]), i)
        got = []
        for keys, tids in zip(queries, lists):
            qkeys = tuple(key for key in sorted(set(keys)) if key in m.rank)
            entries = []
            for pos, tid in enumerate(tids):
                tid = tuple(int(x) for x in tid)
                i, first = where.get(tid), m.live_index(tid, covered)
                if i is not None:
                    entries.append((self.score(qkeys, i), pos, i))
                if first is not None and first != i:
                    self.n_left_out += 1
                    if i is not None:
                        self.reused.add((first, i))
            got.append(m._top(entries, k))
        return np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.uint32)

    def rerank(self, queries, lists, k, count=True):
        m, ring = self.m, self.ring_d
        queries = [q if isinstance(q, Q) else Q(m, q) for q in queries]
        if ring is None:
            return super().rerank(queries, lists, k, count)
        what = f"epoch {self.epoch} rerank k={k}"
        self.scores = {}
        self.assert_dead(what)
        q_cand, cand_tid = lists_csr(lists)
        lexemes = [q.lexemes for q in queries]
        covered, n_rows = ring.directory_docs, self.dlive.n_docs
        if covered != n_rows:
            ring.submit(lexemes, k, q_cand, cand_tid=cand_tid)   # A: against the old directory
            ring.sync()
        ring.submit(lexemes, k, q_cand, cand_tid=cand_tid)       # B
        want = super().rerank(queries, lists, k, count)          # (LiveLife's own assertions, on the handle nobody deletes from)
        assert want["live_covered"] == covered
        dead = self.flags()
        if covered != n_rows:
            assert_same_ranks(ring.collect(), self.dead_out(queries, lists, k, dead, covered), f"{what}, the dead left out, before the sync")
        assert_same_ranks(ring.collect(), self.dead_out(queries, lists, k, dead, n_rows), f"{what}, the dead left out")
        # by index: the model's eligible candidates, dead ones among them
        by_doc = []
        for keys, docs in zip(queries, want["live_docs"]):
            qkeys = tuple(key for key in sorted(set(keys)) if key in m.rank)
            by_doc.append(m._top([(self.score(qkeys, int(i)), pos, int(i)) for pos, i in enumerate(docs) if not dead[int(i)]], k))
        by_doc = np.stack([g[0] for g in by_doc]), np.array([g[1] for g in by_doc], np.uint32)
        d_cand, cand_doc = LF.docs_csr(want["live_docs"])
        ring.submit(lexemes, k, d_cand, cand_doc=cand_doc)
        got = ring.collect()
        assert_same_ranks(got, by_doc, f"{what}, the dead left out, by index")
        terms, off = self.csr(self.gix, queries)
        top = self.scorer_d.topk(terms, off, k, d_cand, cand_doc)
        assert top[0].tobytes() == got[0].tobytes() and top[1].tobytes() == got[1].tobytes(), f"{what}: the scorer made at attach and the ring"
        return want


@pytest.fixture
def lives(monkeypatch):
    monkeypatch.setattr(LF, "LiveLife", DeleteLife)
    DeleteLife.made = []
    yield DeleteLife.made
    DeleteLife.made = []


def test_scripted_corners_with_the_deletes_mirrored(lives):
    """the parent's scripted sequence: sealed rows that share a ctid die together; a sealed row is deleted and its ctid inserted again
    -- sealed row 7, then growing row 5, document 705 -- and the live ring names THE NEW ROW; bulkdeletes of pairs, of nothing, of
    absent ctids, of everything"""
    LF.test_scripted_live_corners()
    life, = lives
    assert (7, 705) in life.reused, sorted(life.reused)
    assert life.n_left_out > 0 and life.n_mirrored >= 6


def test_random_life_with_the_deletes_mirrored(lives):
    LF.test_random_life_live(SEEDS_LIVE[0], {})
    life, = lives
    assert life.n_mirrored > 0 and life.n_left_out > 0, (life.n_mirrored, life.n_left_out, life.n_by_index)
