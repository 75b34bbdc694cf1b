"""scan_win_kernel's completion at the edges of its search and of its row sum, every record against the oracle's brute force, bit for
bit.  -m gpu only.

The search (c1_search): a second arrival's document x is looked for in every term's staged run of the window in eight steps; what
lies behind the run in its stage row -- the next window's ids, unsorted relative to the run -- must never decide a step.  The cases
put a run of exactly L postings into the middle one of three windows -- L around every power of two the steps halve to -- with x on the
run's first, second, middle, last-but-one and last posting, below the first, above the last and between two of them, and 0 .. 3
postings of the term in the window before, so that the run starts at every offset inside its first aligned load.  Runs thicker than
a stage row (the rest is searched in memory) have x inside the staged part, on its last posting, on the first posting behind it
and deep in the rest.  (A build whose search probed past the run's end failed the first of these cases.)

The row sum (c2_sum): lane = (entry, term), a row's MT values are added at the row's first lane after MT - 1 wave shifts; what is
shifted in at lane 63 must never reach a row's first lane.  With 2, 4 and 8 terms the last row of a pass ends at lane 63: the cases
fill a pass -- 32, 16, 8 entries -- and put a document with postings in ALL of the query's terms into its last row.  Five terms: 12
rows, lanes 60 .. 63 idle.

Corpora of 190 000 documents are three windows, one item each (tests/test_gpu_win_lds_merge.py): a batch of one query hands its
lists over through memory, a batch of four through the LDS.  Both are asserted."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import token_keys
from parity import assert_bit_exact

pytestmark = pytest.mark.gpu
N_DOCS = 190_000  # three windows of 2^16 documents
WIN = 65536
K = 10
SEARCH_L = (1, 2, 3, 4, 5, 127, 128, 129, 255, 256)
THICK_L = (257, 300, 600)
PAD = 30  # postings of the partner terms in the last window: the four queries of a batch stay within a quarter of each other's length


class Terms:
    """a corpus written term by term: add(docs, tfs) returns the term's id"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.docs, self.tfs = [], []

    def add(self, docs, tfs=None):
        docs = np.asarray(docs, dtype=np.int64)
        order = np.argsort(docs)
        assert len(docs) and len(np.unique(docs)) == len(docs) and docs.min() >= 0 and docs.max() < N_DOCS
        tfs = self.rng.integers(1, 6, len(docs)) if tfs is None else np.asarray(tfs, dtype=np.int64)
        self.docs.append(docs[order])
        self.tfs.append(tfs[order])
        return len(self.docs) - 1

    def pad(self):
        """PAD documents of the last window"""
        return 2 * WIN + self.rng.choice(N_DOCS - 2 * WIN, PAD, replace=False)

    def build(self):
        dfs = np.array([len(d) for d in self.docs])
        keys, _ = token_keys(len(dfs))  # (term id = rank of its key)
        post_doc = np.concatenate(self.docs).astype(np.uint32)
        post_tf = np.concatenate(self.tfs).astype(np.uint32)
        lens = np.bincount(post_doc, weights=post_tf, minlength=N_DOCS).astype(np.int64) + self.rng.integers(5, 60, N_DOCS)
        payload = self.rng.integers(0, 65536, (N_DOCS, 3)).astype(np.uint16)
        seg = vb.Segment.build(1.2, 0.75, lens.astype(np.uint32), payload, keys, np.r_[0, np.cumsum(dfs)].astype(np.uint64), post_doc, post_tf)
        return vb.GpuIndex(seg), orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())


def _run_case(T, L, prev, shared_at, between_at):
    """Term A: `prev` postings in the first window, a run of L in the middle one (ids at least 3 apart), nothing behind it.  Term B:
    A's postings `shared_at`, the documents right below A's first and right above A's last, and one right behind A's posting
    `between_at`.  Term C shares B's three documents that A lacks -- as second arrivals they are searched for in A's run and not
    found: below it, above it, between two of its postings -- and A's posting shared_at[len // 2].  Returns (A, B, C)."""
    rng = T.rng
    run = WIN + 1000 + np.cumsum(rng.integers(3, 60000 // max(L, 20), L))
    assert run[-1] < 2 * WIN - 2
    before = rng.choice(np.arange(100, WIN - 100), prev, replace=False)
    a = T.add(np.r_[before, run])
    shared = sorted({min(max(i if i >= 0 else L + i, 0), L - 1) for i in shared_at})
    outside = [run[0] - 1, run[-1] + 1, run[min(between_at, L - 1)] + 1]
    outside = sorted(set(int(d) for d in outside) - set(int(d) for d in run))
    b_docs = np.r_[run[shared], outside, T.pad()]
    # (the shared documents with the larger term frequencies: they are the query's best, a wrong posting changes a record)
    b = T.add(b_docs, np.r_[rng.integers(3, 6, len(shared)), rng.integers(1, 4, len(outside)), np.ones(PAD, np.int64)])
    c_docs = np.r_[outside, [run[shared[len(shared) // 2]]], T.pad()]
    c = T.add(c_docs, np.r_[rng.integers(2, 6, len(outside) + 1), np.ones(PAD, np.int64)])
    return a, b, c


def _row_case(T, mt, n, n_all, sparse):
    """A query of mt terms with n second-arrival documents in the middle window, laid out alike in every run (no posting of any term
    in the window before: the runs start aligned).  sparse: the documents in the terms 0 and 1 only, but the LAST n_all of them in
    every term -- the marks list the n entries of term 1 first, lane after lane: one row each in the first pass, the last rows
    the documents with every term.  Not sparse: all n in every term (mt - 1 entries each, pass after pass full of complete rows)."""
    rng = T.rng
    docs = WIN + 500 + np.cumsum(rng.integers(2, 1500, n))
    terms = []
    for t in range(mt):
        mine = docs if (t < 2 or not sparse) else docs[n - n_all:]
        terms.append(T.add(np.r_[mine, T.pad()], np.r_[rng.integers(1, 6, len(mine)), np.ones(PAD, np.int64)]))
    return terms


@pytest.fixture(scope="module")
def world():
    T = Terms(seed=20240)
    cases = {}
    for L in SEARCH_L:
        for prev in range(4):
            cases["search", L, prev] = _run_case(T, L, prev, shared_at=(0, 1, L // 2, -2, -1), between_at=L // 3)
    for L in THICK_L:
        for prev in range(4):
            # inside the staged part, around posting 256 (the staged part ends at 256 - prev), in the part searched in memory; the
            # document C shares with B behind A's posting 270 lies in that part too
            cases["thick", L, prev] = _run_case(T, L, prev, shared_at=(0, 10, 200, 252, 253, 254, 255, 256, 270, -2, -1), between_at=270)
    for mt, n in ((2, 32), (4, 16), (8, 8), (5, 12)):
        for v in range(4):
            cases["rows", mt, "sparse", v] = _row_case(T, mt, n, n_all=1 + v % 2, sparse=True)
            # (all n documents in all 8 terms would be 56 entries, close to the 64 a window's list holds: half of them)
            cases["rows", mt, "full", v] = _row_case(T, mt, n if mt != 8 else 4, n_all=0, sparse=False)
    gix, oix = T.build()
    return gix, oix, cases


def _check(world, rows, what):
    """the queries `rows` as one batch of len(rows) queries (4: through the LDS) and one by one (through memory)"""
    gix, oix, _ = world
    for batch in [rows] + [[r] for r in rows]:
        terms = np.concatenate([np.sort(np.asarray(r)) for r in batch]).astype(np.uint32)
        off = np.r_[0, np.cumsum([len(r) for r in batch])].astype(np.uint32)
        nq = len(batch)
        b = vb.Batch(gix, nq, len(terms), K)
        b.set_queries(terms, off)
        assert b.debug_route() == 3, f"{what}: route {b.debug_route()}"
        b.run()
        assert b.debug_win_launches() == 1
        assert b.debug_win_handover() == (2 if nq >= 4 else 1), f"{what} nq {nq}: hand-over {b.debug_win_handover()}"
        hits, nh = b.fetch()
        assert b.debug_counts()[1] == 0, f"{what} nq {nq}: an item was given up"
        ref, nref, _ = oix.search_batch(terms, off, K, mode="brute", threads=4)
        for q in range(nq):
            assert nh[q] == nref[q], f"{what} nq {nq} q{q}: {nh[q]} hits, want {nref[q]}"
            assert_bit_exact(ref[q, :nref[q]], hits[q, :nh[q]], what=f"{what} nq {nq} q{q}")


@pytest.mark.parametrize("L", SEARCH_L)
def test_run_lengths_at_every_step_edge(tuning, world, L):
    """two-term queries (A, B) and three-term queries (A, B, C); the four queries of a batch are the run at its four alignments"""
    tuning(win_force=1, fused=0)
    cases = world[2]
    _check(world, [cases["search", L, prev][:2] for prev in range(4)], f"L {L} two terms")
    _check(world, [cases["search", L, prev] for prev in range(4)], f"L {L} three terms")


@pytest.mark.parametrize("L", THICK_L)
def test_runs_thicker_than_a_stage_row(tuning, world, L):
    """the search of the staged part ends on its last posting; whatever lies beyond is found in memory"""
    tuning(win_force=1, fused=0)
    cases = world[2]
    _check(world, [cases["thick", L, prev][:2] for prev in range(4)], f"thick L {L} two terms")
    _check(world, [cases["thick", L, prev] for prev in range(4)], f"thick L {L} three terms")


@pytest.mark.parametrize("mt", [2, 4, 8, 5])
def test_row_sums_up_to_the_last_lane(tuning, world, mt):
    """a full first pass whose last row holds a document with every term of the query; further passes behind it"""
    tuning(win_force=1, fused=0)
    cases = world[2]
    for kind in ("sparse", "full"):
        _check(world, [cases["rows", mt, kind, v] for v in range(4)], f"{mt} terms {kind}")
