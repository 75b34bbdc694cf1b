"""scan_win_kernel's window boundaries -- the run lengths a wave keeps per lane, the boundary table in its LDS, the row sum's shift with
zero fill -- at the edges of an item, every record against the oracle's brute force, bit for bit.  -m gpu only.

One index of 126 windows of 2^16 documents, the last of them partial (3 000 documents).  Every query is cut into three items by the
skewed layout with the cut fractions 0.500 / 0.993: 63 windows (the most an item holds: its boundaries fill lanes 0 .. 63), 62
windows, and ONE window -- the index's last, partial one.  Every window has a pool of 2 000 documents its postings are drawn from, so
that the terms of a query share documents (second arrivals, whose completion reads the boundaries) in every window:

  * groups of terms with 200, 80, 66 and 50 postings per window: queries of 2, 5, 6 and 8 terms of their group have about 400
    postings per window each -- the batches keep the caller's order (the arithmetic layout: lists handed over through the LDS) also
    where queries of two and of five terms are mixed (null terms in the kernel compiled for five);
  * two terms whose run in window i has i mod 7 and (i + 3) mod 5 postings: empty runs (also in an item's first and last window)
    and runs starting at every alignment 0 .. 3 inside their first load;
  * a term with 300 postings (more than the 256 one load per lane stages) in the first, a middle and the last window of the 63- and
    of the 62-window item and in the single-window item, 40 elsewhere.

Five and six terms take the table and the lengths, eight terms neither (the selects and both boundaries, as before); k = 1, 10, 64.
A batch of four queries hands its lists over through the LDS, a batch of one through memory: both are asserted."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import token_keys
from parity import assert_bit_exact

pytestmark = pytest.mark.gpu
WIN = 65536
N_WIN = 126
N_DOCS = (N_WIN - 1) * WIN + 3000
POOL = 2000
CUT1, CUT2 = 500, 993  # per mille of the index's windows
ITEMS = (63, 62, 1)
THICK_AT = (0, 30, 62, 63, 90, 124, 125)  # first, middle, last window of the items [0, 63) and [63, 125); the item [125, 126)
GROUPS = {2: (8, 200), 5: (12, 80), 6: (8, 66), 8: (8, 50)}  # query length -> (terms of the group, postings per window)
KS = (1, 10, 64)


class World:
    def __init__(self):
        assert N_WIN * CUT1 // 1000 == ITEMS[0] and N_WIN * CUT2 // 1000 - ITEMS[0] == ITEMS[1] and N_WIN - N_WIN * CUT2 // 1000 == ITEMS[2]
        rng = np.random.default_rng(20261)
        pools = []
        for w in range(N_WIN):
            lo, hi = w * WIN, min((w + 1) * WIN, N_DOCS)
            pools.append(lo + rng.choice(hi - lo, POOL, replace=False))
        docs = []

        def add(counts):
            docs.append(np.sort(np.concatenate([rng.choice(pools[w], int(c), replace=False) for w, c in enumerate(counts)])))
            return len(docs) - 1

        self.group = {n: [add([per] * N_WIN) for _ in range(cnt)] for n, (cnt, per) in GROUPS.items()}
        self.x1 = add([w % 7 for w in range(N_WIN)])
        self.x2 = add([(w + 3) % 5 for w in range(N_WIN)])
        self.thick = add([300 if w in THICK_AT else 40 for w in range(N_WIN)])
        self.docs = docs
        dfs = np.array([len(d) for d in docs])
        keys, _ = token_keys(len(dfs))  # (term id = rank of its key)
        post_doc = np.concatenate(docs).astype(np.uint32)
        post_tf = rng.integers(1, 6, len(post_doc)).astype(np.uint32)
        lens = np.bincount(post_doc, weights=post_tf, minlength=N_DOCS).astype(np.int64) + rng.integers(5, 60, N_DOCS)
        payload = rng.integers(0, 65536, (N_DOCS, 3)).astype(np.uint16)
        seg = vb.Segment.build(1.2, 0.75, lens.astype(np.uint32), payload, keys, np.r_[0, np.cumsum(dfs)].astype(np.uint64), post_doc, post_tf)
        self.gix = vb.GpuIndex(seg)
        self.oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
        self._ref = {}

    def bounds(self, t):
        """term t's postings below every window boundary (the kernel's wo[t])"""
        return np.searchsorted(self.docs[t], np.arange(N_WIN + 1, dtype=np.int64) * WIN)

    def ref(self, terms, off, k):
        key = (terms.tobytes(), off.tobytes(), k)
        if key not in self._ref:
            self._ref[key] = self.oix.search_batch(terms, off, k, mode="brute", threads=4)[:2]
        return self._ref[key]


@pytest.fixture(scope="module")
def world():
    return World()


def _check(tuning, W, rows, k, what):
    """the queries `rows` as one batch of four (through the LDS) and one by one (through memory)"""
    assert len(rows) == 4
    _run(tuning, W, [rows] + [[r] for r in rows], k, what)


def _run(tuning, W, batches, k, what):
    """every batch in one launch: four queries and more hand their lists over through the LDS, fewer through memory"""
    for batch in batches:
        nq = len(batch)
        # (one item of about a third of the windows per resident wave: three items per query, the skewed layout with the cuts above)
        tuning(win_force=1, fused=0, dense_x1000=10 ** 9, win_items=3 * nq, win_cut1=CUT1, win_cut2=CUT2)
        terms = np.concatenate([np.sort(np.asarray(r)) for r in batch]).astype(np.uint32)
        off = np.r_[0, np.cumsum([len(r) for r in batch])].astype(np.uint32)
        b = vb.Batch(W.gix, nq, len(terms), k)
        b.set_queries(terms, off)
        assert b.debug_route() == 3, f"{what}: route {b.debug_route()}"
        b.run()
        assert b.debug_win_launches() == 1
        assert b.debug_win_handover() == (2 if nq >= 4 else 1), f"{what} nq {nq}: hand-over {b.debug_win_handover()}"
        hits, nh = b.fetch()
        items, failed = b.debug_counts()
        assert items == 3 * nq, f"{what} nq {nq}: {items} items"
        assert failed == 0, f"{what} nq {nq}: an item was given up"
        ref, nref = W.ref(terms, off, k)
        for q in range(nq):
            assert nh[q] == nref[q], f"{what} nq {nq} q{q}: {nh[q]} hits, want {nref[q]}"
            assert_bit_exact(ref[q, :nref[q]], hits[q, :nh[q]], what=f"{what} nq {nq} q{q}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mt", [2, 5, 6, 8])
def test_items_of_63_62_and_1_windows(tuning, world, mt, k):
    """every query of the batch with mt terms -- the kernel compiled for exactly that many run loads: with the table and the lengths
    (2, 5, 6) and without (8) -- over items of 63, 62 and 1 windows, the last one the index's partial window"""
    rng = np.random.default_rng(100 + mt)
    rows = [rng.choice(world.group[mt], mt, replace=False) for _ in range(4)]
    _check(tuning, world, rows, k, f"{mt} terms k {k}")


@pytest.mark.parametrize("k", KS)
def test_two_terms_in_a_batch_compiled_for_five(tuning, world, k):
    """null terms: their boundaries are the all-zero table's -- runs without postings -- in the lengths and in the LDS table alike"""
    rng = np.random.default_rng(7)
    g2, g5 = world.group[2], world.group[5]
    rows = [rng.choice(g5, 5, replace=False), rng.choice(g2, 2, replace=False), rng.choice(g5, 5, replace=False), rng.choice(g2, 2, replace=False)]
    _check(tuning, world, rows, k, f"2 in 5 k {k}")
    rows = [rng.choice(g2, 2, replace=False), rng.choice(g5, 5, replace=False), rng.choice(g5, 5, replace=False), rng.choice(g5, 5, replace=False)]
    _check(tuning, world, rows, k, f"2 first in 5 k {k}")
    _run(tuning, world, [rows[:2], rows[1::-1]], k, f"2 in 5 through memory k {k}")


@pytest.mark.parametrize("k", KS)
def test_empty_runs_and_every_alignment(tuning, world, k):
    """the terms x1, x2: empty runs and runs that start 0 .. 3 postings into their first aligned load, beside terms of 200 postings a window"""
    for x in (world.x1, world.x2):
        o = world.bounds(x)
        assert set(o[:-1] & 3) == {0, 1, 2, 3} and (np.diff(o) == 0).any()
        for lo, hi in ((0, 63), (63, 125)):  # an empty run in the item, and one as an item's first or last window
            assert (np.diff(o)[lo:hi] == 0).any()
    # (x1: nothing in the first window of the 63- and of the 62-window item; x2: nothing in the last window of the 63-window item)
    assert np.diff(world.bounds(world.x1))[[0, 63]].tolist() == [0, 0] and np.diff(world.bounds(world.x2))[62] == 0
    g2 = world.group[2]
    _check(tuning, world, [[world.x1, g2[j]] for j in range(4)], k, f"x1 k {k}")
    _check(tuning, world, [[world.x1, world.x2, g2[4 + j]] for j in range(4)], k, f"x1 x2 k {k}")


@pytest.mark.parametrize("k", KS)
def test_thick_runs_at_the_ends_and_the_middle_of_an_item(tuning, world, k):
    """more than 256 postings of a term in an item's first, a middle and its last window: the part behind the staged run is marked by the
    chunk loop, which reads both boundaries, and its second arrivals are found in memory"""
    n = np.diff(world.bounds(world.thick))
    assert (n[list(THICK_AT)] > 256).all() and (np.delete(n, THICK_AT) <= 64).all()
    g2 = world.group[2]
    _check(tuning, world, [[world.thick, g2[j]] for j in range(4)], k, f"thick k {k}")
    _check(tuning, world, [[world.thick, world.x1, g2[4 + j]] for j in range(4)], k, f"thick x1 k {k}")
