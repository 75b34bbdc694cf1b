"""scan_win_kernel's list of second arrivals -- a lane's first two flags appended in one step, the entry as the staged posting's byte
offset; and the threshold a window polls from its query's shared word, at items of every parity -- every record and every count
against the oracle's brute force, bit for bit.  -m gpu only.

One index of six windows of 2^16 documents (the last one partial), every query cut into items of ONE, TWO and THREE windows by the
skewed layout with the cut fractions 0.170 / 0.500.  The postings are explicit, so that a test decides which lane holds which flag:

  * a window has 320 SLOTS of 200 documents; a term holds one document per slot over a range of slots, so that its posting p of the
    window lies in slot first + p whatever the document is.  Every run is a multiple of four postings long: the runs start aligned to
    their loads, lane l holds the postings 4 l .. 4 l + 3 of a window's run, nobody marks a phantom, and the number of second arrivals
    of a window is exactly the number of flags the test sets;
  * the first term of a query (A) holds the slot's document 0; a later term i holds the slot's document 10 + i -- nobody else's --
    unless the test FLAGS its posting: then it holds A's document, finds A's bit in the filter and is a second arrival.  A flag is
    (term of the query, lane, posting of the lane);
  * flagged documents have term frequencies of 6 .. 9 in both lists, the others 1 or 2: the documents the list is about are the best
    ones, so an entry that is lost or reads the wrong posting changes the records.

A batch of four queries hands its lists over through the LDS, a batch of one through memory: both are asserted; k = 1, 10, 64."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import token_keys
from parity import assert_bit_exact

pytestmark = pytest.mark.gpu
WIN = 65536
N_WIN = 6
SLOTS, SLOT, BASE = 320, 200, 100
N_DOCS = (N_WIN - 1) * WIN + BASE + SLOT * SLOTS + 100
CUT1, CUT2 = 170, 500  # per mille of the index's windows
ITEMS = ((0, 1), (1, 3), (3, 6))
RUN = 256              # postings per term and window: one load per lane
THICK = 320            # ... of a thick run: a chunk of 64 postings behind the staged ones
LIST = 64              # the entries a window's list holds
KS = (1, 10, 64)


class Row:
    """one query: `nterms` terms of consecutive ids; flags(w) -> {(term, lane, j)} its flags in window w.  a0: A's first slot;
    thick = (term, windows): the term's runs of THICK postings (A then holds the slots 64 .. 319 there: a chunk's posting can be flagged)"""

    def __init__(self, nterms, flags, a0=0, thick=None):
        self.nterms, self.flags, self.a0, self.thick = nterms, flags, a0, thick
        self.terms = None
        self.nd = [len(flags(w)) for w in range(N_WIN)]

    def is_thick(self, w):
        return self.thick is not None and w in self.thick[1]

    def postings(self, i, rng):
        docs, tfs = [], []
        for w in range(N_WIN):
            fl = self.flags(w)
            assert all(1 <= t < self.nterms and 0 <= l < THICK // 4 and 0 <= j < 4 for t, l, j in fl)
            a_first = 64 if self.is_thick(w) else self.a0
            flagged = {4 * l + j for t, l, j in fl}                 # slots with a flag: A's postings there are hot too
            mine = {4 * l + j for t, l, j in fl if t == i}
            if i == 0:
                first, n = a_first, RUN
            else:
                first, n = 0, THICK if self.is_thick(w) and self.thick[0] == i else RUN
            assert all(s < n for s in mine) and all(a_first <= s < a_first + RUN for s in flagged), "a flag outside the runs"
            for p in range(n):
                s = first + p
                own = i != 0 and s not in mine
                docs.append(w * WIN + BASE + SLOT * s + (10 + i if own else 0))
                hot = s in mine if i else s in flagged
                tfs.append(int(rng.integers(6, 10)) if hot else int(rng.integers(1, 3)))
        return np.asarray(docs, dtype=np.int64), np.asarray(tfs, dtype=np.uint32)


def _spread(n, seed, nterms=5, lanes=(0, 64)):
    """n distinct flags over the terms 1 .. nterms - 1"""
    rng = np.random.default_rng(seed)
    every = [(t, l, j) for t in range(1, nterms) for l in range(*lanes) for j in range(4)]
    return {every[i] for i in rng.choice(len(every), n, replace=False)}


def two_flags(r):
    """lane L: all four postings of term 1 and one of term 3; L - 1 and L + 1 one flag each, L - 2 none, L + 2 two (two terms); lane 0
    two flags with nobody below it, lane 63 two flags of one term with everybody below it"""
    def flags(w):
        L = (5 + 11 * w + 17 * r) % 58 + 2
        return ({(1, L, j) for j in range(4)} | {(3, L, 1), (2, L - 1, 2), (4, L + 1, 0), (1, L + 2, 0), (2, L + 2, 3)} |
                {(1, 0, 3), (2, 0, 0), (3, 63, 1), (3, 63, 2)})
    return Row(5, flags)


def three_and_more(r):
    """lane a: three flags (three terms); lane b: eight (two terms, all four postings); a + 1 two flags, b + 1 one"""
    def flags(w):
        a, b = (3 + 7 * w + 13 * r) % 30, 32 + (5 * w + r) % 30
        return ({(1, a, 0), (2, a, 2), (4, a, 3), (3, a + 1, 1), (4, a + 1, 1), (1, b + 1, 2)} |
                {(t, b, j) for t in (2, 3) for j in range(4)})
    return Row(5, flags)


def cap(n_of_window):
    """exactly n second arrivals: one per lane (posting and term by the lane's number) up to 64, the 65th a second flag of lane 10"""
    def flags(w):
        n = n_of_window(w)
        fl = {(1 + l % 4, l, l % 4) for l in range(min(n, 64))}
        if n == 65:
            fl.add((1, 10, 0))
        assert len(fl) == n
        return fl
    return Row(5, flags)


def both_groups(nterms, r):
    """flags in the terms 1 and 3 (group 0) and 5 .. 7 (group 1), two of a lane in different groups; fewer entries than a completion
    pass holds (8 with eight terms, 10 with six).  A holds the slots from 8 on: an entry of term 5 that named term 0's posting (the group
    left out of the offset) would read another document"""
    def flags(w):
        La, Lb, Lc = 2 + (7 * w + 5 * r) % 20, 25 + (3 * w + r) % 20, 47 + (w + r) % 15
        fl = {(1, La, 0), (3, La, 2), (5, La, 1), (5, Lb, 3)}
        if nterms == 8:
            fl |= {(6, La, 0), (7, Lc, 0), (7, Lc, 1)}
        return fl
    return Row(nterms, flags, a0=8)


THICK_WINDOWS = (0, 2, 4)  # one in every item


def chunks(nterms, r):
    """the term in the middle is thick in one window of every item: flags in its chunk (a lane with one, with two and with all four: id
    entries) and in its staged part and in the other terms (offset entries) of the same window"""
    T = nterms // 2
    def flags(w):
        c = 64 + (3 * w + r) % 10  # (the chunk's lanes: 64 .. 79)
        fl = {(T, 20 + r, 1), (T, 20 + r, 2), (T, 40, 0), (nterms - 1, 30 + w, 3), (nterms - 1, 50, 0)}
        if w in THICK_WINDOWS:
            fl |= {(T, c, 2), (T, c + 1, 0), (T, c + 1, 3)} | {(T, c + 3, j) for j in range(4)}
        return fl
    return Row(nterms, flags, thick=(T, THICK_WINDOWS))


def passes(n, r):
    """n second arrivals a window with five terms (12 entries a pass): 13 the second open pass, 24 two full ones, 25 and 30 the overflow"""
    return Row(5, lambda w: _spread(n, 1000 * r + w))


def poll(windows, r):
    """the flagged (best) documents in the given windows only"""
    return Row(5, lambda w: _spread(10, 2000 * r + w) if w in windows else set())


CASES = {
    "two flags in a lane": [two_flags(r) for r in range(4)],
    "three and more flags in a lane": [three_and_more(r) for r in range(4)],
    # (the 65-entry window: in the three-window item, and as the one-window item)
    "list length at the cap": [cap(lambda w: 63), cap(lambda w: 64), cap(lambda w: 65 if w == 4 else 64), cap(lambda w: 65 if w == 0 else 63)],
    # (the queries of a batch have the same number of terms: a batch of unequal queries is sorted by length and hands over through memory)
    "both groups, eight terms": [both_groups(8, r) for r in range(4)],
    "both groups, six terms": [both_groups(6, 4 + r) for r in range(4)],
    "chunk entries mixed in, five terms": [chunks(5, r) for r in range(4)],
    "chunk entries mixed in, three terms": [chunks(3, 4 + r) for r in range(4)],
    "more than one pass": [passes(13, 0), passes(24, 1), passes(25, 2), passes(30, 3)],
    # (the best documents all in the item of three windows, of one, of two: the siblings hear of them through the shared word only)
    "poll parity": [poll((3, 4, 5), 0), poll((0,), 1), poll((1, 2), 2), poll(range(N_WIN), 3)],
}
GIVEN_UP = {"list length at the cap": (0, 0, 1, 1)}  # items given up per query: the ones whose window has 65 entries


class World:
    def __init__(self):
        assert tuple(N_WIN * c // 1000 for c in (0, CUT1, CUT2, 1000)) == (0, 1, 3, 6)
        rng = np.random.default_rng(20262)
        docs, tfs = [], []
        for rows in CASES.values():
            for row in rows:
                row.terms = np.arange(len(docs), len(docs) + row.nterms, dtype=np.uint32)
                for i in range(row.nterms):
                    d, t = row.postings(i, rng)
                    assert (np.diff(d) > 0).all() and len(d) % 4 == 0
                    docs.append(d)
                    tfs.append(t)
        dfs = np.array([len(d) for d in docs])
        keys, _ = token_keys(len(dfs))  # (term id = rank of its key)
        post_doc = np.concatenate(docs).astype(np.uint32)
        post_tf = np.concatenate(tfs)
        assert post_doc.max() < N_DOCS
        lens = np.bincount(post_doc, weights=post_tf, minlength=N_DOCS).astype(np.int64) + rng.integers(5, 60, N_DOCS)
        payload = rng.integers(0, 65536, (N_DOCS, 3)).astype(np.uint16)
        seg = vb.Segment.build(1.2, 0.75, lens.astype(np.uint32), payload, keys, np.r_[0, np.cumsum(dfs)].astype(np.uint64), post_doc, post_tf)
        self.gix = vb.GpuIndex(seg)
        self.oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
        self._ref = {}

    def ref(self, terms, off, k):
        key = (terms.tobytes(), off.tobytes(), k)
        if key not in self._ref:
            self._ref[key] = self.oix.search_batch(terms, off, k, mode="brute", threads=4)[:2]
        return self._ref[key]


@pytest.fixture(scope="module")
def world():
    return World()


def _run(tuning, W, rows, given_up, k, what):
    """the rows as one batch: four queries hand their lists over through the LDS, one through memory.  given_up: the items of the batch
    that have a window of more than LIST second arrivals -- asserted either way, so that the fallback cannot hide a wrong list"""
    nq = len(rows)
    tuning(win_force=1, fused=0, dense_x1000=10 ** 9, win_items=3 * nq, win_cut1=CUT1, win_cut2=CUT2)
    terms = np.concatenate([r.terms for r in rows]).astype(np.uint32)
    off = np.r_[0, np.cumsum([r.nterms for r in rows])].astype(np.uint32)
    b = vb.Batch(W.gix, nq, len(terms), k)
    b.set_queries(terms, off)
    assert b.debug_route() == 3, f"{what}: route {b.debug_route()}"
    b.run()
    assert b.debug_win_launches() == 1
    assert b.debug_win_handover() == (2 if nq >= 4 else 1), f"{what} nq {nq}: hand-over {b.debug_win_handover()}"
    hits, nh = b.fetch()
    items, failed = b.debug_counts()
    assert items == 3 * nq, f"{what} nq {nq}: {items} items"
    assert failed == given_up, f"{what} nq {nq}: {failed} items given up, want {given_up}"
    # (an item given up: fetch has run the batch again with scan_many_kernel and merge_kernel behind the window kernel)
    assert b.debug_win_launches() == (3 if given_up else 1), f"{what} nq {nq}: {b.debug_win_launches()} launches"
    ref, nref = W.ref(terms, off, k)
    for q in range(nq):
        assert nh[q] == nref[q], f"{what} nq {nq} q{q}: {nh[q]} hits, want {nref[q]}"
        assert_bit_exact(ref[q, :nref[q]], hits[q, :nh[q]], what=f"{what} nq {nq} q{q}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", list(CASES))
def test_list_of_second_arrivals(tuning, world, case, k):
    rows = CASES[case]
    gu = GIVEN_UP.get(case, (0, 0, 0, 0))
    for row, g in zip(rows, gu):  # (the test's own construction: the entries of every window, and which items go beyond the list)
        assert g == sum(any(row.nd[w] > LIST for w in range(lo, hi)) for lo, hi in ITEMS)
    if case == "list length at the cap":
        assert [max(r.nd) for r in rows] == [63, 64, 65, 65] and [min(r.nd) for r in rows] == [63, 64, 64, 63]
    if case == "more than one pass":
        assert [r.nd[0] for r in rows] == [13, 24, 25, 30]
    _run(tuning, world, rows, sum(gu), k, f"{case} k {k}")
    for row, g in zip(rows, gu):
        _run(tuning, world, [row], g, k, f"{case} k {k}")
