"""scan_win_kernel's in-kernel merge when a query's three lists change hands inside the workgroup (through the LDS) and when they go
through memory, in one launch and side by side: every record against the oracle's brute force, bit for bit.  -m gpu only.

The layout decides the path (scan_win.h, the item end): a one-launch run in the arithmetic order (order_on == 2: three items per
query, queries of about equal length in the caller's order) keeps the queries 0 .. 4 (nq // 4) - 1 inside workgroups -- the LDS path
-- and sends the last nq mod 4 through memory.  Corpora of 190 000 documents are three windows: three items of one window per query
whatever nq is.  `debug_win_handover` says which form a run took; the tests assert it, so that a change of the routing cannot turn
them into tests of one path only."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries, token_keys
from parity import assert_bit_exact

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
N_DOCS = 190_000  # three windows of 2^16 documents
WIN = 65536
NQS = (1, 3, 4, 5, 8, 9)  # memory only (1, 3), LDS only (4, 8), both in one launch (5, 9)


def _corpus(groups, seed, constant=False, spread=None):
    """`groups`: (number of terms, df) -- every term of a group in exactly df documents, so that queries built from one term of
    each of n groups, or n terms of one group, have the same number of postings (the host keeps the caller's order -- the
    arithmetic layout -- only for queries within a quarter of each other).  constant: tf 1 and one length for every document (equal
    scores in masses).  spread[t]: the windows term t's documents are drawn from (default: all three).
    Returns the make_corpus dict; term ids are group after group, in order."""
    rng = np.random.default_rng(seed)
    dfs = np.concatenate([np.full(n, df) for n, df in groups])
    vocab = len(dfs)
    keys, rank = token_keys(vocab)
    # (term id = rank of its key: tokens are assigned so that token_of[t] has rank t)
    docs, tfs = [], []
    for t, df in enumerate(dfs):
        wins = (0, 1, 2) if spread is None or t not in spread else spread[t]
        pool = np.concatenate([np.arange(w * WIN, min((w + 1) * WIN, N_DOCS)) for w in wins])
        d = np.sort(rng.choice(pool, int(df), replace=False))
        docs.append(d)
        tfs.append(np.ones(len(d), np.int64) if constant else rng.integers(1, 6, len(d)))
    post_doc = np.concatenate(docs).astype(np.uint32)
    post_tf = np.concatenate(tfs).astype(np.uint32)
    term_start = np.r_[0, np.cumsum(dfs)].astype(np.uint64)
    if constant:
        lens = np.full(N_DOCS, 40, np.int64)
    else:
        lens = np.bincount(post_doc, weights=post_tf, minlength=N_DOCS).astype(np.int64) + rng.integers(5, 200, N_DOCS)
    payload = rng.integers(0, 65536, (N_DOCS, 3)).astype(np.uint16)
    return dict(n_docs=N_DOCS, doc_len=lens.astype(np.uint32), doc_payload=payload, term_key=keys, term_start=term_start,
                post_doc=post_doc, post_tf=post_tf, dfs=dfs)


class Built:
    def __init__(self, c):
        self.c = c
        self.seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
        self.gix = vb.GpuIndex(self.seg)
        self.oix = orc.OracleIndex.from_arrays(self.seg.meta(), self.seg.arrays())
        self._ref = {}

    def ref(self, terms, off, k):
        """the oracle's brute force for a query set, computed once per (queries, k)"""
        key = (terms.tobytes(), off.tobytes(), k)
        if key not in self._ref:
            self._ref[key] = self.oix.search_batch(terms, off, k, mode="brute", threads=8)[:2]
        return self._ref[key]


# V: scores of every kind.  Groups of 12 terms with df 750 / 500 / 375 / 300: a query of 2 / 3 / 4 / 5 terms of ONE group has 1500
# postings -- queries of two to five terms in one batch keep the arithmetic layout.  Runs of 100 .. 250 postings per window.
V_GROUPS = ((12, 750), (12, 500), (12, 375), (12, 300))
# R: rare terms, df 4 -- terms 0 .. 7 in all windows, 8 .. 15 in the windows 0 and 2 only (a middle item without a posting)
R_GROUPS = ((16, 4),)
# T: equal scores in masses -- 16 terms of df 600, tf 1, one document length
T_GROUPS = ((16, 600),)


@pytest.fixture(scope="module")
def V():
    return Built(_corpus(V_GROUPS, seed=1))


@pytest.fixture(scope="module")
def R():
    return Built(_corpus(R_GROUPS, seed=2, spread={t: (0, 2) for t in range(8, 16)}))


@pytest.fixture(scope="module")
def T():
    return Built(_corpus(T_GROUPS, seed=3, constant=True))


def _queries(rows):
    terms = np.concatenate([np.sort(np.asarray(r)) for r in rows]).astype(np.uint32)
    off = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint32)
    return terms, off


def _v_queries(nq, seed, nterms=None):
    """query q: n terms of the group of n-term queries (n = 2 + q mod 4, or nterms for all)"""
    rng = np.random.default_rng(seed)
    rows = []
    for q in range(nq):
        n = nterms or 2 + q % 4
        rows.append(12 * (n - 2) + rng.choice(12, n, replace=False))
    return _queries(rows)


def _expect_handover(nq, forced=None):
    return forced if forced is not None else (2 if nq >= 4 else 1)


def _run_and_check(B, terms, off, k, handover=None, doc_filter=None, sel=None, want=None, what=""):
    nq = len(off) - 1
    b = vb.Batch(B.gix, nq, max(1, len(terms)), k)
    b.set_queries(terms, off)
    assert b.debug_route() == 3, f"route {b.debug_route()}"
    if doc_filter is not None:
        b.set_filter(doc_filter, sel)
    b.run()
    assert b.debug_win_launches() == (1 if handover != 0 else 3)
    assert b.debug_win_handover() == _expect_handover(nq, handover), f"{what}: hand-over {b.debug_win_handover()}"
    hits, nh = b.fetch()
    assert b.debug_counts()[1] == 0, "an item was given up"
    if want is None:
        ob, onb = B.ref(terms, off, k)
        want = [ob[q, :onb[q]] for q in range(nq)]
    for q in range(nq):
        assert nh[q] == len(want[q]), f"{what} q{q}: {nh[q]} hits, want {len(want[q])}"
        assert_bit_exact(want[q], hits[q, :nh[q]], what=f"{what} q{q}")
    return b, hits, nh


@pytest.mark.parametrize("k", [1, 10, 64, 100, 256])
def test_every_nq_and_k_on_both_paths(tuning, V, k):
    """nq = 1, 3: memory only; 4, 8: LDS only; 5, 9: both in one launch.  k = 1 .. 256: one, two and four register rows; up to 64 the
    merge ranks by counting, beyond it through the register top-k.  Queries of two to five terms in one batch (null terms)."""
    tuning(win_force=1, fused=0)
    for nq in NQS:
        terms, off = _v_queries(nq, seed=10 + nq)
        _run_and_check(V, terms, off, k, what=f"nq {nq} k {k}")


@pytest.mark.parametrize("nterms", [2, 3, 4, 5])
def test_term_counts_of_their_own_instantiation(tuning, V, nterms):
    """every query of the batch with the same number of terms: the kernel compiled for exactly that many run loads"""
    tuning(win_force=1, fused=0)
    terms, off = _v_queries(9, seed=40 + nterms, nterms=nterms)
    _run_and_check(V, terms, off, 10, what=f"{nterms} terms")
    _run_and_check(V, terms, off, 100, what=f"{nterms} terms k 100")


def test_short_lists_and_an_empty_middle_item(tuning, R):
    """Two rare terms per query: eight postings, fewer than k = 10 hits in all; the queries of the terms 8 .. 15 have no posting in
    the middle window -- their middle item hands over an empty list."""
    tuning(win_force=1, fused=0)
    for nq in (3, 4, 5, 8):
        rows = [[q % 8, (q + 3) % 8] if q % 2 == 0 else [8 + q % 8, 8 + (q + 3) % 8] for q in range(nq)]
        terms, off = _queries(rows)
        _, hits, nh = _run_and_check(R, terms, off, 10, what=f"rare nq {nq}")
        assert (nh < 10).all() and (nh > 0).all()
        for q in range(1, nq, 2):
            assert not ((hits[q, :nh[q]]["doc_id"] >= WIN) & (hits[q, :nh[q]]["doc_id"] < 2 * WIN)).any()


@pytest.mark.parametrize("k", [10, 64, 100])
def test_more_than_64_entries_tie_at_the_threshold(tuning, T, k):
    """tf 1 and one document length: every document with one of a query's terms has the same score.  With k = 64 and 100 the three
    lists are full of them: far more than 64 entries at the final threshold -- the merge leaves the ranking by counting for the
    register top-k (ties by ascending document)."""
    tuning(win_force=1, fused=0)
    rng = np.random.default_rng(5)
    for nq in (3, 4, 5):
        terms, off = _queries([rng.choice(16, 3, replace=False) for _ in range(nq)])
        _, hits, nh = _run_and_check(T, terms, off, k, what=f"ties nq {nq} k {k}")
        if k >= 64:
            for q in range(nq):
                assert (hits[q, :nh[q]]["score"] == hits[q, nh[q] - 1]["score"]).sum() > 32, "the corpus is expected to tie in masses"


def test_document_filter_on_both_paths(tuning, V):
    """the FILT instantiation: filtered and unfiltered queries in one batch; the filtered answer is the oracle's full ranking with
    the rejected documents removed (every query matches fewer than 65535 documents)."""
    tuning(win_force=1, fused=0)
    k = 10
    ids = np.arange(N_DOCS)
    for nq in (3, 5, 8):
        terms, off = _v_queries(nq, seed=70 + nq)
        fulls = []
        for q in range(nq):
            f = V.oix.search_brute(terms[off[q]:off[q + 1]], 65535)
            assert len(f) < 65535
            fulls.append(f)
        keeps = np.stack([ids % 2 == 0, ids % 7 == 3])
        keeps[1, fulls[0]["doc_id"][:4 * k]] = False
        sel = np.array([[0, NONE, 1][q % 3] for q in range(nq)], dtype=np.uint32)
        want = [fulls[q][:k] if sel[q] == NONE else fulls[q][keeps[sel[q]][fulls[q]["doc_id"]]][:k] for q in range(nq)]
        f = vb.DocFilter(V.gix, keeps)
        b, hits, nh = _run_and_check(V, terms, off, k, doc_filter=f, sel=sel, want=want, what=f"filtered nq {nq}")
        b.run()
        h2, n2 = b.fetch()
        assert h2.tobytes() == hits.tobytes() and np.array_equal(n2, nh)


@pytest.mark.parametrize("nq", [3, 5, 8])
def test_state_is_left_for_the_next_launch(tuning, V, nq):
    """The same batch object three times in a row, and two batch objects (other queries, other k) alternating on one stream: the
    same records every time -- threshold words, counters and flags are as the next launch expects them on both paths."""
    tuning(win_force=1, fused=0)
    ta, oa = _v_queries(nq, seed=80 + nq)
    tb, ob = _v_queries(nq, seed=90 + nq)
    a, ha, na = _run_and_check(V, ta, oa, 10, what="a")
    for _ in range(2):
        a.run()
        assert a.debug_win_launches() == 1
        h, n = a.fetch()
        assert h.tobytes() == ha.tobytes() and np.array_equal(n, na)
    b, hb, nb = _run_and_check(V, tb, ob, 64, what="b")
    for _ in range(2):
        a.run()
        b.run()
        h, n = a.fetch()
        assert h.tobytes() == ha.tobytes() and np.array_equal(n, na)
        h, n = b.fetch()
        assert h.tobytes() == hb.tobytes() and np.array_equal(n, nb)
    # one object, another query set of another size: what the first left behind must not reach the second
    a.set_queries(tb, ob)
    a.run()
    h, n = a.fetch()
    rb, rnb = V.ref(tb, ob, 10)
    for q in range(nq):
        assert_bit_exact(rb[q, :rnb[q]], h[q, :n[q]], what=f"reused q{q}")


@pytest.fixture(scope="module")
def G():
    # the corpus of test_one_launch_merge_and_its_fallback at three windows: lists of about a thousand postings per window, more
    # second arrivals in a window than the list holds
    return Built(make_corpus(N_DOCS, 3000, seed=2, length="lognormal", mean_len=60))


@pytest.mark.parametrize("nq", [3, 5, 8])
def test_a_given_up_item_on_both_paths(tuning, G, nq):
    """Thick lists: items are given up.  The one-launch run marks the query (on the LDS path from the flag in the LDS, on the
    memory path from item_failed), fetch() re-runs the batch with scan_many_kernel and merge_kernel: the oracle's records for the
    affected queries and for the others, and the query set stays on the three-launch form."""
    tuning(win_force=1, fused=0, win_fuse=1)
    terms, off = make_queries(G.c, nq, 4, seed=9)
    b = vb.Batch(G.gix, nq, len(terms), 10)
    b.set_queries(terms, off)
    assert b.debug_route() == 3
    b.run()
    assert b.debug_win_launches() == 1 and b.debug_win_handover() == _expect_handover(nq)
    hits, nh = b.fetch()
    items, failed = b.debug_counts()
    assert failed > 0 and b.debug_win_launches() == 3, "this shape is expected to give items up"
    rb, rnb = G.ref(terms, off, 10)
    assert np.array_equal(nh, rnb)
    for q in range(nq):
        assert_bit_exact(rb[q, :rnb[q]], hits[q, :nh[q]], what=f"fallback q{q}")
    b.run()
    assert b.debug_win_launches() == 3
    h3, n3 = b.fetch()
    assert h3.tobytes() == hits.tobytes() and np.array_equal(n3, nh)
    # a fresh query set on the same object is tried in one launch again
    b.set_queries(terms, off)
    b.run()
    assert b.debug_win_launches() == 1
    h4, n4 = b.fetch()
    assert h4.tobytes() == hits.tobytes() and np.array_equal(n4, nh)


def test_one_given_up_query_among_others(tuning, V):
    """A term frequency above 255 in a second arrival gives ONE item up: that query comes back complete through fetch() and the
    others are what they were -- with the affected query inside a workgroup (LDS) and as the batch's last (memory)."""
    c = dict(V.c)
    tf = c["post_tf"].copy()
    lens = c["doc_len"].copy()
    # a document of the terms 0 and 1 (group of the two-term queries): one is made if there is none
    s = c["term_start"].astype(np.int64)
    d0, d1 = c["post_doc"][s[0]:s[1]], c["post_doc"][s[1]:s[2]]
    both = np.intersect1d(d0, d1)
    assert len(both), "the corpus is expected to hold a document with both terms"
    d = both[0]
    tf[s[0] + np.searchsorted(d0, d)] = 300
    lens[d] += 300
    c["post_tf"], c["doc_len"] = tf, lens
    B = Built(c)
    tuning(win_force=1, fused=0)
    for nq, at in ((8, 2), (5, 4)):
        terms, off = _v_queries(nq, seed=120 + nq, nterms=2)
        terms[off[at]:off[at] + 2] = (0, 1)
        b = vb.Batch(B.gix, nq, len(terms), 10)
        b.set_queries(terms, off)
        b.run()
        assert b.debug_win_launches() == 1 and b.debug_win_handover() == 2
        hits, nh = b.fetch()
        assert b.debug_counts()[1] == 1 and b.debug_win_launches() == 3, "exactly one item is expected to be given up"
        rb, rnb = B.ref(terms, off, 10)
        assert np.array_equal(nh, rnb)
        for q in range(nq):
            assert_bit_exact(rb[q, :rnb[q]], hits[q, :nh[q]], what=f"nq {nq} q{q}")


@pytest.mark.parametrize("tune,handover", [(dict(win_order_arith=0), 1), (dict(win_grid=2), 0), (dict(win_fuse=0), 0), (dict(win_skew=0), 1)],
                         ids=["order_from_memory", "win_grid", "three_launches", "no_skew"])
def test_launches_that_do_not_qualify(tuning, V, tune, handover):
    """the item order loaded from memory, a grid set by hand, the three-launch form, equal parts: the lists go through memory
    (or merge_kernel merges) exactly as before"""
    tuning(win_force=1, fused=0, **tune)
    for nq in (4, 9):
        terms, off = _v_queries(nq, seed=10 + nq)
        b, hits, nh = _run_and_check(V, terms, off, 10, handover=handover, what=str(tune))
        b.run()
        h2, n2 = b.fetch()
        assert h2.tobytes() == hits.tobytes() and np.array_equal(n2, nh)
