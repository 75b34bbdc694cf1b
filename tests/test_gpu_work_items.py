"""Work items on every route but the window route: the cut of a query into document ranges (plan_kernel, its host mirror, the
in-kernel cut of the plan-free and the one-launch route), the item loops of scan_range_kernel, scan_dense_kernel and scan_many_kernel,
and merge_kernel -- on designed inputs, every record against the oracle's brute force bit for bit.  -m gpu only.

Every case first asserts its route (Batch.debug_route), its item total against tests/work_items_model.py (Batch.debug_counts) and,
on the general route, the kernel classes of its items (Batch.debug_routes): a run that silently makes one item fails.  What the
designed inputs reach is asserted without a GPU in tests/test_work_items_model.py.

A  batches of 1023 .. 3001 queries: from 1025 on a plan_kernel thread owns several queries (another code path), the staged block, the
   host's item order, merge_kernel's grid, vbm25_search_batch's cached batch and a MultiBatch share hold more than 1024 queries.
B  an index whose block edges sit on the item boundaries (work_items_model.cut_index), with spike documents on both sides of every
   boundary: a boundary document dropped, or scored in two items, changes the records.  Finest cut and one item: the same bytes.
C  merge_kernel's forms on one score bit pattern (order by document alone) and on two: at most 64 survivors ranked by counting, the
   register top-k from the 65th on, the LDS top-k beyond k = 256, rounds of 16 lists.  Batch.debug_lists proves the form taken
   wherever k holds every match (with a smaller k the number of surviving entries depends on when the items publish thresholds).
D  the clamps of c and dense_c to n_docs on indexes of 1, 2, 3 and 5 documents.
E  one batch object across routes and query counts, on memory dirtied first."""
import functools

import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
import work_items_model as M
from parity import assert_bit_exact

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------------------------------------------------
class Index:
    def __init__(self, seg):
        self.seg = seg
        a = seg.arrays()
        self.df = [int(x) for x in a["term_df"]]
        self.n_docs, self.n_terms = seg.n_docs, seg.n_terms
        self.gix = vb.GpuIndex(seg)
        self.oix = orc.OracleIndex.from_arrays(seg.meta(), a)
        self._ref = {}

    @classmethod
    def build(cls, n_docs, lists, doc_len):
        ix = cls(vb.Segment.build(1.2, 0.75, *M.build_args(n_docs, lists, doc_len)))
        assert ix.df == [len(d) for d, _ in lists]
        return ix

    def oracle(self, queries, k):
        """the brute-force records of a query list, computed once"""
        key = (k, tuple(tuple(q) for q in queries))
        if key not in self._ref:
            terms, off = M.csr(queries)
            ref, n_ref, _ = self.oix.search_batch(terms, off, k, mode="brute", threads=8)
            ref.setflags(write=False)
            n_ref.setflags(write=False)
            self._ref[key] = (ref, n_ref)
        return self._ref[key]


def assert_oracle(ix, queries, k, hits, nh, what):
    ref, n_ref = ix.oracle(queries, k)
    assert np.array_equal(nh, n_ref), f"{what}: hit counts differ at queries {np.flatnonzero(nh != n_ref)[:8]}"
    live = np.arange(k)[None, :] < n_ref[:, None]
    same = (hits["doc_id"] == ref["doc_id"]) & (hits["score"].view(np.uint64) == ref["score"].view(np.uint64)) & \
        (hits["payload"] == ref["payload"]).all(axis=2)
    bad = np.flatnonzero((~same & live).any(axis=1))
    for q in bad[:1]:
        assert_bit_exact(ref[q, :n_ref[q]], hits[q, :nh[q]], what=f"{what} q{q} {queries[q][:8]}")
    assert not len(bad)


def records(hits, nh, rows=None):
    """the returned records as bytes, field by field (what lies beyond a query's count is not part of the result, nor is the padding
    of numpy's record, which a concatenation of slices does not carry over)"""
    rows = range(len(nh)) if rows is None else rows
    return b"".join(np.ascontiguousarray(hits[f][q, :nh[q]]).tobytes() for q in rows for f in ("score", "doc_id", "payload")) + \
        np.asarray(nh)[list(rows)].tobytes()


def run_batch(ix, queries, k, plan=None, route=None, what="", max_queries=None):
    """one batch object under the current tuning: route, item total and kernel classes asserted, then the records"""
    terms, off = M.csr(queries)
    b = vb.Batch(ix.gix, max_queries or len(queries), len(terms), k)
    return rerun_batch(b, ix, queries, k, plan, route, what)


def rerun_batch(b, ix, queries, k, plan=None, route=None, what=""):
    terms, off = M.csr(queries)
    b.set_queries(terms, off)
    want = plan["route"] if plan is not None else route
    assert b.debug_route() == want, f"{what}: route {b.debug_route()}, not {want}"
    b.run()
    hits, nh = b.fetch()
    if plan is not None:
        assert b.debug_counts() == (plan["total"], 0), f"{what}: {b.debug_counts()} items (made, given up), the model has {plan['total']}"
        if plan["route"] == M.GENERAL:
            assert list(b.debug_routes()[3:]) == plan["classes"], f"{what}: items by kernel {b.debug_routes()}, the model has {plan['classes']}"
    return b, hits, nh


def in_slices(ix, queries, k, step=1024):
    """the same queries through batches of at most 1024, under the current tuning"""
    out_h, out_n = [], []
    for s in range(0, len(queries), step):
        terms, off = M.csr(queries[s:s + step])
        b = vb.Batch(ix.gix, step, len(terms), k)
        b.set_queries(terms, off)
        b.run()
        h, n = b.fetch()
        out_h.append(h)
        out_n.append(n)
    return np.concatenate(out_h), np.concatenate(out_n)


# --------------------------------------------------------------------------------------------------------------------------------
# A: beyond 1024 queries
# --------------------------------------------------------------------------------------------------------------------------------
CUT_TUNE = dict(dense_x1000=10**9, range_min_chunk=128, range_items=8192)


@pytest.fixture(scope="module")
def corpus():
    return Index(vb.Segment.synth(3000, 300, mean_len=20, len_mode=1, seed=5))


@pytest.mark.parametrize("nq", [1023, 1024, 1025, 2047, 2049, 3001])
def test_batches_beyond_the_planner_workgroup(tuning, corpus, nq):
    """the general route (a 20-term query and queries without postings are in the batch) at the default tuning -- sparse, dense and
    many-term items side by side --, cut finely (several items a query: the thread's base advances by more than one), and at k = 300
    (scan_many_kernel only): equal to the oracle, and to the same queries in batches of at most 1024"""
    queries = M.big_queries(nq, corpus.n_terms, seed=nq)
    for name, k, tune in (("default", 10, {}), ("cut", 10, CUT_TUNE), ("k300", 300, {})):
        vb.reset_tuning()
        tuning(**tune)
        p = M.plan(corpus.n_docs, corpus.df, queries, k, **tune)
        assert p["route"] == M.GENERAL and p["classes"][2] >= 1
        if name == "default":
            assert p["classes"][0] > 100 and p["classes"][1] > 100          # sparse and dense items side by side
        if name == "cut":
            assert p["total"] > 2 * nq and p["classes"][1] == 0
        if name == "k300":
            assert p["chunk"] == M.MIN_CHUNK and p["total"] <= M.TARGET_ITEMS + nq
        _, hits, nh = run_batch(corpus, queries, k, plan=p, what=f"{name} nq={nq}")
        assert_oracle(corpus, queries, k, hits, nh, f"{name} nq={nq}")
        if nq > 1024:
            sh, sn = in_slices(corpus, queries, k)
            assert records(hits, nh) == records(sh, sn), f"{name} nq={nq}: one batch and slices of 1024 differ"


@pytest.mark.parametrize("nq", [1025, 2049])
def test_routes_without_plan_kernel_beyond_1024_queries(tuning, corpus, nq):
    """every query with postings: the plan-free route (the host's item order for more than 1024 queries), the one-launch route, the
    window route (route only: its items are windows), and the same through vb.search_batch (its cached batch object)"""
    queries = M.big_queries(nq, corpus.n_terms, seed=nq, holes=False)
    k = 10
    free = dict(CUT_TUNE, win=0, fused=0)
    one = dict(CUT_TUNE, win=0, fused=1, fused_items=1 << 20)
    got = {}
    for name, tune in (("plan-free", free), ("one-launch", one)):
        vb.reset_tuning()
        tuning(**tune)
        p = M.plan(corpus.n_docs, corpus.df, queries, k, **tune)
        assert p["route"] == (M.PLAN_FREE if name == "plan-free" else M.ONE_LAUNCH) and p["g"] >= 2 and p["total"] == nq * p["g"]
        _, hits, nh = run_batch(corpus, queries, k, plan=p, what=f"{name} nq={nq}")
        assert_oracle(corpus, queries, k, hits, nh, f"{name} nq={nq}")
        sh, sn = in_slices(corpus, queries, k)
        assert records(hits, nh) == records(sh, sn), f"{name} nq={nq}: one batch and slices of 1024 differ"
        got[name] = records(hits, nh)
    assert got["plan-free"] == got["one-launch"]
    vb.reset_tuning()
    tuning(win_force=1, fused=0, dense_x1000=10**9)
    b, hits, nh = run_batch(corpus, queries, k, route=M.WINDOW, what=f"window nq={nq}")
    items, _ = b.debug_counts()   # (win_force on lists this dense: some windows overflow their list and go to scan_many_kernel)
    assert items >= nq and items % nq == 0
    assert_oracle(corpus, queries, k, hits, nh, f"window nq={nq}")
    assert records(hits, nh) == got["plan-free"]
    for name, tune in (("search_batch", {}), ("search_batch-cut", free)):
        vb.reset_tuning()
        tuning(**tune)
        terms, off = M.csr(queries)
        hits, nh = vb.search_batch(corpus.gix, terms, off, k)
        assert_oracle(corpus, queries, k, hits, nh, f"{name} nq={nq}")
        part = [vb.search_batch(corpus.gix, *M.csr(queries[s:s + 1024]), k) for s in range(0, nq, 1024)]  # (the cached batch shrinks and grows)
        assert records(hits, nh) == records(np.concatenate([h for h, _ in part]), np.concatenate([n for _, n in part]))
        hits2, nh2 = vb.search_batch(corpus.gix, terms, off, k)
        assert records(hits, nh) == records(hits2, nh2)


@pytest.mark.parametrize("holes", [True, False])
def test_multi_batch_shares_beyond_1024_queries(tuning, corpus, holes):
    """two replicas on one device, 3001 queries: shares of 1501 and 1500"""
    nq, k = 3001, 10
    queries = M.big_queries(nq, corpus.n_terms, seed=77, holes=holes)
    tuning(**CUT_TUNE, win=0, fused=0)
    multi = vb.MultiIndex(corpus.seg, [0, 0])
    assert multi.n_devices == 2 and nq // 2 > 1024
    terms, off = M.csr(queries)
    mb = vb.MultiBatch(multi, nq, len(terms), k)
    for _ in range(2):
        mb.set_queries(terms, off)
        mb.run()
        hits, nh = mb.fetch()
        assert_oracle(corpus, queries, k, hits, nh, f"multi holes={holes}")
    hits2, nh2 = multi.search_batch(terms, off, k)
    assert records(hits, nh) == records(hits2, nh2)
    sh, sn = in_slices(corpus, queries, k)
    assert records(hits, nh) == records(sh, sn), f"multi holes={holes}: the two shares and slices of 1024 differ"


# --------------------------------------------------------------------------------------------------------------------------------
# B: designed item cuts
# --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cut_ix(spikes):
    return Index.build(*M.cut_index(spikes))


@functools.lru_cache(maxsize=None)
def cut_run(spikes, name):
    """one case of work_items_model.cut_cases on the index of that spike variant: asserted against plan and oracle, records kept"""
    ix = cut_ix(spikes)
    queries, k, tune, route, cls = M.cut_cases()[name]
    vb.reset_tuning()
    try:
        for key, value in tune.items():
            vb.set_tuning(key, value)
        p = M.plan(ix.n_docs, ix.df, queries, k, **tune)
        assert p["route"] == route
        b, hits, nh = run_batch(ix, queries, k, plan=p, what=f"{name} spikes={spikes}")
    finally:
        vb.reset_tuning()
    assert_oracle(ix, queries, k, hits, nh, f"{name} spikes={spikes}")
    return p, hits, nh


@pytest.mark.parametrize("spikes", ["both", "lo", "hi"])
@pytest.mark.parametrize("name", list(M.cut_cases()))
def test_designed_cuts(name, spikes):
    ix = cut_ix(spikes)
    p, hits, nh = cut_run(spikes, name)
    queries, k = M.cut_cases()[name][:2]
    if not name.endswith("-one"):
        assert min(p["c"]) >= M.B_CUT
    # the spikes are among the hits of every query that holds them (all of them: fewer than k), the two of the index's ends first
    s = set(int(x) for x in M.cut_index(spikes)[1][M.T_S][0])
    for q, query in enumerate(queries[:2]):
        got = set(int(x) for x in hits["doc_id"][q, :nh[q]])
        held = s if M.T_S in query else {d for t in query for d in M.cut_index(spikes)[1][t][0] if int(d) in s}
        assert set(int(x) for x in held) <= got, f"{name} q{q}: spikes {sorted(set(int(x) for x in held) - got)} are not among the hits"


@pytest.mark.parametrize("spikes", ["both", "lo", "hi"])
def test_the_finest_cut_and_one_item_give_the_same_bytes(spikes):
    """(k = 300 has no uncut twin: beyond k = 256 an item is 8192 postings whatever the switches, so the 15- and the 20-term query, which
    need 8 x 8192 postings to be cut at all, cannot be made one item on the same index -- scan_many_kernel's hash and dense mode at
    k = 300 are held to the oracle alone; its item loop at k = 32 has its twin, many-term-one)"""
    for family in ("general", "plan-free", "one-launch", "dense", "many-term"):
        one = cut_run(spikes, family + "-one")
        n = len(M.cut_cases()[family + "-one"][0])
        rows = range(min(n, 2))
        for name in M.cut_cases():
            if name.startswith(family) and not name.endswith("-one"):
                p, hits, nh = cut_run(spikes, name)
                assert records(hits, nh, rows) == records(one[1], one[2], rows), f"{name} and {family}-one differ (spikes={spikes})"
    # ... and the routes among each other (the same two queries)
    base = cut_run(spikes, "general-one")
    for name in ("plan-free-finest", "one-launch-finest", "dense-default", "dense-8"):
        p, hits, nh = cut_run(spikes, name)
        assert records(hits, nh, range(2)) == records(base[1], base[2], range(2)), name


# --------------------------------------------------------------------------------------------------------------------------------
# C: the merge
# --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flat_ix(n_docs, high, docs=None):
    return Index.build(*M.flat_index(n_docs, high, docs))


def two_levels(n_docs):
    """the documents of the second, higher score level: a few in every third of the index, the last document among them"""
    return tuple(sorted({3, n_docs // 3 + 1, n_docs // 2, n_docs - 2, n_docs - 1}))


# name -> (documents, k, items, what Batch.debug_lists must show: form, the round of 16 lists in which the 65th survivor comes, rounds,
# survivors -- None: not pinned)
MERGE_CASES = {
    "63-entries": (63, 100, 1, ("ranked", None, 1, 63)),
    "64-entries": (64, 100, 1, ("ranked", None, 1, 64)),
    "65-entries": (65, 100, 1, ("register", 0, 1, 65)),
    "two-items-16-lists": (200, 256, 2, ("register", 0, 1, 200)),
    "three-items-small-k": (384, 4, 3, (None, None, 2, None)),      # (k < the matches: how many entries survive depends on when
    "eight-items-small-k": (1000, 10, 8, (None, None, 4, None)),    # the items publish their thresholds -- the form is not pinned)
    "k-over-the-matches": (100, 256, 1, ("register", 0, 1, 100)),
    "k-over-the-matches-lds": (300, 1024, 1, ("lds", None, None, 300)),
    "k=64": (1000, 64, 8, (None, None, 4, None)),
    "k=65": (1000, 65, 8, (None, None, 4, None)),
    "k=128": (1000, 128, 8, ("register", 0, 4, 1000)),               # (an item's 125 matches fit every list: all survive)
    "k=256": (1000, 256, 8, ("register", 0, 4, 1000)),
    "k=257": (20000, 257, 2, ("lds", None, None, None)),
    "k=1024": (20000, 1024, 2, ("lds", None, None, None)),
}


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("name", list(MERGE_CASES))
def test_merge_forms(tuning, name, levels):
    n_docs, k, items, want = MERGE_CASES[name]
    high = two_levels(n_docs) if levels == 2 else ()
    ix = flat_ix(n_docs, high)
    tuning(**M.MERGE_TUNE)
    queries = [[0]]
    p = M.plan(n_docs, ix.df, queries, k, **M.MERGE_TUNE)
    assert p["c"] == [items], p["c"]
    b, hits, nh = run_batch(ix, queries, k, plan=p, what=name)
    cnt, surv = b.debug_lists(0)
    form = M.merge_form(cnt, surv, k)
    print(f"{name} levels={levels}: lists {len(cnt)} entries {int(cnt.sum())} survivors {int(surv.sum())} form {form}")
    assert len(cnt) == items * (M.LISTS_PER_ITEM if k <= M.REG_K else 1)
    assert nh[0] == min(k, n_docs)
    assert hits["doc_id"][0, :nh[0]].tolist() == M.flat_expected(n_docs, k, high), name
    assert len(set(hits["score"][0, :nh[0]].view(np.uint64).tolist())) == (levels if k > len(high) else 1)
    assert_oracle(ix, queries, k, hits, nh, name)
    if levels == 1 or k >= n_docs:
        for i, (w, g) in enumerate(zip(want, form)):       # (with k >= the matches every entry survives on both levels)
            assert w is None or w == g, f"{name}: merge_kernel took {form}, the case needs {want}"


@pytest.mark.parametrize("n_docs", [64, 65])
def test_merge_of_more_than_16_lists_at_64_and_65_survivors(tuning, n_docs):
    """64 and 65 survivors over eight items (64 lists, four rounds) -- which only scan_dense_kernel's cut by documents reaches: a
    sparse query of so few postings is one item"""
    tune = dict(fused=0, win=0, dense_x1000=0, dense_items=256)
    tuning(**tune)
    ix = flat_ix(n_docs, ())
    queries, k = [[0]] * 32, 100
    p = M.plan(n_docs, ix.df, queries, k, **tune)
    assert p["c"] == [8] * 32 and p["classes"] == [0, 256, 0]
    b, hits, nh = run_batch(ix, queries, k, plan=p, what=f"dense {n_docs}")
    for q in (0, 31):
        cnt, surv = b.debug_lists(q)
        form = M.merge_form(cnt, surv, k)
        print(f"dense n_docs={n_docs} q{q}: entries {int(cnt.sum())} survivors {int(surv.sum())} form {form}")
        assert form[2:] == (4, n_docs) and form[0] == ("ranked" if n_docs == 64 else "register")
        if n_docs == 65:  # the 65th comes after the first round of 16 lists: survivors buffered in one round are offered in another
            assert form[1] is not None and form[1] >= 1
        assert hits["doc_id"][q, :nh[q]].tolist() == list(range(n_docs))
    assert_oracle(ix, queries, k, hits, nh, f"dense {n_docs}")


@pytest.mark.parametrize("levels", [1, 2])
def test_the_65th_survivor_comes_in_the_second_round_of_lists(tuning, levels):
    """a sparse query of three items whose first two (16 lists, the first round) hold 30 matches each and the third 260: k = 256 holds
    every list whole, so no threshold cuts an entry, the first round buffers 60 survivors and the second one brings the 65th -- the
    buffered ones are offered to the register top-k first.  The hits: the 256 lowest of the 320 documents."""
    n_docs, k = 3000, 256
    docs = np.r_[np.arange(30) * 33 + 5, 1000 + np.arange(30) * 31, 2000 + np.arange(260) * 3 + 1]
    high = (docs[3], docs[45], docs[100], docs[319]) if levels == 2 else ()
    ix = flat_ix(n_docs, tuple(int(x) for x in high), tuple(int(x) for x in docs))
    tuning(**M.MERGE_TUNE)
    p = M.plan(n_docs, ix.df, [[0]], k, **M.MERGE_TUNE)
    assert p["c"] == [3] and [int(((docs >= lo) & (docs < hi)).sum()) for lo, hi in M.item_ranges(n_docs, 3)] == [30, 30, 260]
    b, hits, nh = run_batch(ix, [[0]], k, plan=p, what="second round")
    cnt, surv = b.debug_lists(0)
    form = M.merge_form(cnt, surv, k)
    print(f"second round levels={levels}: entries {cnt.tolist()} survivors {surv.tolist()} form {form}")
    assert hits["doc_id"][0, :nh[0]].tolist() == M.flat_expected(n_docs, k, high, docs)
    assert_oracle(ix, [[0]], k, hits, nh, "second round")
    assert int(cnt[:16].sum()) == 60 and int(cnt.sum()) == 320
    if levels == 1:  # (one score: every entry is at the threshold or above it, whenever it was published)
        assert form == ("register", 1, 2, 320)


def test_the_kth_place_is_a_tie_between_two_items(tuning):
    """384 documents in three items of 128; six higher ones in the last item; k = 136: the 130 places behind them go to the documents
    0 .. 129 -- 128 and 129 from the second item's lists, against the equal scores of the third item's"""
    high = (300, 301, 302, 303, 304, 305)
    ix = flat_ix(384, high)
    tuning(**M.MERGE_TUNE)
    for k in (136, 134, 6, 7):
        p = M.plan(384, ix.df, [[0]], k, **M.MERGE_TUNE)
        assert p["c"] == [3]
        b, hits, nh = run_batch(ix, [[0]], k, plan=p, what=f"tie k={k}")
        assert hits["doc_id"][0, :nh[0]].tolist() == (list(high) + list(range(k - 6)))[:k]
        assert_oracle(ix, [[0]], k, hits, nh, f"tie k={k}")


# --------------------------------------------------------------------------------------------------------------------------------
# D: clamps
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", [1, 2, 3])
def test_more_items_than_documents(tuning, n_docs):
    ix = Index.build(*M.tiny_index(n_docs))
    queries = [list(range(300)), list(range(17)), [0, 1, 2, 3, 4]]
    general = dict(fused=0, win=0, arith=0, dense_x1000=10**9, range_min_chunk=128, range_items=256)
    dense = dict(fused=0, win=0, dense_x1000=0, dense_items=256)
    for name, k, tune in (("general", 10, general), ("dense", 10, dense), ("dense-default", 10, dict(dense_x1000=0)), ("k300", 300, {})):
        vb.reset_tuning()
        tuning(**tune)
        p = M.plan(n_docs, ix.df, queries, k, **tune)
        if name == "general":
            assert p["raw_c"][0] > n_docs == p["c"][0]
        if name.startswith("dense"):
            assert p["dense_c"] > n_docs and p["c"] == [n_docs] * 3
        _, hits, nh = run_batch(ix, queries, k, plan=p, what=f"{name} n_docs={n_docs}")
        assert nh.tolist() == [n_docs] * 3
        assert_oracle(ix, queries, k, hits, nh, f"{name} n_docs={n_docs}")


def test_nine_queries_on_five_documents(tuning):
    ix = Index.build(*M.tiny_index(5, 16))
    tune = dict(fused=1, win=0, fused_items=4096, dense_x1000=10**9, range_min_chunk=128, range_items=256)
    tuning(**tune)
    for nq, g in ((9, 1), (8, 3), (1, 3)):
        queries = [list(range(16 - q % 3)) for q in range(nq)]
        p = M.plan(5, ix.df, queries, 10, **tune)
        assert p["route"] == M.ONE_LAUNCH and p["g"] == g <= 5
        _, hits, nh = run_batch(ix, queries, 10, plan=p, what=f"{nq} queries")
        assert nh.tolist() == [5] * nq
        assert_oracle(ix, queries, 10, hits, nh, f"{nq} queries")
    vb.reset_tuning()
    tuning(**dict(tune, fused=0))
    queries = [list(range(16 - q % 3)) for q in range(8)]
    p = M.plan(5, ix.df, queries, 10, **dict(tune, fused=0))
    assert p["route"] == M.PLAN_FREE and p["g"] == 3
    _, hits, nh = run_batch(ix, queries, 10, plan=p, what="plan-free")
    assert_oracle(ix, queries, 10, hits, nh, "plan-free")


# --------------------------------------------------------------------------------------------------------------------------------
# E: one batch object across routes and query counts
# --------------------------------------------------------------------------------------------------------------------------------
def test_one_batch_object_across_routes_and_counts(tuning, corpus):
    from test_gpu_search import _dirty_the_allocator

    tune = dict(CUT_TUNE, win=0, fused=1, fused_items=128)
    tuning(**tune)
    k = 10
    sets = {(nq, holes): M.big_queries(nq, corpus.n_terms, seed=1000 + nq, holes=holes) for nq in (2049, 3, 1025) for holes in (True, False)}
    sets[(3, False)] = [q[:1] for q in sets[(3, False)]]      # (one term each: few enough items for the one-launch route)
    order = [(2049, False), (3, False), (1025, True), (3, False), (2049, True), (1025, False), (3, True), (2049, False), (3, False),
             (1025, True), (1025, False)]
    _dirty_the_allocator()
    b = vb.Batch(corpus.gix, 2049, max(len(M.csr(q)[0]) for q in sets.values()), k)
    seen = set()
    for step, key in enumerate(order):
        queries = sets[key]
        p = M.plan(corpus.n_docs, corpus.df, queries, k, **tune)
        seen.add((p["route"], key[0]))
        _, hits, nh = rerun_batch(b, corpus, queries, k, plan=p, what=f"step {step} {key}")
        assert_oracle(corpus, queries, k, hits, nh, f"step {step} {key}")
    assert {(M.PLAN_FREE, 2049), (M.ONE_LAUNCH, 3), (M.GENERAL, 1025), (M.GENERAL, 2049), (M.PLAN_FREE, 1025), (M.GENERAL, 3)} <= seen
