"""What tests/test_gpu_work_items.py needs of tests/work_items_model.py, stated without a GPU so that a GPU case cannot pass by never
reaching its edge: every boundary kind of the designed index occurs under the tunings the GPU test uses, every clamp is reached (or
shown to be out of reach), the batches beyond 1024 queries put their queries without postings on both slots of a plan_kernel
thread, and the segment builder lays the lists into the blocks the model says.  The conditions are conditions, not measurements: if
one fails, mend the data or the tuning, not the condition."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import work_items_model as M

BIG_NQ = (1023, 1024, 1025, 2047, 2049, 3001)


# ---- the planner's arithmetic ---------------------------------------------------------------------------------------------------
def test_ranges_tile_the_documents_for_every_cut():
    for n_docs in (1, 2, 3, 5, 64, 65, 6000, 19997):
        for c in sorted(x for x in {1, 2, 3, 7, 64, n_docs} if x <= n_docs):
            r = M.item_ranges(n_docs, c)
            assert r[0][0] == 0 and r[-1][1] == n_docs and all(a[1] == b[0] for a, b in zip(r, r[1:]))
            assert all(lo < hi for lo, hi in r)           # c <= n_docs: no empty range
    assert any(lo == hi for lo, hi in M.item_ranges(2, 5))  # ... which is what the n_docs clamp is for


def test_plan_rounds_to_nearest_with_a_floor_of_one():
    df = [100, 191, 192, 64000]
    general = dict(fused=0, win=0, arith=0, dense_x1000=10**9, range_min_chunk=128, range_items=256)
    p = M.plan(10**6, df, [[0], [1], [2], [7]], 10, **general)
    assert p["route"] == M.GENERAL and p["chunk"] == 128 and p["c"] == [1, 1, 2, 0] and p["total"] == 4
    p = M.plan(10**6, df, [[3], [0]], 10, **general)      # chunk = ceil(64100 / 256) = 251
    assert p["chunk"] == 251 and p["c"] == [255, 1]
    p = M.plan(10**6, df, [[3]], 300)                     # k > 256: 8192 postings an item, whatever the switches
    assert p["chunk"] == M.MIN_CHUNK and p["c"] == [8] and p["classes"] == [8, 0, 0]
    # the g routes: a quarter of the chunk up to 8 queries, one g for all, at most 64
    free = dict(fused=0, win=0, dense_x1000=10**9, range_min_chunk=128, range_items=256)
    assert M.plan(10**6, df, [[2]], 10, **free)["g"] == 6 and M.plan(10**6, df, [[2]] * 9, 10, **free)["g"] == 2
    assert M.plan(10**6, df, [[3]], 10, **free)["g"] == 64 and M.plan(10**6, df, [[3]], 10, **free)["raw_g"] == 2000
    assert M.plan(10**6, df, [[3]] * 100, 10, **free)["g"] == 3   # (256 + 50) // 100
    assert M.plan(10**6, df, [[2]], 10, **free)["route"] == M.PLAN_FREE
    assert M.plan(10**6, df, [[2]], 10, **dict(free, fused=1))["route"] == M.ONE_LAUNCH
    assert M.plan(10**6, df, [[2], []], 10, **free)["route"] == M.GENERAL      # a query without postings: plan_kernel's


# ---- A: beyond 1024 queries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", BIG_NQ)
def test_big_batches_put_their_holes_on_both_slots(nq):
    n_terms = 300
    queries = M.big_queries(nq, n_terms, seed=nq)
    per, threads = M.plan_threads(nq)
    assert per == (1 if nq <= 1024 else 2 if nq <= 2048 else 3)
    assert sum(q1 - q0 for q0, q1 in threads) == nq and threads[-1][1] == nq
    if nq == 2047:
        assert threads[-1] == (2046, 2047)                # the last thread's share is short
    elif nq > 1024:
        assert any(q1 == q0 for q0, q1 in threads)        # threads beyond ceil(nq / per) own nothing
        assert nq % per == 0 or any(0 < q1 - q0 < per for q0, q1 in threads)
    slots = M.hole_slots(queries, n_terms)
    assert {("first", "empty"), ("first", "unknown"), ("last", "empty"), ("last", "unknown")} <= slots
    if per >= 2:  # a thread whose first two queries both make no item: the next one's base must not move
        assert any(all(not any(x < n_terms for x in queries[q]) for q in (q0, q0 + 1)) for q0, q1 in threads if q1 - q0 >= 2)
    assert sum(len([x for x in q if x < n_terms]) > 16 for q in queries) == 1
    assert all(q == sorted(set(q)) for q in queries)
    full = M.big_queries(nq, n_terms, seed=nq, holes=False)
    assert all(1 <= len(q) <= 4 and max(q) < n_terms for q in full)


def test_big_batches_are_cut_under_the_cut_tuning():
    """with a made-up df of 200 postings a term (the GPU test uses the corpus's own): most queries get more than one item, and the
    items stay within the batch's room (max_queries + target items)"""
    df = np.full(300, 200)
    for nq in BIG_NQ:
        p = M.plan(3000, df, M.big_queries(nq, 300, seed=nq), 10, dense_x1000=10**9, range_min_chunk=128, range_items=8192)
        assert p["route"] == M.GENERAL and p["total"] <= nq + 8192
        assert sum(c > 1 for c in p["c"]) > nq // 2 and p["classes"][2] >= 1 and p["classes"][0] > nq
        f = M.plan(3000, df, M.big_queries(nq, 300, seed=nq, holes=False), 10, fused=0, win=0, dense_x1000=10**9, range_min_chunk=128,
                   range_items=8192)
        assert f["route"] == M.PLAN_FREE and f["g"] >= 2


# ---- B: designed cuts -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["both", "lo", "hi"])
def cut(request):
    n_docs, lists, doc_len = M.cut_index(request.param)
    return request.param, n_docs, lists, doc_len, [len(d) for d, _ in lists]


def test_every_cut_case_takes_its_route_and_a_multiple_of_eight_items(cut):
    _, n_docs, lists, _, df = cut
    seen = set()
    for name, (queries, k, tune, route, cls) in M.cut_cases().items():
        p = M.plan(n_docs, df, queries, k, **tune)
        assert p["route"] == route, name
        if name.endswith("-one"):
            assert set(p["c"]) == {1}, name
        else:
            assert all(c % M.B_CUT == 0 and c >= M.B_CUT for c in p["c"]), (name, p["c"])
        if cls is not None:
            assert p["classes"][cls] == p["total"], (name, p["classes"])
        assert p["total"] <= len(queries) + (max(256, tune.get("range_items", 1024)) if k <= 256 else M.TARGET_ITEMS) + \
            (max(256, tune.get("dense_items", M.D_TARGET_ITEMS)) if p["has_dense"] else 0), name
        seen.add((route, cls, k > 256, "grid1" in name))
    p = M.plan(n_docs, df, *M.cut_cases()["k300"][:2])
    assert p["c"] == [8, 8] and p["valid"] == [15, 20]   # scan_many_kernel's hash mode (< 16 terms) and its dense mode
    assert {(M.GENERAL, 0, False, True), (M.PLAN_FREE, None, False, True), (M.GENERAL, 1, False, True), (M.ONE_LAUNCH, None, False, False),
            (M.GENERAL, 2, False, False), (M.GENERAL, None, True, False)} <= seen


def test_the_boundaries_fall_where_the_design_says(cut):
    spikes, n_docs, lists, doc_len, df = cut
    E = M.B_EDGES
    w = lists[M.T_W][0]
    kinds = {e: M.boundary_kinds(w, e) for e in E}
    assert "in_full" in kinds[E[0]] and "on_min" in kinds[E[1]] and kinds[E[2]] == {"past_max"} and E[2] not in w
    assert kinds[E[3]] == {"in_full"} and E[3] in w and {"on_min", "past_max"} <= kinds[E[4]]
    assert kinds[E[5]] == {"in_full"} and kinds[E[6]] == {"in_tail"}
    assert {"in_full", "in_tail", "on_min", "past_max"} == set().union(*kinds.values())
    # the split query: items of one term only, and items without any posting, with a list ending and one beginning on a boundary
    it = M.items_terms(lists, M.Q_SPLIT, n_docs, M.B_CUT)
    assert it == [{M.T_L}] * 3 + [set()] * 2 + [{M.T_H}] * 3
    assert "past_max" in M.boundary_kinds(lists[M.T_L][0], E[2]) and "on_min" in M.boundary_kinds(lists[M.T_H][0], E[4])
    finest = M.items_terms(lists, M.Q_SPLIT, n_docs, 32)
    assert set() in finest and {M.T_L} in finest and {M.T_H} in finest
    # the wide query has every term in every item
    assert all(x == set(M.Q_WIDE) for x in M.items_terms(lists, M.Q_WIDE, n_docs, M.B_CUT))
    # spikes: short documents with tf 200, on the side(s) of every boundary the variant names, fewer than k of them
    s = set(int(x) for x in lists[M.T_S][0])
    assert {0, n_docs - 1} <= s and len(s) < M.B_K
    for e in E:
        assert (e in s) == (spikes in ("both", "lo")) and (e - 1 in s) == (spikes in ("both", "hi"))
    assert all(doc_len[d] == 1 for d in s) and (doc_len == 1).sum() == len(s)
    for t in (M.T_L, M.T_H):
        d, tf = lists[t]
        assert all(tf[np.isin(d, list(s))] == 200) and tf[~np.isin(d, list(s))].max() <= 3
        assert np.isin(d, list(s)).sum() >= (6 if spikes == "both" else 3)


def test_the_segment_builder_lays_the_blocks_as_the_model_says(cut):
    _, n_docs, lists, doc_len, df = cut
    seg = vb.Segment.build(1.2, 0.75, *M.build_args(n_docs, lists, doc_len))
    a = seg.arrays()
    assert seg.n_docs == n_docs and a["term_df"].tolist() == df
    first = a["term_first_block"]
    for t in (M.T_W, M.T_S, M.T_L, M.T_H, M.T_F0):
        got = [(int(a["blk_min_doc"][j]), int(a["blk_max_doc"][j]), int(a["blk_n"][j])) for j in range(first[t], first[t + 1])]
        assert got == M.blocks(lists[t][0]), t
    j = first[M.T_W + 1] - 1                              # W's tail is byte-packed, its other blocks bit-packed
    assert a["blk_meta_doc"][j] >= 0x80 and a["blk_n"][j] == 114 and all(a["blk_meta_doc"][first[M.T_W]:j] < 32)


# ---- C: the merge ---------------------------------------------------------------------------------------------------------------
def test_flat_indexes_are_cut_as_the_merge_cases_need():
    for n, c in ((63, 1), (64, 1), (65, 1), (200, 2), (384, 3), (1000, 8)):
        n_docs, lists, _ = M.flat_index(n)
        p = M.plan(n_docs, [n], [[0]], 10, **M.MERGE_TUNE)
        assert p["route"] == M.GENERAL and p["c"] == [c] and p["classes"] == [c, 0, 0], n
    assert M.LISTS_PER_ITEM * 3 > 16 >= M.LISTS_PER_ITEM * 2   # three items: a second round of 16 lists
    p = M.plan(20000, [20000], [[0]], 300)
    assert p["c"] == [2]                                       # the LDS form with two lists
    assert M.flat_expected(10, 4) == [0, 1, 2, 3] and M.flat_expected(10, 4, high=[7, 2]) == [2, 7, 0, 1]
    assert M.flat_expected(5, 9, high=[4]) == [4, 0, 1, 2, 3]


def test_merge_form_follows_the_kernel_rounds():
    z = np.zeros(8, dtype=np.uint32)
    eight = np.full(8, 8, dtype=np.uint32)
    assert M.merge_form(eight, eight, 10) == ("ranked", None, 1, 64)
    nine = eight.copy()
    nine[7] = 9
    assert M.merge_form(nine, nine, 10) == ("register", 0, 1, 65)
    four = np.full(24, 4, dtype=np.uint32)
    assert M.merge_form(four, four, 4) == ("register", 1, 2, 96)
    assert M.merge_form(four, np.r_[four[:16], z], 4) == ("ranked", None, 2, 64)
    assert M.merge_form(z[:2], z[:2], 300)[0] == "lds"


# ---- D: the clamps --------------------------------------------------------------------------------------------------------------
def test_the_clamps_are_reached_or_out_of_reach():
    general = dict(fused=0, win=0, arith=0, dense_x1000=10**9, range_min_chunk=128, range_items=256)
    for n_docs in (1, 2, 3):
        _, lists, _ = M.tiny_index(n_docs)
        df = [len(d) for d, _ in lists]
        queries = [list(range(300)), list(range(17)), [0, 1, 2, 3, 4]]
        p = M.plan(n_docs, df, queries, 10, **general)
        assert p["raw_c"][0] > n_docs == p["c"][0] and p["c"][1:] == [1, 1] and p["classes"] == [1, 0, n_docs + 1]   # chunks_of's clamp
        # every query dense: min(dense_c, n_docs), the many-term queries too (they are scan_many_kernel's all the same)
        p = M.plan(n_docs, df, queries, 10, fused=0, win=0, dense_x1000=0, dense_items=256)
        assert p["dense_c"] == 85 and p["raw_c"] == [85] * 3 and p["c"] == [n_docs] * 3
        assert p["classes"] == [0, n_docs, 2 * n_docs]
        # k = 300: 8192 postings an item -- 1024 terms (the most a query may hold) in 3 documents are 3072 postings: no clamp to reach
        p = M.plan(n_docs, df, queries, 300)
        assert p["raw_c"] == [1, 1, 1] and 1024 * 3 < M.MIN_CHUNK + M.MIN_CHUNK // 2
    # g <= min(64, n_docs): a query of the g routes has at most 16 terms, so at most 16 n_docs postings, and the finest chunk is 32:
    # g = (16 n_docs + 16) // 32 <= n_docs before the clamp -- it cannot bind.  (64 does: test_plan_rounds_...)
    for n_docs in range(1, 200):
        assert (16 * n_docs + 16) // 32 <= n_docs
    _, lists, _ = M.tiny_index(5, 16)
    nine = [list(range(16))] * 9
    p = M.plan(5, [5] * 16, nine, 10, fused=1, win=0, fused_items=4096, dense_x1000=10**9, range_min_chunk=128, range_items=256)
    assert p["route"] == M.ONE_LAUNCH and p["g"] == 1 and p["raw_g"] <= 5
    p = M.plan(5, [5] * 16, nine[:8], 10, fused=1, win=0, fused_items=4096, dense_x1000=10**9, range_min_chunk=128, range_items=256)
    assert p["g"] == 3 and p["raw_g"] == 3                # (80 + 16) // 32: three items of one or two documents each


def test_the_gpu_tests_corpus_is_cut_as_they_need():
    """the synthetic corpus of the GPU file (3000 documents, 300 tokens), its own document frequencies"""
    seg = vb.Segment.synth(3000, 300, mean_len=20, len_mode=1, seed=5)
    df = [int(x) for x in seg.arrays()["term_df"]]
    assert seg.n_terms == 300 and min(df) > 128
    cut = dict(dense_x1000=10**9, range_min_chunk=128, range_items=8192)
    for nq in BIG_NQ:
        queries = M.big_queries(nq, 300, seed=nq)
        p = M.plan(3000, df, queries, 10)
        assert p["route"] == M.GENERAL and min(p["classes"]) >= 1 and p["classes"][0] > 100 and p["classes"][1] > 100
        p = M.plan(3000, df, queries, 10, **cut)
        assert p["total"] > 2 * nq and p["total"] <= nq + 8192 and p["classes"][1] == 0 and max(p["c"]) > 16
        per, threads = M.plan_threads(nq)
        if per > 1:  # a thread whose first query has several items: the second one's base is not the thread's
            assert any(p["c"][q0] > 1 and q1 - q0 > 1 and p["c"][q0 + 1] > 0 for q0, q1 in threads)
        p = M.plan(3000, df, queries, 300)
        assert p["chunk"] == M.MIN_CHUNK and set(p["c"]) == {0, 1}
    for nq in (1025, 2049):
        full = M.big_queries(nq, 300, seed=nq, holes=False)
        assert M.plan(3000, df, full, 10, win=0, fused=0, **cut)["g"] >= 4
        assert M.plan(3000, df, full, 10, win=0, fused=1, fused_items=1 << 20, **cut)["route"] == M.ONE_LAUNCH
