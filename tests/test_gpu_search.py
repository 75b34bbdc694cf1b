"""Parity of the HIP path (through the C ABI) against the CPU oracle.  -m gpu only.

Bit-exact rule: GPU == canonical brute force (doc ids, score bits, payloads).
Reference rule: GPU vs the faithful Block-WAND restatement: same ranking outside tie groups,
scores within 1e-5 (BASELINE.json north_star)."""
import json
import os

import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from parity import assert_bit_exact, assert_same_ranking

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def both(c=None, seg=None, k1=1.2, b=0.75):
    if seg is None:
        seg = vb.Segment.build(k1, b, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"],
                               c["post_doc"], c["post_tf"])
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    return seg, vb.GpuIndex(seg), oix


def _dirty_the_allocator():
    """Fill 1 GiB of HBM with 0x0a bytes and hand it back: what the library allocates next is not zero by luck (round 4: the
    one-launch route after a plan-free batch found the allocator's leftovers in a counter array nobody had initialised --
    and passed for as long as fresh memory happened to be zero)."""
    import torch
    junk = torch.full((1 << 28,), 0x0a0a0a0a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    del junk
    torch.cuda.empty_cache()


def check_batch(gix, oix, terms, off, k, wand=True):
    hits, nh = vb.search_batch(gix, terms, off, k)
    ob, onb, _ = oix.search_batch(terms, off, k, mode="brute", threads=8)
    assert np.array_equal(nh, onb)
    for q in range(len(off) - 1):
        assert_bit_exact(ob[q, :onb[q]], hits[q, :nh[q]], what=f"q{q} vs brute")
    if wand:
        ow, onw, _ = oix.search_batch(terms, off, k, mode="wand", threads=8)
        for q in range(len(off) - 1):
            t = terms[off[q]:off[q + 1]]
            assert_same_ranking(ow[q, :onw[q]], hits[q, :nh[q]], ref_ext=oix.search_brute(t, k + 300),
                                what=f"q{q} vs wand")
    return hits, nh


def test_c1_1k_docs_3_terms_top10():
    c = make_corpus(1000, 1000, seed=1, length="lognormal", mean_len=100)
    seg, gix, oix = both(c)
    terms, off = make_queries(c, 64, 3, seed=1)
    check_batch(gix, oix, terms, off, 10)


@pytest.mark.parametrize("length,zipf,nterms,k", [
    ("fixed", None, 3, 10), ("lognormal", None, 5, 10), ("mixed", None, 2, 1),
    ("lognormal", 1.0, 10, 100), ("lognormal", 1.0, 4, 7), ("fixed", None, 5, 1000)])
def test_random_corpora(length, zipf, nterms, k):
    c = make_corpus(20000, 2000, seed=7, length=length, mean_len=60, zipf=zipf)
    seg, gix, oix = both(c)
    terms, off = make_queries(c, 48, nterms, seed=9, zipf=zipf)
    check_batch(gix, oix, terms, off, k)


@pytest.mark.parametrize("nterms,k", [(1, 10), (8, 256), (9, 10), (12, 64), (16, 10), (17, 10), (40, 100), (5, 300), (5, 1000)])
def test_kernel_routing_by_term_count(nterms, k):
    """Sparse queries of 1..8 / 9..16 indexed terms (k <= 256) take scan_range_kernel<., 8> / <., 16>; more terms, or
    256 < k <= 1024, scan_many_kernel.  A single-term query is all single-posting documents (the cold pass)."""
    c = make_corpus(150_000, 3000, seed=11, length="lognormal", mean_len=60)
    seg, gix, oix = both(c)
    terms, off = make_queries(c, 24, nterms, seed=5)
    check_batch(gix, oix, terms, off, k, wand=k <= 256)


def test_queries_of_hundreds_of_terms():
    """search.rs:53-79 pushes one Token per found key, without a limit (a tsvector of a whole document): 400 and 1000
    indexed terms through scan_many_kernel (term loops of four per thread); 1025 is the documented limit."""
    c = make_corpus(60_000, 3000, seed=4, length="lognormal", mean_len=80)
    seg, gix, oix = both(c)
    rng = np.random.default_rng(8)
    n_terms = seg.meta()["n_terms"]
    qs = [np.sort(rng.choice(n_terms, n, replace=False)).astype(np.uint32) for n in (400, 1000, 17, 257)]
    terms = np.concatenate(qs)
    off = np.r_[0, np.cumsum([len(q) for q in qs])].astype(np.uint32)
    for k in (10, 300):
        hits, nh = vb.search_batch(gix, terms, off, k)
        for q in range(len(qs)):
            assert_bit_exact(oix.search_brute(qs[q], k), hits[q, :nh[q]], what=f"k={k} q{q} ({len(qs[q])} terms)")
    big = np.sort(rng.choice(n_terms, 1025, replace=False)).astype(np.uint32)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.search_batch(gix, big, np.array([0, 1025], dtype=np.uint32), 10)
    assert e.value.code == -4  # VBM25_ERR_UNSUPPORTED


def test_tiny_and_large_batches_through_batch_run():
    """vbm25_batch_run: a handful of work items takes the one-launch instantiation of scan_range_kernel (device buffers),
    a batch that fills the GPU plan_kernel + scan_range_kernel + merge_kernel; same results either way."""
    c = make_corpus(150_000, 3000, seed=11, length="lognormal", mean_len=60)
    seg, gix, oix = both(c)
    terms, off = make_queries(c, 200, 4, seed=6)
    for nq in (1, 3, 200):
        b = vb.Batch(gix, nq, int(off[nq]), 10)
        b.set_queries(terms[:off[nq]], off[:nq + 1])
        b.run()
        hits, nh = b.fetch()
        for q in range(nq):
            want = oix.search_brute(terms[off[q]:off[q + 1]], 10)
            assert_bit_exact(want, hits[q, :nh[q]], what=f"nq={nq} q{q} vs brute")


def test_route_transitions_on_one_handle():
    """The three routes of a batch of sparse queries -- plan-free (every query sparse, many items), one-launch (a handful of
    items; pinned through vbm25_search_batch, device buffers through vbm25_batch_run) and general (plan_kernel: a many-term
    query in the batch) -- in every order on ONE batch object and ONE search handle, on memory that was not zero when it was
    allocated: each route has to leave the per-launch state as every other route expects to find it."""
    c = make_corpus(150_000, 3000, seed=14, length="lognormal", mean_len=60)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    _dirty_the_allocator()
    gix = vb.GpuIndex(seg)
    rng = np.random.default_rng(9)
    n_terms = seg.meta()["n_terms"]
    big_t, big_o = make_queries(c, 300, 4, seed=21)          # plan-free route
    few_t, few_o = make_queries(c, 3, 4, seed=22)            # one-launch route
    many = np.sort(rng.choice(n_terms, 30, replace=False)).astype(np.uint32)
    gen_t = np.r_[big_t[:big_o[40]], many].astype(np.uint32)  # general route: 40 sparse queries + one of 30 terms
    gen_o = np.r_[big_o[:41], big_o[40] + 30].astype(np.uint32)
    shapes = {"free": (big_t, big_o), "one": (few_t, few_o), "gen": (gen_t, gen_o)}
    want = {}
    for name, (t, o) in shapes.items():
        want[name] = [oix.search_brute(t[o[q]:o[q + 1]], 10) for q in range(len(o) - 1)]

    def check(name, hits, nh):
        for q, w in enumerate(want[name]):
            assert_bit_exact(w, hits[q, :nh[q]], what=f"{name} q{q}")

    order = ["free", "one", "free", "gen", "one", "gen", "free", "one", "one", "gen", "free"]
    b = vb.Batch(gix, 300, int(max(big_o[-1], gen_o[-1])), 10)
    for name in order:  # vbm25_batch_run (device buffers)
        t, o = shapes[name]
        b.set_queries(t, o)
        b.run()
        check(name, *b.fetch())
    for name in order:  # vbm25_search_batch (its cached batch object; the one-launch route writes to pinned memory)
        t, o = shapes[name]
        check(name, *vb.search_batch(gix, t, o, 10))


def test_mixed_batch_all_kernels():
    """One batch whose queries are spread over scan_range_kernel (row strides 8 and 16) and scan_many_kernel, with
    unknown tokens and an empty query in between."""
    c = make_corpus(150_000, 3000, seed=12, length="lognormal", mean_len=60)
    seg, gix, oix = both(c)
    rng = np.random.default_rng(3)
    n_terms = seg.meta()["n_terms"]
    sizes = [1, 2, 5, 8, 9, 10, 12, 13, 20, 40, 0, 3, 7, 11, 6, 4]
    qs = []
    for i, n in enumerate(sizes):
        t = np.sort(rng.choice(n_terms, n, replace=False)).astype(np.uint32)
        if i % 5 == 1 and n:
            t = np.r_[t, np.uint32(0xFFFFFFFF)]  # unknown token: ignored (search.rs:59-61)
        qs.append(t.astype(np.uint32))
    terms = np.concatenate(qs).astype(np.uint32)
    off = np.r_[0, np.cumsum([len(q) for q in qs])].astype(np.uint32)
    hits, nh = vb.search_batch(gix, terms, off, 10)
    assert nh[sizes.index(0)] == 0
    for q in range(len(sizes)):
        t = terms[off[q]:off[q + 1]]
        t = t[t != 0xFFFFFFFF]
        want = oix.search_brute(t, 10)
        assert_bit_exact(want, hits[q, :nh[q]], what=f"q{q} ({sizes[q]} terms) vs brute")


def test_fuzz_shape_100_term_queries_top100():
    # tests/fuzz:43-59 shape: 10 000 docs x 100 draws of 10 000 tokens, ~100-term queries
    c = make_corpus(10000, 10000, seed=11, length="fixed", mean_len=100)
    seg, gix, oix = both(c)
    terms, off = make_queries(c, 16, 100, seed=5)
    check_batch(gix, oix, terms, off, 100)
    # 250- and 300-term queries (the GPU path's limit is 1024 indexed terms; the error beyond it is covered by
    # test_queries_of_hundreds_of_terms)
    terms, off = make_queries(c, 4, 250, seed=6)
    check_batch(gix, oix, terms, off, 20, wand=False)
    t = np.arange(300, dtype=np.uint32)
    check_batch(gix, oix, t, np.array([0, 300], dtype=np.uint32), 5, wand=False)


def test_edge_cases():
    c = make_corpus(3000, 300, seed=3, length="lognormal", mean_len=50)
    seg, gix, oix = both(c)
    nt = gix.n_terms
    df = seg.arrays()["term_df"]
    rare = int(np.argmin(df))
    terms = np.array([
        # empty | unknown only | known+unknown | rare | all-known pair
        nt + 7, 3, nt + 9, rare, 5, 6], dtype=np.uint32)
    off = np.array([0, 0, 1, 3, 4, 6], dtype=np.uint32)
    hits, nh = check_batch(gix, oix, terms, off, 10)
    assert nh[0] == 0 and nh[1] == 0 and nh[2] == 10
    # k larger than the number of matches: every matching doc comes back, sorted
    hits, nh = check_batch(gix, oix, np.array([rare], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), 1000)
    assert nh[0] == df[rare]
    # k == 0 is the reference's "number of needed rows is set to 0" error (default.rs:114-116)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.search_batch(gix, np.array([1], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), 0)
    assert e.value.code == -1
    with pytest.raises(vb.Vbm25Error):  # not strictly ascending (Query::new)
        vb.search_batch(gix, np.array([5, 5], dtype=np.uint32), np.array([0, 2], dtype=np.uint32), 5)
    with pytest.raises(vb.Vbm25Error) as e:  # beyond bm25.limit's maximum (gucs.rs:37-46)
        vb.search_batch(gix, np.array([5], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), 65536)
    assert e.value.code == -1


def test_codec_corner_case_index():
    # bitwidth-32 raw block, df == 128 exactly, single posting, 4-byte tf (see test_segment_builder)
    n_docs = 3_000_000
    docs_a = np.r_[np.arange(64), 2_900_000 + np.arange(64) * 3].astype(np.uint32)
    docs_b = (np.arange(128) * 7 + 5).astype(np.uint32)
    docs_c = np.array([123456], dtype=np.uint32)
    docs_d = (np.arange(300) * 9000 + 17).astype(np.uint32)
    rng = np.random.default_rng(0)
    post_tf = np.r_[np.ones(128), rng.integers(1, 70000, 128), [1 << 30], rng.integers(1, 4, 300)].astype(np.uint32)
    keys = np.zeros((4, 16), dtype=np.uint8)
    keys[:, 0] = [ord("a"), ord("b"), ord("c"), ord("d")]
    rng = np.random.default_rng(1)
    seg = vb.Segment.build(1.2, 0.75, rng.integers(1, 3000, n_docs).astype(np.uint32),
                           np.zeros((n_docs, 3), dtype=np.uint16), keys,
                           np.array([0, 128, 256, 257, 557], dtype=np.uint64),
                           np.r_[docs_a, docs_b, docs_c, docs_d], post_tf)
    seg, gix, oix = both(seg=seg)
    terms = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 3], dtype=np.uint32)
    off = np.array([0, 1, 2, 3, 4, 8, 10], dtype=np.uint32)
    check_batch(gix, oix, terms, off, 10)
    check_batch(gix, oix, terms, off, 300)


def test_sqllogictest_golden_orders_on_gpu():
    from test_oracle_pins import _slt_index
    fixture = json.load(open(os.path.join(GOLD, "slt_corpus.json")))
    for case in fixture["expect"]:
        sel = {"all": range(1, 11), "even": range(2, 11, 2), "odd": range(1, 11, 2)}[case["ids"]]
        oix, q, ids = _slt_index(set(sel), fixture)
        desc, keep = vb.api.desc_from_arrays(
            dict(n_docs=oix.n_docs, n_terms=oix.n_terms, n_blocks=oix.n_blocks, sum_len=oix.sum_len,
                 k1=oix.k1, b=oix.b), oix.arrays)
        gix = vb.GpuIndex(desc)
        # through the reference-shaped entry point: Query of interned lexemes -> search()
        hits = vb.search(gix, case["k"], vb.Query.from_tokens([t.encode() for t in fixture["query"]]))
        assert [int(h["payload"][2]) for h in hits] == case["order"], case["name"]


def test_c2_1m_docs_single_3_term_query_top10():
    seg = vb.Segment.synth(1_000_000, 30000, mean_len=100, len_mode=1, seed=20260925)
    seg, gix, oix = both(seg=seg)
    rng = np.random.default_rng(1)
    for _ in range(4):
        toks = rng.choice(30000, 3, replace=False).astype(np.uint32)
        t = np.sort(seg.token_terms(toks))
        check_batch(gix, oix, t, np.array([0, 3], dtype=np.uint32), 10)
    # a batch on the same index (C3 shape at 1/10 of the documents)
    toks = np.stack([rng.choice(30000, 5, replace=False) for _ in range(256)]).astype(np.uint32)
    t = np.sort(seg.token_terms(toks.reshape(-1)).reshape(256, 5), axis=1).reshape(-1)
    check_batch(gix, oix, t, (np.arange(257) * 5).astype(np.uint32), 10, wand=False)


def test_properties_idempotent_sorted_batch_invariant():
    seg = vb.Segment.synth(2_000_000, 30000, mean_len=100, len_mode=1, seed=5)
    _dirty_the_allocator()
    gix = vb.GpuIndex(seg)
    rng = np.random.default_rng(2)
    nq = 512
    toks = np.stack([rng.choice(30000, 5, replace=False) for _ in range(nq)]).astype(np.uint32)
    t = np.sort(seg.token_terms(toks.reshape(-1)).reshape(nq, 5), axis=1).reshape(-1)
    off = (np.arange(nq + 1) * 5).astype(np.uint32)
    h1, n1 = vb.search_batch(gix, t, off, 10)
    h2, n2 = vb.search_batch(gix, t, off, 10)
    assert h1.tobytes() == h2.tobytes() and np.array_equal(n1, n2)
    assert (n1 == 10).all()
    s = h1["score"]
    assert (s[:, :-1] >= s[:, 1:]).all() and (s > 0).all()
    tie = s[:, :-1] == s[:, 1:]
    assert (h1["doc_id"][:, :-1][tie] < h1["doc_id"][:, 1:][tie]).all()
    # a query's result does not depend on what else is in the batch
    sub = [3, 77, 500]
    for q in sub:
        hq, nq1 = vb.search_batch(gix, t[off[q]:off[q + 1]], np.array([0, 5], dtype=np.uint32), 10)
        assert hq[0].tobytes() == h1[q].tobytes()
    # top-10 is a prefix of top-100
    h100, _ = vb.search_batch(gix, t[:50], off[:11], 100)
    assert np.array_equal(h100[:, :10]["doc_id"], h1[:10]["doc_id"])
    # payload is the synthetic ctid of the doc (fetcher.rs:218-225 layout)
    d = h1["doc_id"].astype(np.int64)
    assert np.array_equal(h1["payload"][..., 2], d % 64 + 1)
    assert np.array_equal(h1["payload"][..., 1], (d // 64) & 0xffff)


def test_corrupt_index_is_rejected():
    c = make_corpus(500, 50, seed=2, length="fixed", mean_len=20)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"],
                           c["post_doc"], c["post_tf"])
    arrs = {k: v.copy() for k, v in seg.arrays().items()}
    arrs["blk_max_doc"][0] += 1  # summary disagrees with the block body
    desc, keep = vb.api.desc_from_arrays(seg.meta(), arrs)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.GpuIndex(desc)
    assert e.value.code == -2
    # a WAND pair that does not bound its block: the scan kernels prune with it, so it is checked
    arrs = {k: v.copy() for k, v in seg.arrays().items()}
    arrs["blk_wand_tf"][:] = 1
    arrs["blk_wand_fn"][:] = 255  # the longest documents: the smallest score a posting can have
    desc, keep = vb.api.desc_from_arrays(seg.meta(), arrs)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.GpuIndex(desc)
    assert e.value.code == -2 and "WAND" in str(e.value)
    arrs = {k: v.copy() for k, v in seg.arrays().items()}
    arrs["term_wand_tf"][:] = 1
    arrs["term_wand_fn"][:] = 255
    desc, keep = vb.api.desc_from_arrays(seg.meta(), arrs)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.GpuIndex(desc)
    assert e.value.code == -2


def test_correlated_terms_spill_and_abort_paths():
    """Terms that co-occur in the same documents: almost every posting of a tile is a second arrival, which exercises
    (a) scan_range_kernel's row overflow (the tile is undone and planned again with half the blocks), (b) its give-up path
    (rows overflow even at one block per term: item_failed, the item is redone by scan_many_kernel) and (c) documents with
    three and more addends."""
    n_docs = 600_000
    rng = np.random.default_rng(42)
    base = np.sort(rng.choice(n_docs, 9000, replace=False)).astype(np.uint32)
    lists = [
        base,                                                     # t0
        base,                                                     # t1: same documents as t0
        np.sort(np.r_[base[::7], rng.choice(n_docs, 6000, replace=False)]).astype(np.uint32),  # t2: 1/7 of t0 + noise
        np.sort(np.r_[base[::3], rng.choice(n_docs, 2000, replace=False)]).astype(np.uint32),  # t3: 1/3 of t0 + noise
        np.sort(rng.choice(n_docs, 7000, replace=False)).astype(np.uint32),                     # t4: independent
    ]
    lists = [np.unique(l) for l in lists]
    keys = np.zeros((len(lists), 16), dtype=np.uint8)
    keys[:, 0] = np.arange(len(lists)) + ord("a")
    term_start = np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.uint64)
    post_doc = np.concatenate(lists)
    post_tf = rng.integers(1, 4, len(post_doc)).astype(np.uint32)
    seg = vb.Segment.build(1.2, 0.75, rng.integers(5, 400, n_docs).astype(np.uint32),
                           np.zeros((n_docs, 3), dtype=np.uint16), keys, term_start, post_doc, post_tf)
    seg, gix, oix = both(seg=seg)
    queries = [[0, 1], [0, 2], [0, 3], [0, 1, 2, 3], [0, 1, 2, 3, 4], [2, 3, 4], [1, 4], [0, 2, 4]]
    terms = np.array([t for q in queries for t in q], dtype=np.uint32)
    off = np.r_[0, np.cumsum([len(q) for q in queries])].astype(np.uint32)
    for k in (10, 100):
        check_batch(gix, oix, terms, off, k)


def test_growing_segment_merged_with_device_hits():
    """The shim's full result: sealed hits from the device + unsealed documents scored on the host
    (vbm25_growing_search) + vbm25_merge_hits, against the oracle's search with a growing segment."""
    c = make_corpus(30_000, 800, seed=31, length="lognormal", mean_len=50)
    seg, gix, oix = both(c)
    a = seg.arrays()
    n_terms = seg.meta()["n_terms"]
    terms, off = make_queries(c, 10, 4, seed=2)
    rng = np.random.default_rng(8)
    for q in range(len(off) - 1):
        t = terms[off[q]:off[q + 1]]
        t = t[t < n_terms]
        starts, ranks, keys, tfs = [0], [], [], []
        for _ in range(40):
            own = sorted(set(rng.choice(n_terms, 6, replace=False).tolist()) |
                         set(rng.choice(t, rng.integers(0, len(t) + 1), replace=False).tolist()))
            for r in own:
                ranks.append(r)
                keys.append(a["term_key"][r].tobytes())
                tfs.append(int(rng.integers(1, 5)))
            starts.append(len(ranks))
        fn = rng.integers(0, 100, 40).astype(np.uint8)
        pl = rng.integers(0, 60000, (40, 3)).astype(np.uint16)
        dl = (rng.random(40) < 0.2).astype(np.uint8)
        query = vb.Query([a["term_key"][r].tobytes() for r in t])
        gkeys = np.frombuffer(b"".join(keys), np.uint8)
        for k in (3, 25):
            sealed, n = vb.search_batch(gix, t, np.array([0, len(t)], np.uint32), k)
            grow = vb.growing_search(seg, query, k, starts, gkeys, tfs, fn, pl, dl)
            merged = vb.merge_hits(sealed[0, :n[0]], grow, k)
            ref = oix.search_wand_growing(t, k, np.array(starts, np.uint64), np.array(ranks, np.uint32),
                                          np.array(tfs, np.uint32), fn, pl, dl)
            ext = vb.merge_hits(oix.search_brute(t, k + 300),
                                vb.growing_search(seg, query, k + 300, starts, gkeys, tfs, fn, pl, dl), k + 300)
            assert_same_ranking(ref, merged, ref_ext=ext, what=f"q{q} k={k} growing + device")


def test_index_read_from_reference_format_pages():
    """PostgreSQL-page relation (oracle/pages.cpp, the reference's on-disk layout) -> page reader ->
    HBM -> search, with unsealed documents from the same relation merged on the host."""
    c = make_corpus(12_000, 600, seed=17, length="lognormal", mean_len=40)
    seg0, _, oix = both(c)
    pages = orc.Pages(oix)
    a = seg0.arrays()
    rng = np.random.default_rng(6)
    n_terms = seg0.meta()["n_terms"]
    grow_docs = []
    for _ in range(25):
        ranks = np.sort(rng.choice(n_terms, int(rng.integers(1, 30)), replace=False))
        tfs = rng.integers(1, 5, len(ranks)).astype(np.uint32)
        pages.insert(rng.integers(0, 60000, 3).astype(np.uint16), [a["term_key"][r].tobytes() for r in ranks], tfs)
        grow_docs.append((ranks, tfs))
    pl = [pages.page(i) for i in range(len(pages))]
    seg = vb.segment_from_pages(pl)
    g = vb.growing_from_pages(pl)
    gix = vb.GpuIndex(seg)
    terms, off = make_queries(c, 16, 4, seed=4)
    check_batch(gix, oix, terms, off, 10)
    # with the growing segment: oracle takes term ranks for the unsealed documents
    g_rank = np.concatenate([r for r, _ in grow_docs]).astype(np.uint32)
    for q in range(len(off) - 1):
        t = terms[off[q]:off[q + 1]]
        t = t[t < n_terms]
        query = vb.Query([a["term_key"][r].tobytes() for r in t])
        sealed, n = vb.search_batch(gix, t, np.array([0, len(t)], np.uint32), 10)
        merged = vb.merge_hits(sealed[0, :n[0]], vb.growing_search(seg, query, 10, **g), 10)
        ref = oix.search_wand_growing(t, 10, g["g_start"], g_rank, g["g_tf"], g["g_fieldnorm"], g["g_payload"], g["g_deleted"])
        ext = vb.merge_hits(oix.search_brute(t, 310), vb.growing_search(seg, query, 310, **g), 310)
        assert_same_ranking(ref, merged, ref_ext=ext, what=f"q{q} pages + growing")


def test_bench_distributed_code_path_single_rank():
    """bench.py's N>1 code path (RCCL init, segment hand-over through /dev/shm, device-buffer
    view for torch, all-gather of the hit records) with one rank on the one GPU of this box."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VBM25_BENCH_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--workload", "C2",
                                   "--queries", "64", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full"],
                                  env=env, text=True, timeout=600)
    line = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["roofline"]["frac"] > 0
    cfg = line["config"]  # the gather runs on its own stream: what of it is left after the last scan is reported apart
    assert cfg["gather_ms"] > 0 and 0 <= cfg["gather_exposed_ms"] <= line["ms_per_step"]


def test_bench_dump_outputs_are_the_last_steps_hits(tmp_path):
    """bench.py --dump-outputs DIR: the hits of the last timed step (batch (steps - 1) % batches, made from the bench's own seeds)
    as float64 / float32 .npy files, equal to the oracle's brute force on the same corpus and queries."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from bench import WORKLOADS, make_queries as bench_queries
    out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--workload", "C1", "--steps", "3",
                                   "--warmup", "1", "--no-cpu-baseline", "--extra-budget-s", "0", "--dump-outputs", str(tmp_path)],
                                  text=True, timeout=600)
    line = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("score", "doc_id", "payload", "n_hits")}
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{n}.npy" for n in got)
    assert [got[n].dtype for n in ("score", "doc_id", "payload", "n_hits")] == [np.float64, np.float64, np.float32, np.float64]
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C1"]
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    terms, off = bench_queries(dseg, vocab, nq, nterms, seed=1 + 2, zipf_s=zipf_s)  # step 2 of 3 runs batch 2 of 4
    seg = dseg.download()
    ref, n_ref, _ = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays()).search_batch(terms, off, k, mode="brute", threads=4)
    assert np.array_equal(got["n_hits"], n_ref) and n_ref.sum() > 0
    for q, n in enumerate(n_ref):
        assert np.array_equal(got["score"][q, :n].view(np.uint64), ref["score"][q, :n].view(np.uint64)), f"q{q}: score bits differ"
        assert np.array_equal(got["doc_id"][q, :n], ref["doc_id"][q, :n]), f"q{q}: doc ids differ"
        assert np.array_equal(got["payload"][q, :n], ref["payload"][q, :n]), f"q{q}: payloads differ"


def test_bench_full_adds_what_the_headline_does_not_need():
    """A plain bench.py run prints the headline figure alone; --full adds the one-stream-per-batch figure, the 64-query parity
    sample and the CPU baseline to the same line."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for mode in ([], ["--full"]):
        out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--workload", "C1", "--steps", "3",
                                       "--warmup", "1", *mode], text=True, timeout=600)
        lines[bool(mode)] = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    for line in lines.values():
        assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["roofline"]["kernel_ms"] > 0
        assert line["config"]["host_buffer_inclusive_qps_per_gpu"] > 0  # (the pre-timed launches: in every run)
    plain, full = lines[False], lines[True]
    assert "cpu_baseline" not in plain and "verified_sample" not in plain["config"]
    assert plain["config"]["resident_one_stream_per_batch_qps_per_gpu"] is None
    assert full["cpu_baseline"]["value"] > 0 and full["config"]["verified_sample"]["bit_exact_vs_oracle_brute_force"]
    assert full["config"]["resident_one_stream_per_batch_qps_per_gpu"] > 0


def test_c3_full_size_full_batch_parity():
    """BASELINE config C3 at full size (10M docs / 30k vocab, 5-term queries, top-10): ALL 1024 of the
    bench's own queries bit-exact against the oracle's brute force, a sample against the faithful
    Block-WAND restatement, plus batch invariance; no work item of the batch is served by the fallback kernel."""
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import make_queries as bench_queries, usable_cpus
    # (the bench's own corpus: generated, flushed and indexed ON THE DEVICE -- the oracle gets the segment's download)
    dseg = vb.DeviceSegment.synth(10_000_000, 30000, mean_len=100, len_mode=1, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    terms, off = bench_queries(dseg, 30000, 1024, 5, seed=1, zipf_s=0.0)
    seg = dseg.download()
    b = vb.Batch(gix, 1024, len(terms), 10)  # (the bench's own object and call sequence)
    b.set_queries(terms, off)
    assert b.debug_route() == 3, "the bench line would not be scan_win_kernel's"
    b.set_queries(terms, off)
    b.run()
    hits, nh = b.fetch()
    items, failed = b.debug_counts()
    assert failed == 0, f"{failed} of {items} work items fell back to scan_many_kernel: the bench line would not be scan_win_kernel's"
    assert (nh == 10).all()
    h1, n1 = vb.search_batch(gix, terms, off, 10)
    assert h1.tobytes() == hits.tobytes() and np.array_equal(n1, nh)
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    t0 = time.perf_counter()
    ob, onb, _ = oix.search_batch(terms, off, 10, mode="brute", threads=usable_cpus())
    assert time.perf_counter() - t0 < 60.0, "the full-batch check must stay cheap"
    assert np.array_equal(nh, onb)
    for q in range(1024):
        assert_bit_exact(ob[q, :onb[q]], hits[q, :nh[q]], what=f"q{q} vs brute")
    sample = list(range(0, 1024, 37))
    st = np.concatenate([terms[off[q]:off[q + 1]] for q in sample])
    so = (np.arange(len(sample) + 1) * 5).astype(np.uint32)
    ow, onw, _ = oix.search_batch(st, so, 10, mode="wand", threads=usable_cpus())
    for i, q in enumerate(sample):
        assert_same_ranking(ow[i, :onw[i]], hits[q, :nh[q]], ref_ext=oix.search_brute(st[so[i]:so[i + 1]], 300),
                            what=f"q{q} vs wand")
    # the sampled queries alone give the same records as inside the 1024-query batch
    h2, n2 = vb.search_batch(gix, st, so, 10)
    for f in ("score", "doc_id", "payload"):
        assert np.array_equal(h2[f], hits[sample][f]), f


def test_c3z_full_size_full_batch_parity():
    """C3's shape over a Zipf(1) vocabulary at full size (bench.py --workload C3z: 10 M documents, 30 k tokens, 1024 five-term queries
    whose tokens follow the same law, top-10) -- a batch of dense and sparse queries on the general route (plan_kernel; scan_dense_kernel
    for the queries with a head term, scan_range_kernel for the others): ALL 1024 queries bit-exact against the oracle's brute force,
    no work item served by the fallback kernel, a sample against the faithful Block-WAND restatement."""
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import WORKLOADS, make_queries as bench_queries, usable_cpus
    n_docs, vocab, mean_len, len_mode, zipf_s, nq, nterms, k = WORKLOADS["C3z"]
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    terms, off = bench_queries(dseg, vocab, nq, nterms, seed=1, zipf_s=zipf_s)
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_queries(terms, off)
    assert b.debug_route() == 0, "a batch with dense queries takes the general route"
    b.run()
    hits, nh = b.fetch()
    items, failed = b.debug_counts()
    assert failed == 0, f"{failed} of {items} work items fell back to scan_many_kernel"
    r = b.debug_routes()
    assert r[0] + r[1] == nq and r[1] > 0 and r[3] + r[4] == items and r[4] > 0, r
    assert (nh == k).all()
    seg = dseg.download()
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    t0 = time.perf_counter()
    ob, onb, _ = oix.search_batch(terms, off, k, mode="brute", threads=usable_cpus())
    assert time.perf_counter() - t0 < 300.0, "the full-batch check must stay affordable"
    assert np.array_equal(nh, onb)
    for q in range(nq):
        assert_bit_exact(ob[q, :onb[q]], hits[q, :nh[q]], what=f"C3z q{q} vs brute")
    sample = list(range(0, nq, 64))
    st = np.concatenate([terms[off[q]:off[q + 1]] for q in sample])
    so = (np.arange(len(sample) + 1) * nterms).astype(np.uint32)
    ow, onw, _ = oix.search_batch(st, so, k, mode="wand", threads=usable_cpus())
    for i, q in enumerate(sample):
        assert_same_ranking(ow[i, :onw[i]], hits[q, :nh[q]], ref_ext=oix.search_brute(st[so[i]:so[i + 1]], 300), what=f"C3z q{q} vs wand")


@pytest.mark.parametrize("n_docs,vocab,nq,nterms,k", [(300_000, 20_000, 96, 10, 100), (1_000_000, 50_000, 64, 6, 10)])
def test_maxscore_split_zipf(tuning, n_docs, vocab, nq, nterms, k):
    """Zipf(1) queries through scan_range_kernel's MaxScore split (tuning(dense_x1000=...) declares nothing dense:
    non-essential lists looked up instead of scanned, tile retries; the items it gives up go to scan_many_kernel): same
    records as the default route (scan_dense_kernel), as without the split, and as the oracle."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import make_queries as bench_queries
    seg = vb.Segment.synth(n_docs, vocab, mean_len=100, len_mode=1, zipf_s=1.0, seed=3)
    gix = vb.GpuIndex(seg)
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    terms, off = bench_queries(seg, vocab, nq, nterms, seed=5, zipf_s=1.0)
    h_ex, n_ex = vb.search_batch(gix, terms, off, k)
    for ne in (1, 0):
        tuning(dense_x1000=10 ** 9, ne=ne)  # read when a batch object is created
        b = vb.Batch(gix, nq, len(terms), k)
        b.set_queries(terms, off)
        b.run()
        h_ne, n_ne = b.fetch()
        assert np.array_equal(n_ne, n_ex)
        for q in range(nq):
            assert h_ne[q, :n_ne[q]].tobytes() == h_ex[q, :n_ex[q]].tobytes(), (ne, q)
    ob, onb, _ = oix.search_batch(terms, off, k, mode="brute", threads=8)
    for q in range(nq):
        assert_bit_exact(ob[q, :onb[q]], h_ne[q, :n_ne[q]], what=f"q{q} vs brute")


def test_c5_full_size_sample_parity(tuning):
    """BASELINE config C5 at full size (50M docs / 100k vocab Zipf(1), 10-term queries, top-100): the bench's
    batch of 1024 runs on scan_dense_kernel (the default route); 32 of its queries bit-exact against the oracle's
    brute force and ranking-equal to the faithful Block-WAND restatement; the exhaustive scan_many_kernel gives the
    same records on 16 of them."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import make_queries as bench_queries, usable_cpus
    seg = vb.Segment.synth(50_000_000, 100_000, mean_len=100, len_mode=1, zipf_s=1.0, seed=20260925,
                           threads=usable_cpus())
    gix = vb.GpuIndex(seg)
    terms, off = bench_queries(seg, 100_000, 1024, 10, seed=1, zipf_s=1.0)
    hits, nh = vb.search_batch(gix, terms, off, 100)
    assert (nh == 100).all()
    s = hits["score"]
    assert (s[:, :-1] >= s[:, 1:]).all()
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    ns = 32
    ob, onb, _ = oix.search_batch(terms[:off[ns]], off[:ns + 1], 100, mode="brute", threads=usable_cpus())
    ow, onw, _ = oix.search_batch(terms[:off[ns]], off[:ns + 1], 100, mode="wand", threads=usable_cpus())
    for q in range(ns):
        assert_bit_exact(ob[q, :onb[q]], hits[q, :nh[q]], what=f"q{q} vs brute")
        assert_same_ranking(ow[q, :onw[q]], hits[q, :nh[q]], ref_ext=oix.search_brute(terms[off[q]:off[q + 1]], 400),
                            what=f"q{q} vs wand")
    tuning(dense=0)  # the exhaustive kernel
    b = vb.Batch(gix, 16, int(off[16]), 100)
    b.set_queries(terms[:off[16]], off[:17])
    b.run()
    h3, n3 = b.fetch()
    assert h3.tobytes() == hits[:16].tobytes() and np.array_equal(n3, nh[:16])


def test_evaluate_batch_on_the_device_matches_the_oracle_bitwise():
    """vbm25_evaluate_batch (seq-scan `<&>`, evaluate.rs:22-74, many documents x one query on the device)
    against the oracle's restatement and the host's single-pair vbm25_evaluate, bit for bit."""
    c = make_corpus(3000, 400, seed=13, length="lognormal", mean_len=40)
    seg, gix, oix = both(c)
    a = seg.arrays()
    n_terms = seg.meta()["n_terms"]
    rng = np.random.default_rng(4)
    for trial in range(4):
        q_rank = np.sort(rng.choice(n_terms, int(rng.integers(1, 9)), replace=False)).astype(np.uint32)
        q_ids = q_rank
        if trial == 1:
            q_ids = np.r_[q_rank, np.uint32(0xFFFFFFFF)]  # an unknown query token, last in key order
        if trial == 3:  # ... and in the middle and in front (ids follow key order, unknown ones stay where they sorted)
            mid = len(q_rank) // 2
            q_ids = np.r_[np.uint32(0xFFFFFFFF), q_rank[:mid], np.uint32(0xFFFFFFFF), q_rank[mid:]].astype(np.uint32)
        docs_t, docs_f, start = [], [], [0]
        for i in range(500):
            d_rank = np.sort(rng.choice(n_terms, int(rng.integers(0, 40)), replace=False)).astype(np.uint32)
            if len(d_rank) and rng.random() < 0.7:
                d_rank = np.unique(np.r_[d_rank, rng.choice(q_rank, min(3, len(q_rank)), replace=False)]).astype(np.uint32)
            d_tf = rng.integers(1, 2000 if rng.random() < 0.1 else 6, len(d_rank)).astype(np.uint32)
            docs_t.append(d_rank)
            docs_f.append(d_tf)
            start.append(start[-1] + len(d_rank))
        got = vb.evaluate_batch(gix, q_ids, np.array(start, dtype=np.uint64), np.concatenate(docs_t), np.concatenate(docs_f))
        for i in range(500):
            want = orc.lib().orc_score_to_f64(oix.evaluate(docs_t[i], docs_f[i], q_rank))
            assert got[i] == want, (trial, i)
        assert (got > 0).sum() > 100
    one_doc = (np.array([0, 1], dtype=np.uint64), np.array([5], dtype=np.uint32), np.array([1], dtype=np.uint32))
    assert vb.evaluate_batch(gix, np.array([5, 0xFFFFFFFF, 7], dtype=np.uint32), *one_doc)[0] > 0
    with pytest.raises(vb.Vbm25Error):  # known ids out of order around an unknown one are still rejected
        vb.evaluate_batch(gix, np.array([7, 0xFFFFFFFF, 5], dtype=np.uint32), *one_doc)
    # an element whose key is not in the index still counts for the document's length (vector.rs:77-83)
    k3 = np.array([3], dtype=np.uint32)
    s_known = vb.evaluate_batch(gix, k3, np.array([0, 1], dtype=np.uint64), k3, np.array([2], dtype=np.uint32))[0]
    s_longer = vb.evaluate_batch(gix, k3, np.array([0, 2], dtype=np.uint64), np.array([3, 0xFFFFFFFF], dtype=np.uint32),
                                 np.array([2, 500], dtype=np.uint32))[0]
    assert 0 < s_longer < s_known
    want = vb.evaluate(seg, [a["term_key"][3].tobytes(), b"zzzzzzzzzzzzzzz\0"], [2, 500], vb.Query([a["term_key"][3].tobytes()]))
    assert s_longer == want


def test_empty_sealed_segment_and_abi_holes():
    """An index over an empty table is valid in the reference (every row still in the growing segment): search
    returns nothing.  NULL term_ids with terms declared is an argument error; a batch may outlive its index."""
    import ctypes as C
    meta = dict(n_docs=0, n_terms=0, n_blocks=0, sum_len=0, k1=1.2, b=0.75)
    arrays = {k: np.zeros(0, dtype=dt) for k, dt in vb.api._DESC_ARRAYS}
    arrays["term_first_block"] = np.zeros(1, dtype=np.uint32)
    arrays["blk_off8"] = np.zeros(1, dtype=np.uint32)
    desc, keep = vb.api.desc_from_arrays(meta, arrays)
    gix = vb.GpuIndex(desc)
    hits, nh = vb.search_batch(gix, np.array([0, 5], dtype=np.uint32), np.array([0, 1, 2], dtype=np.uint32), 10)
    assert nh.tolist() == [0, 0]
    c = make_corpus(500, 50, seed=2, length="fixed", mean_len=20)
    seg, gix2, oix = both(c)
    b = vb.Batch(gix2, 4, 16, 10)
    rc = vb.lib().vbm25_batch_set_queries(b.h, None, np.array([0, 2], dtype=np.uint32).ctypes.data_as(C.c_void_p), 1)
    assert rc == -1
    del gix2  # vbm25_index_destroy before vbm25_batch_destroy
    del b


@pytest.mark.parametrize("k", [1025, 5000, 65535])
def test_k_up_to_bm25_limit_maximum(k):
    """bm25.limit goes up to 65535 (gucs.rs:37-46): beyond 1024 the exhaustive per-query path (accumulate per term
    in key order, stable radix sort of score bits) answers, bit-exact against the oracle's brute force."""
    c = make_corpus(150_000, 3000, seed=11, length="lognormal", mean_len=60)
    seg, gix, oix = both(c)
    terms, off = make_queries(c, 6, 5, seed=5)
    terms = np.r_[terms, np.uint32(0xFFFFFFFF)]  # a last query with an unknown token only: no hits
    off = np.r_[off, np.uint32(len(terms))].astype(np.uint32)
    hits, nh = vb.search_batch(gix, terms, off, k)
    assert nh[-1] == 0
    for q in range(len(off) - 1):
        t = terms[off[q]:off[q + 1]]
        want = oix.search_brute(t[t != 0xFFFFFFFF], k)
        assert_bit_exact(want, hits[q, :nh[q]], what=f"k={k} q{q} vs brute")
    assert nh[:-1].min() > 1024


def test_one_launch_route_of_search_batch(tuning):
    """vbm25_search_batch with at most 8 sparse queries: ONE launch (scan_range_kernel makes the items, the query's last
    workgroup merges, queries / hits in pinned host memory).  Same records as the general route (tuning(fused=0)) and the
    oracle; repeated calls and general-route calls in between find the per-launch state clean; 9 queries take the
    general route; an item the kernel gives up sends the batch to the general route (correlated lists)."""
    c = make_corpus(400_000, 4000, seed=21, length="lognormal", mean_len=70)
    seg, gix, oix = both(c)
    terms, off = make_queries(c, 64, 4, seed=8)
    tuning(fused=0)
    gix0 = vb.GpuIndex(seg)  # its scratch batch is created with the one-launch route off
    ref = {nq: vb.search_batch(gix0, terms[:off[nq]], off[:nq + 1], 10) for nq in (1, 3, 8, 9)}
    tuning(fused=1)
    for rep in range(3):
        for nq in (1, 3, 8, 9, 1):
            hits, nh = vb.search_batch(gix, terms[:off[nq]], off[:nq + 1], 10)
            assert hits.tobytes() == ref[nq][0].tobytes() and np.array_equal(nh, ref[nq][1]), (rep, nq)
            for q in range(nq):
                assert_bit_exact(oix.search_brute(terms[off[q]:off[q + 1]], 10), hits[q, :nh[q]], what=f"nq={nq} q{q}")
        # a general-route batch on the same index in between (its plan_kernel / merge_kernel leave other state behind)
        check_batch(gix, oix, terms, off, 10, wand=False)
    # single queries of different shapes, k up to the register top-k's limit
    for q, k in ((0, 1), (5, 64), (9, 100), (17, 256)):
        t = terms[off[q]:off[q + 1]]
        hits, nh = vb.search_batch(gix, t, np.array([0, len(t)], dtype=np.uint32), k)
        assert_bit_exact(oix.search_brute(t, k), hits[0, :nh[0]], what=f"k={k}")


def test_plane_block_boundaries(tuning):
    """The derived planes (post_rel16: ids relative to min_doc in 16 bits; post_tfn: term frequencies in a byte) serve
    only the blocks that fit them -- full blocks spanning <= 65535 documents / tf fields of <= 7 bits; every other block is
    decoded from the blob.  Blocks exactly on either side of both limits, mixed in one query, through scan_range_kernel
    and (every query declared dense) scan_dense_kernel, against the oracle bit for bit."""
    n_docs = 70_000
    docs_a = np.r_[np.arange(127), 65535].astype(np.uint32)            # span 65535: plane
    docs_b = np.r_[np.arange(1, 128), 65537].astype(np.uint32)          # span 65536: no plane
    docs_c = (3 * np.arange(128)).astype(np.uint32)                     # plane ids, a tf of 128 -> 8-bit tf fields: no tf plane
    docs_d = (2 * np.arange(256)).astype(np.uint32)                     # two full plane blocks, tf up to 127
    docs_e = np.r_[5 * np.arange(128), 60_000 + 7 * np.arange(40)].astype(np.uint32)  # a full block and a byte-packed tail
    rng = np.random.default_rng(9)
    tf_a = rng.integers(1, 4, 128)
    tf_a[[0, 127]] = 127
    tf_c = rng.integers(1, 4, 128)
    tf_c[17] = 128
    tf_d = rng.integers(1, 128, 256)
    tf_d[[3, 200]] = 127
    post_doc = np.r_[docs_a, docs_b, docs_c, docs_d, docs_e]
    post_tf = np.r_[tf_a, rng.integers(1, 4, 128), tf_c, tf_d, rng.integers(1, 300, 168)].astype(np.uint32)
    term_start = np.cumsum([0, 128, 128, 128, 256, 168]).astype(np.uint64)
    keys = np.zeros((5, 16), dtype=np.uint8)
    keys[:, 0] = [ord(x) for x in "abcde"]
    seg = vb.Segment.build(1.2, 0.75, rng.integers(1, 3000, n_docs).astype(np.uint32), np.zeros((n_docs, 3), dtype=np.uint16),
                           keys, term_start, post_doc, post_tf)
    a = seg.arrays()
    assert a["blk_max_doc"][0] - a["blk_min_doc"][0] == 65535 and a["blk_max_doc"][1] - a["blk_min_doc"][1] == 65536
    assert a["blk_meta_tf"][0] == 7 and a["blk_meta_tf"][2] == 8 and a["blk_n"].tolist() == [128, 128, 128, 128, 128, 128, 40]
    gix = vb.GpuIndex(seg)
    oix = orc.OracleIndex.from_arrays(seg.meta(), a)
    terms = np.array([0, 1, 0, 2, 3, 1, 2, 3, 0, 1, 2, 3, 4, 4, 2, 4, 1], dtype=np.uint32)
    off = np.array([0, 2, 5, 7, 8, 13, 14, 16, 17], dtype=np.uint32)
    for dense in (False, True):
        if dense:
            tuning(dense_x1000=0)
        for k in (5, 100, 256):
            check_batch(gix, oix, terms, off, k, wand=False)
        b = vb.Batch(gix, len(off) - 1, len(terms), 10)  # the general route (vbm25_search_batch of eight queries is the one-launch route)
        b.set_queries(terms, off)
        b.run()
        hits, nh = b.fetch()
        ob, onb, _ = oix.search_batch(terms, off, 10, mode="brute", threads=4)
        assert np.array_equal(nh, onb)
        for q in range(len(off) - 1):
            assert_bit_exact(ob[q, :onb[q]], hits[q, :nh[q]], what=f"dense={dense} q{q}")
        assert b.debug_counts()[1] == 0
