"""vbm25_index_maintain where tests/test_gpu_maintain.py does not reach: every codec width of decode.h through the compaction's count and
scatter passes and through the re-encode of what they wrote, lengths at the clamp, documents without a posting, every legal (k1, b),
the forms a growing segment can arrive in, the empty index as a source, a lineage of compactions, and the second grid-stride pass of
every kernel of maintain.hip that has one.  Every comparison is byte for byte against tests/maintain_model.py put through the host
builder (compact_and_check), searches against the oracle over the downloaded segment.  -m gpu only."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from codec_data import (TAIL_DOCS, WIDTH_DOCS, assert_tail_blocks, assert_width_blocks, build_args, codec_growing, list_keys, low_lists, tail_lists,
                        wide_tf_lists, wide_tf_tail, width_lists)
from filter_remap_model import remap_words
from maintain_edge_data import FORMS, U32, growing_form, hand_tf_growing, sparse_corpus, sparse_deletes
from maintain_model import NONE, key_halves, maintain, make_growing_new_keys
from parity import assert_bit_exact
from test_gpu_bm25_params import PARAMS, PIDS
from test_gpu_maintain import assert_same_segment, build_args as corpus_args, compact_and_check, corpus
from test_segment_builder import decode_all

pytestmark = pytest.mark.gpu

ONE_LAUNCH = 4096 * 256  # threads of the largest launch grid_of (maintain.hip) makes: a loop over more items runs a second pass


def search_check(ds, got, ks, nq=12, seed=0):
    """nq queries of one to three terms on the index of the compacted segment against the oracle's brute force over its download"""
    cix = vb.GpuIndex(ds)
    oix = orc.OracleIndex.from_arrays(got.meta(), got.arrays())
    rng = np.random.default_rng(seed)
    qs = [np.sort(rng.choice(got.n_terms, min(1 + q % 3, got.n_terms), replace=False)) for q in range(nq)]
    terms = np.concatenate(qs).astype(np.uint32)
    off = np.cumsum([0] + [len(q) for q in qs]).astype(np.uint32)
    for k in ks:
        hits, nh = vb.search_batch(cix, terms, off, k)
        ref, nref, _ = oix.search_batch(terms, off, k, mode="brute", threads=8)
        assert np.array_equal(nh, nref), k
        assert nh.max() > 0
        for q in range(nq):
            assert_bit_exact(ref[q, :nref[q]], hits[q, :nh[q]], what=f"k={k} q{q}")


# ---------------------------------------------------------------------------
# 1. codec widths through the compaction
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["tails", "widths"])
def codec_source(request):
    """(name, lists, segment, index) of an index of 2^25 + ... documents: the hand-made lists of tests/test_gpu_codec.py, the tf widths
    they lack (full blocks of 18 .. 31 bits, a 4-byte tail) and two lists that end at a low id.  One source at a time is alive."""
    if request.param == "tails":
        n, lists = TAIL_DOCS, tail_lists() + [wide_tf_tail()] + low_lists()
    else:
        n, lists = WIDTH_DOCS, width_lists(1) + wide_tf_lists(3) + low_lists()
    seg = vb.Segment.build(1.2, 0.75, *build_args(n, lists, 1, payload=True))
    a = seg.arrays()
    first, md, mt = a["term_first_block"], a["blk_meta_doc"], a["blk_meta_tf"]
    if request.param == "tails":
        assert_tail_blocks(a)
        assert md[first[5]] == 0x83 and mt[first[5]] == 0x84 and a["blk_n"][first[5]] == 9
    else:
        assert_width_blocks(a)
        for i, w in enumerate(range(18, 32)):
            assert mt[first[26 + i]] == w and md[first[26 + i]] < 0x80, w
    assert a["blk_max_doc"][first[len(lists) - 2]] < 1000 and a["blk_max_doc"][first[len(lists) - 1]] < 1000
    return request.param, lists, seg, vb.GpuIndex(seg)


@pytest.mark.parametrize("pattern", ["nothing", "all_without_posting", "half_of_the_posting_bearing"])
def test_codec_widths_through_the_compaction(codec_source, pattern):
    name, lists, seg, gix = codec_source
    n = seg.n_docs
    bearing = np.unique(np.concatenate([np.asarray(d) for d, _ in lists]))
    rng = np.random.default_rng(9)
    if pattern == "nothing":  # the same widths come back, re-encoded from the compaction's own scatter
        deleted = None
    elif pattern == "all_without_posting":  # ids collapse, every width shrinks to a few bits
        deleted = np.ones(n, bool)
        deleted[bearing] = False
    else:  # gaps stay wide, tails change length
        deleted = np.zeros(n, bool)
        deleted[rng.choice(bearing, len(bearing) // 2, replace=False)] = True
    G = None if pattern == "all_without_posting" else codec_growing(lists, deleted)
    ds, got, _ = compact_and_check(gix, seg, deleted, G, f"{name} {pattern}")
    a = got.arrays()
    md, mt = a["blk_meta_doc"], a["blk_meta_tf"]
    if pattern == "all_without_posting":
        assert got.n_docs == len(bearing) < (1 << 14)
        assert np.all(md[md < 0x80] <= 14) and np.all(md[md >= 0x80] <= 0x82)
    else:
        assert 0x83 in md and 0x84 in md and 0x84 in mt, (sorted(set(md.tolist())), sorted(set(mt.tolist())))
        assert np.any((md < 0x80) & (md >= 20))
        if pattern == "nothing":  # every source width is an output width
            s = seg.arrays()
            assert set(s["blk_meta_doc"].tolist()) <= set(md.tolist()) and set(s["blk_meta_tf"].tolist()) <= set(mt.tolist())
    search_check(ds, got, (10, 300))


# ---------------------------------------------------------------------------
# 2. parameters, lengths and input forms
# ---------------------------------------------------------------------------
_SPARSE = {}


def sparse_source(k1, b):
    if (k1, b) not in _SPARSE:
        args, bare = sparse_corpus()
        seg = vb.Segment.build(k1, b, *args)
        _SPARSE[(k1, b)] = (seg, vb.GpuIndex(seg), bare)
    return _SPARSE[(k1, b)]


@pytest.mark.parametrize("k1,b", PARAMS, ids=PIDS)
def test_lengths_at_the_clamp_and_documents_without_a_posting(k1, b):
    seg, gix, bare = sparse_source(k1, b)
    n = seg.n_docs
    deleted = sparse_deletes(bare)
    G, picked = hand_tf_growing(seg.arrays()["term_key"])
    ds, got, args = compact_and_check(gix, seg, deleted, G, f"k1={k1} b={b}")
    _, relabel = maintain(seg.arrays(), seg.meta(), deleted, G)
    assert got.meta()["k1"] == seg.meta()["k1"] == k1 and got.meta()["b"] == seg.meta()["b"] == b
    doc_len, fn = args[2], got.arrays()["doc_fieldnorm"]
    for case, (g, length) in picked.items():
        assert relabel[n + g] != NONE and doc_len[relabel[n + g]] == length, case
    assert {int(doc_len[relabel[n + picked[c][0]]]) for c in picked} == {U32 - 1, U32}
    kept_bare = bare[~deleted[bare]]
    assert 0 < len(kept_bare) < len(bare)
    assert np.all(doc_len[relabel[kept_bare]] == 0) and np.all(fn[relabel[kept_bare]] == 0)
    assert np.all(relabel[bare[deleted[bare]]] == NONE)
    assert 0 in fn and 255 in fn and fn[relabel[n + picked["over"][0]]] == 255
    search_check(ds, got, (1, 10, 300, 1500), nq=16, seed=int(10 * k1 + 100 * b))
    # once more from the result: the tfs up to 2^32 - 1 (4-byte tf tails) are now the compaction's own input, the documents without a
    # posting stay at length 0
    assert 0x84 in got.arrays()["blk_meta_tf"]
    again = np.random.default_rng(3).random(got.n_docs) < 0.1
    again[relabel[[n + g for g, _ in picked.values()]]] = False
    ds2, got2, args2 = compact_and_check(vb.GpuIndex(ds), got, again, None, f"k1={k1} b={b}, second round")
    assert U32 in args2[7] and 2 ** 31 in args2[7] and 0x84 in got2.arrays()["blk_meta_tf"]
    assert got2.meta()["k1"] == k1 and got2.meta()["b"] == b


@pytest.mark.parametrize("k1,b", PARAMS, ids=PIDS)
@pytest.mark.parametrize("form", FORMS)
def test_growing_dict_forms(form, k1, b):
    seg, gix, bare = sparse_source(k1, b)
    G = growing_form(form, seg.arrays()["term_key"])
    ds, got, _ = compact_and_check(gix, seg, sparse_deletes(bare), G, form)
    n_kept, n_grow = int((~sparse_deletes(bare)).sum()), len(G["g_start"]) - 1
    if form == "all_deleted":
        assert got.n_docs == n_kept and got.n_terms <= seg.n_terms
    elif form == "all_empty":
        assert got.n_docs == n_kept + n_grow and np.all(got.arrays()["doc_fieldnorm"][n_kept:] == 0)
    elif form == "no_flags":
        assert got.n_docs == n_kept + n_grow
    elif form == "none_unknown":
        assert got.n_terms <= seg.n_terms
    elif form == "all_unknown":
        assert got.n_terms > seg.n_terms


# ---------------------------------------------------------------------------
# 3. starting points and chains
# ---------------------------------------------------------------------------
def test_from_the_empty_index():
    """The first VACUUM of an index created on an empty table: N = T = B = W = 0, only growing documents come in"""
    c = corpus("lognormal", n=2000, seed=2)
    seg = vb.Segment.build(1.6, 0.5, *corpus_args(c))
    ds0 = vb.DeviceSegment.maintain(vb.GpuIndex(seg), np.ones(seg.n_docs, bool), None)
    empty = ds0.download()
    assert (empty.n_docs, empty.n_terms, empty.n_blocks) == (0, 0, 0)
    eix = vb.GpuIndex(ds0)
    hits, nh = vb.search_batch(eix, np.array([0, 1], np.uint32), np.array([0, 1, 2], np.uint32), 5)
    assert nh.tolist() == [0, 0] and not np.frombuffer(hits.tobytes(), np.uint8).any()  # no kernel runs: the records are zeros
    ds, relabel = vb.DeviceSegment.maintain(eix, None, None, return_relabel=True)  # nothing in, nothing out
    assert (ds.n_docs, ds.n_terms, ds.n_blocks, ds.n_postings) == (0, 0, 0, 0) and len(relabel) == 0
    G = make_growing_new_keys(seg.arrays()["term_key"], 500, seed=3)
    live = int((G["g_deleted"] == 0).sum())
    for deleted in (None, np.zeros(0, np.uint64)):
        ds, got, args = compact_and_check(eix, empty, deleted, G, f"from empty, sealed_deleted={deleted!r}")
        assert got.n_docs == live and got.n_terms > 0
        assert got.meta()["k1"] == 1.6 and got.meta()["b"] == 0.5
    search_check(ds, got, (10, 300))


def test_four_rounds_on_one_lineage():
    """Compacting what a compaction made, again and again: each round's download is the model applied to the previous round's"""
    c = corpus("zipf", n=6000, seed=21)
    seg = vb.Segment.build(1.2, 0.75, *corpus_args(c))
    gix = vb.GpuIndex(seg)
    for r in range(4):
        n = seg.n_docs
        rng = np.random.default_rng(50 + r)
        deleted = rng.random(n) < (0.1, 0.3, 0.05, 0.2)[r]
        G = make_growing_new_keys(seg.arrays()["term_key"], 700, seed=60 + r)
        gk = G["g_key"].reshape(-1, 16)
        fresh = (gk[:, 0] == 0x01) & (gk[:, 1] <= 6) & (gk[:, 2:] == 0).all(axis=1)  # (not the earlier rounds', sealed by now)
        gk[fresh, 1] += 100 - 10 * r             # the keys in front of every sealed key: in front of the earlier rounds' too
        gk[gk[:, 0] == 0xFE, 0] = 0xF0 + r       # the keys behind every sealed key: behind the earlier rounds' too
        gone = []
        if r == 1:  # every document of three tokens no growing document brings back: the tokens vanish
            in_g = {bytes(k) for k in gk}
            free = [t for t in range(seg.n_terms) if bytes(seg.arrays()["term_key"][t]) not in in_g]
            docs_, _, ts = decode_all(seg.arrays())
            ts = ts.astype(np.int64)
            for t in (free[0], free[len(free) // 2], free[-1]):
                deleted[docs_[ts[t]:ts[t + 1]]] = True
                gone.append(bytes(seg.arrays()["term_key"][t]))
        args, want_relabel = maintain(seg.arrays(), seg.meta(), deleted, G)
        sealed = {bytes(k) for k in seg.arrays()["term_key"]}
        is_new = np.array([bytes(k) not in sealed for k in args[4]])
        assert is_new[0] and is_new[-1] and is_new[1:-1].any() and not is_new.all(), r  # new keys before, between and after the sealed ones
        if r == 1:
            have = {bytes(k) for k in args[4]}
            assert len(gone) == 3 and not any(k in have for k in gone)
        if r == 2:  # the packed words
            words = np.zeros((n + 63) // 64, np.uint64)
            packed = np.packbits(deleted, bitorder="little")
            words.view(np.uint8)[:len(packed)] = packed
            ds, relabel = vb.DeviceSegment.maintain(gix, words, G, return_relabel=True)
        elif r == 3:  # no relabel asked for
            ds, relabel = vb.DeviceSegment.maintain(gix, deleted, G), None
        else:
            ds, relabel = vb.DeviceSegment.maintain(gix, deleted, G, return_relabel=True)
        got = ds.download()
        assert_same_segment(got, vb.Segment.build(*args), f"round {r}")
        assert relabel is None or np.array_equal(relabel, want_relabel), r
        seg, gix = got, vb.GpuIndex(ds)
    search_check(ds, got, (10, 300))


# ---------------------------------------------------------------------------
# 4. past one launch's threads
# ---------------------------------------------------------------------------
def test_growing_documents_past_one_launch():
    """1.25 M growing documents of two elements, a sealed key and one of 1.15 M new keys: the loops over growing documents, unknown
    elements, merged and final tokens of maintain.hip all run a second pass (the smallest size at which one exists)"""
    c = corpus("zipf", n=3000, seed=31)
    seg = vb.Segment.build(1.2, 0.75, *corpus_args(c))
    gix = vb.GpuIndex(seg)
    keys = seg.arrays()["term_key"]
    T, n = len(keys), seg.n_docs
    n_grow, n_new = 1_250_000, 1_150_000
    rng = np.random.default_rng(8)
    u = np.r_[np.arange(n_new), rng.integers(0, n_new, n_grow - n_new)]  # the last 100 000 documents share keys with earlier ones
    new = keys[u % T].copy()  # a sealed key's first bytes, 0x01, a counter: right behind that sealed key
    z = (new == 0).argmax(axis=1)
    assert z.max() + 5 < 16
    row = np.arange(n_grow)
    new[row, z] = 1
    for j in range(4):
        new[row, z + 1 + j] = (u >> (8 * (3 - j))) & 255
    pair = np.stack([keys[rng.integers(0, T, n_grow)], new], axis=1)
    hi, lo = key_halves(pair.reshape(-1, 16))
    hi, lo = hi.reshape(-1, 2), lo.reshape(-1, 2)
    swap = (hi[:, 1] < hi[:, 0]) | ((hi[:, 1] == hi[:, 0]) & (lo[:, 1] < lo[:, 0]))
    pair[swap] = pair[swap][:, ::-1]
    g_del = (rng.random(n_grow) < 0.02).astype(np.uint8)
    g_del[ONE_LAUNCH - 4:ONE_LAUNCH + 4] = [1, 0, 0, 1, 0, 1, 1, 0]  # deleted flags on both sides of the first pass's end
    g_del[-1] = 0
    payload = np.zeros((n_grow, 3), np.uint16)
    payload[:, :2] = np.arange(n_grow, dtype="<u4").view("<u2").reshape(-1, 2)
    payload[:, 2] = 7
    G = dict(g_start=(2 * np.arange(n_grow + 1)).astype(np.uint64), g_key=pair.reshape(-1), g_tf=rng.integers(1, 6, 2 * n_grow).astype(np.uint32),
             g_fieldnorm=np.zeros(n_grow, np.uint8), g_payload=payload, g_deleted=g_del)
    deleted = rng.random(n) < 0.1
    ds, got, args = compact_and_check(gix, seg, deleted, G, "1.25 M growing documents")
    live = g_del == 0
    n_unknown = int(live.sum())
    n_new_live = len(np.unique(u[live]))
    assert n_unknown > ONE_LAUNCH and n_new_live > ONE_LAUNCH and T + n_new_live > ONE_LAUNCH  # unknown elements, new keys, merged keys
    assert got.n_terms > ONE_LAUNCH  # final tokens
    assert np.bincount(u[live]).max() >= 3
    # the documents of the second pass are live, so their relabel entries, payloads, lengths and postings are among the bytes compared
    n_kept = int((~deleted).sum())
    late = np.flatnonzero(live[ONE_LAUNCH:]) + ONE_LAUNCH
    assert len(late) > 150_000
    late_id = n_kept + np.cumsum(live)[late] - 1
    a = got.arrays()
    assert got.n_docs == n_kept + n_unknown == late_id[-1] + 1
    assert np.array_equal(a["doc_payload"][late_id], payload[late])
    want_len = G["g_tf"].reshape(-1, 2).sum(axis=1)[late]
    assert np.array_equal(args[2][late_id], want_len) and np.all(a["doc_fieldnorm"][late_id] > 0)
    assert int((args[6] >= late_id[0]).sum()) == 2 * len(late)  # two postings each


def test_keep_words_past_one_launch():
    """64 x 1 048 576 + 64 x 3 + 17 documents: the keep words of the relabel (mt_keep_kernel, and filter_remap_kernel's input words)
    run a second pass (the smallest size at which one exists).  Postings, kept and deleted documents in the words at and beyond
    1 048 576, the last document among them; nearly everything deleted, so the output is small.  Then a filter of two bitmaps
    carried across this compaction, with bits in the second-pass words and in the growing part."""
    second = 64 * ONE_LAUNCH
    n = second + 64 * 3 + 17
    rng = np.random.default_rng(12)
    lists = [(np.r_[5, 1000, second - 1, second, second + 70, n - 1], np.r_[1, 2, 3, 70000, 5, 6]),
             (np.unique(np.r_[rng.integers(0, n, 300), second + np.arange(0, 209, 3)]), None),
             (np.arange(second - 100, second + 30), None),  # a full block and a tail across the first pass's end
             (np.r_[7, 8, 9, 64, 4096], None)]
    lists = [(d, rng.integers(1, 9, len(d)) if t is None else t) for d, t in lists]
    seg = vb.Segment.build(1.2, 0.75, *build_args(n, lists, 2, payload=True))
    gix = vb.GpuIndex(seg)
    bearing = np.unique(np.concatenate([d for d, _ in lists]))
    deleted = np.ones(n, bool)
    deleted[bearing[rng.random(len(bearing)) < 0.6]] = False
    deleted[[second, second + 70, n - 1, n - 2, 5]] = False          # kept, with and (n - 2) without a posting
    deleted[second + 200:second + 206] = False                        # kept without a posting, in a second-pass word
    deleted[[second + 3, second + 6, second - 1]] = True              # posting-bearing and deleted
    G = make_growing_new_keys(list_keys(len(lists)), 300, seed=4)
    ds, got, args = compact_and_check(gix, seg, deleted, G, "keep words past one launch")
    n_kept = int((~deleted).sum())
    kept_late = np.flatnonzero(~deleted[second:]) + second
    assert len(kept_late) > 20 and got.n_docs == n_kept + int((G["g_deleted"] == 0).sum())
    late_id = n_kept - len(kept_late) + np.arange(len(kept_late))
    assert np.array_equal(got.arrays()["doc_payload"][late_id][:, :2].copy().view("<u4").ravel(), kept_late)
    assert np.isin(args[6], late_id).sum() > 20  # postings of second-pass documents
    # the filter: bits on kept and on deleted documents everywhere, the second-pass words and the growing documents included
    bits_s = np.zeros((2, n), bool)
    bits_s[0, bearing[::2]] = True
    bits_s[1, bearing[1::3]] = True
    bits_s[0, second:n:2] = True
    bits_s[1, second + 1:n:3] = True
    bits_s[:, n - 1] = True
    bits_g = rng.random((2, 300)) < 0.5
    f = vb.DocFilter(gix, bits_s)
    gs = vb.GrowingSegment(gix, **G)
    f.set_growing(gs, bits_g)
    nix = vb.GpuIndex(ds)
    nf = f.remap(nix, deleted, G["g_deleted"])
    want = remap_words(bits_s, deleted, bits_g, G["g_deleted"])
    assert want.shape == (2, (nix.n_docs + 63) // 64)
    w_late, w_grow = late_id[0] // 64, n_kept // 64
    for i in range(2):
        assert want[i][w_late:w_grow + 1].any() and want[i][w_grow + 1:].any()  # second-pass sealed bits, growing bits
        got_words = nf.read(i)
        assert got_words.tobytes() == want[i].tobytes(), f"bitmap {i} differs at words {np.flatnonzero(got_words != want[i])[:8]}"
