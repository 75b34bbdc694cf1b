"""VACUUM's compaction without a GPU: the numpy model of maintain.rs (tests/maintain_model.py) on a hand-sized example pinned to the
reference's text, its output through the host builder against the oracle's flush, and the argument checks of vbm25_index_maintain
that come before any device call."""
import ctypes as C

import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from codec_data import TAIL_DOCS, assert_tail_blocks, build_args, codec_growing, low_lists, tail_lists, wide_tf_tail
from corpus import make_corpus, make_long_corpus
from growing_data import make_growing
from maintain_edge_data import FORMS, U32, growing_form, hand_tf_growing, sparse_corpus, sparse_deletes
from maintain_model import NONE, decode_all_np, key_halves, maintain, make_growing_new_keys
from test_segment_builder import assert_same_index, decode_all


def key(s):
    return np.frombuffer(s.ljust(16, b"\0"), np.uint8)


def hand_segment():
    """apple: doc 0 (tf 3), doc 1 (tf 1); cherry: doc 0 (tf 1), doc 2 (tf 2); kiwi: doc 1 only (tf 2)"""
    term_key = np.stack([key(b"apple"), key(b"cherry"), key(b"kiwi")])
    term_start = np.array([0, 2, 4, 5], np.uint64)
    post_doc = np.array([0, 1, 0, 2, 1], np.uint32)
    post_tf = np.array([3, 1, 1, 2, 2], np.uint32)
    doc_len = np.array([4, 3, 2], np.uint32)  # sums of the tfs
    payload = np.array([[0, 1, 1], [0, 1, 2], [0, 1, 3]], np.uint16)
    return vb.Segment.build(1.2, 0.75, doc_len, payload, term_key, term_start, post_doc, post_tf)


def test_hand_sized_example_pinned_to_maintain_rs():
    seg = hand_segment()
    # doc 1 deleted (DocumentTuple.deleted); one growing document: banana (a key the sealed segment lacks, between apple and
    # cherry) tf 2 and cherry tf 1; a second growing document, deleted
    grow = dict(g_start=np.array([0, 2, 3], np.uint64), g_key=np.concatenate([key(b"banana"), key(b"cherry"), key(b"zebra")]),
                g_tf=np.array([2, 1, 7], np.uint32), g_payload=np.array([[9, 9, 9], [8, 8, 8]], np.uint16),
                g_deleted=np.array([0, 1], np.uint8))
    args, relabel = maintain(seg.arrays(), seg.meta(), np.array([False, True, False]), grow)
    k1, b, doc_len, payload, term_key, term_start, post_doc, post_tf = args
    assert relabel.tolist() == [0, NONE, 1, 2, NONE]
    # maintain.rs:344-362: a kept sealed document's length is the number of its postings -- doc 0 holds apple tf 3 and cherry tf 1:
    # length 2, not 4; the growing document keeps Document::length() = 2 + 1
    assert doc_len.tolist() == [2, 1, 3]
    assert payload.tolist() == [[0, 1, 1], [0, 1, 3], [9, 9, 9]]
    # kiwi (held only by the deleted document) is gone, zebra (a deleted growing document's) never comes; banana sorts between
    assert [bytes(k).rstrip(b"\0") for k in term_key] == [b"apple", b"banana", b"cherry"]
    assert term_start.tolist() == [0, 1, 2, 5]
    assert post_doc.tolist() == [0, 2, 0, 1, 2] and post_tf.tolist() == [3, 2, 1, 2, 1]
    out = vb.Segment.build(*args)
    assert out.n_docs == 3 and out.desc.sum_len == 6
    # the fieldnorm of doc 0 is recomputed from 2, not 4
    L = orc.lib()
    assert out.arrays()["doc_fieldnorm"].tolist() == [L.orc_length_to_fieldnorm(x) for x in (2, 1, 3)]
    assert L.orc_length_to_fieldnorm(2) != L.orc_length_to_fieldnorm(4)


def test_packed_words_and_flags_agree():
    c = make_corpus(700, 40, seed=3, length="lognormal", mean_len=20)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    flags = np.random.default_rng(1).random(700) < 0.3
    words = np.zeros(11, np.uint64)
    for d in np.flatnonzero(flags):
        words[d // 64] |= np.uint64(1) << np.uint64(d % 64)
    a1, r1 = maintain(seg.arrays(), seg.meta(), flags)
    a2, r2 = maintain(seg.arrays(), seg.meta(), words)
    assert np.array_equal(r1, r2) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a1, a2))


EDGE_PARAMS = [(1.2, 0.0), (2.0, 1.0), (1.6, 0.5)]


@pytest.mark.parametrize("seed,frac,grow", [(1, 0.0, False), (2, 0.01, True), (3, 0.5, True), (4, 0.99, False), (5, 0.3, "new")]
                         + [(6 + i, None, g) for i, g in enumerate(["hand_tf"] + FORMS)])
def test_model_through_the_host_builder_equals_the_oracle_flush(seed, frac, grow):
    """frac None: the inputs of tests/test_gpu_maintain_edges.py at 3000 documents -- sealed documents without a posting (some kept,
    some deleted), growing lengths at and beyond 2^32 - 1 (a tf of 2^32 - 1: a 4-byte tf tail), a growing CSR sliced out of a
    larger one, growing segments all empty, all deleted, without flags, without and with nothing but unknown keys -- at three (k1, b)"""
    if frac is None:
        k1, b = EDGE_PARAMS[seed % 3]
        args, bare = sparse_corpus()
        seg = vb.Segment.build(k1, b, *args)
        deleted = sparse_deletes(bare)
        if grow == "hand_tf":
            G, picked = hand_tf_growing(seg.arrays()["term_key"])
        else:
            G = growing_form(grow, seg.arrays()["term_key"])
    else:
        k1, b = 1.5, 0.6
        c = make_corpus(3000, 150, seed=seed, length="lognormal", mean_len=30, zipf=1.0 if seed % 2 else None)
        seg = vb.Segment.build(k1, b, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
        deleted = np.random.default_rng(seed).random(3000) < frac
        G = None
        if grow is True:
            G, _ = make_growing(seg.arrays()["term_key"], 400, seed=seed)
        elif grow == "new":
            G = make_growing_new_keys(seg.arrays()["term_key"], 400, seed=seed)
    args, relabel = maintain(seg.arrays(), seg.meta(), deleted, G)
    assert args[0] == k1 and args[1] == b
    oix = orc.OracleIndex.build(*args)
    out = vb.Segment.build(*args)
    assert_same_index(out, oix)
    hi, lo = key_halves(args[4])
    assert np.all((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] > lo[:-1])))
    n_grow = 0 if G is None else len(G["g_start"]) - 1
    n_live_g = n_grow if G is None or G["g_deleted"] is None else int((G["g_deleted"] == 0).sum())
    assert len(args[2]) == int((~deleted).sum()) + n_live_g
    assert np.array_equal(np.sort(relabel[relabel != NONE]), np.arange(len(args[2])))
    if frac is None:  # the kept documents without a posting: length 0, fieldnorm code 0
        kept_bare = bare[~deleted[bare]]
        fn = out.arrays()["doc_fieldnorm"]
        assert 0 < len(kept_bare) < len(bare) and np.all(args[2][relabel[kept_bare]] == 0) and np.all(fn[relabel[kept_bare]] == 0)
    if grow == "hand_tf":
        for case, (g, length) in picked.items():
            assert args[2][relabel[3000 + g]] == length, case
        assert sorted(length for _, length in picked.values()) == [U32 - 1, U32, U32, U32]
        assert fn[relabel[3000 + picked["over"][0]]] == 255 and 0x84 in out.arrays()["blk_meta_tf"]
    if grow == "sliced":
        assert G["g_start"][0] != 0 and len(G["g_tf"]) > G["g_start"][-1]
    if grow == "all_empty":
        assert len(G["g_tf"]) == 0 and np.all(fn[-n_grow:] == 0)


def test_model_at_the_widest_tails_equals_the_oracle_flush():
    """The byte-packed tails of tests/test_gpu_codec.py (3-byte deltas, raw absolute 4-byte ids, 2- and 3-byte tfs), a 4-byte tf tail and
    the growing documents of tests/test_gpu_maintain_edges.py behind two lists that end at a low id, on 2^25 + 5000 documents, half
    of the posting-bearing ones deleted: the model decodes them, and what it makes of them is the oracle's flush"""
    lists = tail_lists() + [wide_tf_tail()] + low_lists()
    seg = vb.Segment.build(1.2, 0.75, *build_args(TAIL_DOCS, lists, 1, payload=True))
    a = seg.arrays()
    assert_tail_blocks(a)
    assert a["blk_meta_doc"][a["term_first_block"][5]] == 0x83 and a["blk_meta_tf"][a["term_first_block"][5]] == 0x84
    bearing = np.unique(np.concatenate([np.asarray(d) for d, _ in lists]))
    deleted = np.zeros(TAIL_DOCS, bool)
    deleted[np.random.default_rng(9).choice(bearing, len(bearing) // 2, replace=False)] = True
    args, relabel = maintain(a, seg.meta(), deleted, codec_growing(lists, deleted))
    out = vb.Segment.build(*args)
    assert_same_index(out, orc.OracleIndex.build(*args))
    md, mt = out.arrays()["blk_meta_doc"], out.arrays()["blk_meta_tf"]
    assert 0x83 in md and 0x84 in md and 0x84 in mt and np.any((md < 0x80) & (md >= 20))


@pytest.mark.parametrize("kind", ["lognormal", "widetf", "mixed"])
def test_vectorised_decode_equals_the_oracle_codec(kind):
    """decode_all_np (the host route's CPU decode in tools/maintain_cost.py) against the oracle's per-block codec"""
    if kind == "widetf":
        c = make_long_corpus(8000, 300, seed=2, wide_tf=True)
    else:
        c = make_corpus(15000, 500, seed=4, length=kind, mean_len=40, zipf=1.0 if kind == "mixed" else None)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    want = decode_all(seg.arrays())
    got = decode_all_np(seg.arrays(), chunk=777)
    assert all(np.array_equal(x, y) for x, y in zip(want, got))


def test_maintain_argument_errors_without_a_device():
    """NULL index or NULL out: VBM25_ERR_INVALID before any device call (this machine may have none)."""
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_index_maintain(None, None, None, None, C.byref(out)) == -1
    assert out.value is None  # *out is NULL after a failure
    assert b"index" in L.vbm25_last_error()
    assert L.vbm25_index_maintain(None, None, None, None, None) == -1
    assert b"out" in L.vbm25_last_error()
