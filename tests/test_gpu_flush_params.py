"""The device builders (csrc/flush.hip) on the corpora of test_gpu_bm25_params.py at every parameter pair: every fieldnorm code,
document lengths up to 2^32 - 1 (the sum of lengths beyond 2^32: doc_kernel's 64-bit sum), short documents under a huge mean,
masses of equal block maxima at b = 0 (block_stats_kernel's and term_wand_kernel's first-maximiser tie-break across lanes).  Every
array and meta() byte for byte the host builder's and the oracle's flush; the device-generated corpus at the parameter edges
re-flushed by the oracle and searched in place.  -m gpu only."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from parity import assert_bit_exact
from test_gpu_bm25_params import PARAMS, PIDS, _bench_queries, _corpus, _fieldnorm_coverage, _raw, run_route
from test_gpu_flush import _triples, assert_same_segment
from test_segment_builder import assert_same_index, decode_all

pytestmark = pytest.mark.gpu


def _args(c):
    return c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"]


def _tied_block_maxima(c, seg):
    """blocks whose maximum tf (the block maximum at b = 0, where every document has the same S1) is held by two or more postings
    of different fieldnorms: the WAND pair depends on which of them the tie-break keeps"""
    a = seg.arrays()
    ts = c["term_start"].astype(np.int64)
    term_of = np.repeat(np.arange(len(ts) - 1), np.diff(ts))
    blk = a["term_first_block"].astype(np.int64)[term_of] + (np.arange(len(term_of)) - ts[term_of]) // 128
    tf = c["post_tf"].astype(np.int64)
    mx = np.zeros(seg.n_blocks, np.int64)
    np.maximum.at(mx, blk, tf)
    at_max = tf == mx[blk]
    fn = a["doc_fieldnorm"][c["post_doc"]].astype(np.int64)
    lo = np.full(seg.n_blocks, 256, np.int64)
    hi = np.full(seg.n_blocks, -1, np.int64)
    np.minimum.at(lo, blk[at_max], fn[at_max])
    np.maximum.at(hi, blk[at_max], fn[at_max])
    return int((hi > lo).sum())


@pytest.mark.parametrize("k1,b", PARAMS, ids=PIDS)
@pytest.mark.parametrize("corpus", ["L127", "Lwide", "S", "T"])
def test_device_builders_at_the_parameter_edges(k1, b, corpus):
    c = _raw(corpus)
    host = _corpus(corpus, k1, b)[0]
    assert_same_index(host, orc.OracleIndex.build(k1, b, *_args(c)))
    if corpus in ("L127", "Lwide"):
        _fieldnorm_coverage(host)
        assert host.meta()["sum_len"] > 2 ** 32, "the sum of document lengths fits 32 bits"
    if b == 0.0 and corpus != "Lwide":  # (Lwide: tf log-uniform up to 2^27, no two postings of a block share the maximum)
        assert _tied_block_maxima(c, host) > 0, "no block maximum is tied across fieldnorms"
    assert_same_segment(vb.Segment.build_device(k1, b, *_args(c)), host)
    term, doc, tf = _triples(c)
    perm = np.random.default_rng(len(corpus)).permutation(len(term))
    assert_same_segment(vb.Segment.build_device_unsorted(k1, b, c["doc_len"], c["doc_payload"], c["term_key"], term[perm], doc[perm],
                                                         tf[perm]), host)
    dseg = vb.DeviceSegment.build(k1, b, *_args(c))
    assert (dseg.n_docs, dseg.n_terms, dseg.n_blocks) == (host.n_docs, host.n_terms, host.n_blocks)
    assert_same_segment(dseg.download(), host)


@pytest.mark.parametrize("zipf", [0.0, 1.0])
@pytest.mark.parametrize("k1,b", [(2.0, 1.0), (1.2, 0.0)], ids=["k1=2.0-b=1.0", "k1=1.2-b=0.0"])
def test_device_synth_at_the_parameter_edges(tuning, k1, b, zipf):
    """vbm25_device_segment_synth at the parameter edges: a valid flush (decoded, flushed again by the oracle: the same arrays),
    searched bit-exactly in place on the window route and at k = 300, and the index of DeviceSegment.build of its postings returns
    the records of the index of Segment.build."""
    n_docs, vocab = 200_000, 1500
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=60, len_mode=1, zipf_s=zipf, k1=k1, b=b, seed=9)
    seg = dseg.download()
    a = seg.arrays()
    assert (seg.meta()["k1"], seg.meta()["b"]) == (k1, b)
    docs, tfs, ts = decode_all(a)
    lens = np.zeros(seg.n_docs, dtype=np.int64)
    np.add.at(lens, docs, tfs)
    assert lens.sum() == seg.desc.sum_len
    args = (lens.astype(np.uint32), a["doc_payload"].copy(), a["term_key"].copy(), ts, docs, tfs)
    oix = orc.OracleIndex.build(k1, b, *args)
    assert_same_index(seg, oix)
    # searched where it was made
    terms, off = _bench_queries(seg, vocab, 64, 4, seed=4, zipf_s=zipf)
    run_route(tuning, dseg, oix, terms, off, 10, 3, dict(fused=0, win_force=1, dense_x1000=10 ** 9), expect_failed=None)
    run_route(tuning, dseg, oix, terms, off, 300, 0, {}, expect_failed=None)
    # the index of the device-built segment of the same postings and the index of the host-built one
    vb.reset_tuning()
    g_dev, g_host = vb.GpuIndex(vb.DeviceSegment.build(k1, b, *args)), vb.GpuIndex(vb.Segment.build(k1, b, *args))
    for k in (10, 300):
        h1, n1 = vb.search_batch(g_dev, terms, off, k)
        h2, n2 = vb.search_batch(g_host, terms, off, k)
        assert np.array_equal(n1, n2) and h1.tobytes() == h2.tobytes(), f"k={k}"
        ob, onb, _ = oix.search_batch(terms, off, k, mode="brute", threads=8)
        assert np.array_equal(n1, onb)
        for q in range(len(off) - 1):
            assert_bit_exact(ob[q, :onb[q]], h1[q, :n1[q]], what=f"q{q} k={k}")
