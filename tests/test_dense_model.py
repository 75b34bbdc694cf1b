"""The scheme of the device's dense-window kernel (scan_dense_kernel) checked on the CPU through its scalar
model (oracle/dense_model.inc): 16-bit fixed-point upper-bound sums select, exact f64 sums decide -- the hits must be those
of the canonical brute force for every window size, with and without the MaxScore split / block skipping,
and the skipping must actually skip on a Zipf corpus."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_long_corpus, make_queries, make_short_corpus, make_tie_corpus

PARAMS = [(1.2, 0.0), (1.2, 1.0), (2.0, 0.0), (2.0, 1.0), (1.6, 0.5), (1.2, 0.75)]


def oracle_of(c):
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"],
                           c["post_doc"], c["post_tf"])
    return orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())


@pytest.mark.parametrize("zipf,nterms,k", [(1.0, 10, 100), (1.0, 4, 7), (None, 5, 10), (1.0, 16, 256)])
def test_model_matches_brute_force(zipf, nterms, k):
    c = make_corpus(40000, 3000, seed=7, length="lognormal", mean_len=60, zipf=zipf)
    oix = oracle_of(c)
    terms, off = make_queries(c, 12, nterms, seed=9, zipf=zipf)
    for q in range(len(off) - 1):
        t = terms[off[q]:off[q + 1]]
        ref = oix.search_brute(t, k)
        for wmax, w0, ph in ((16384, 256, 1), (1024, 64, 2), (8192, 0, 0), (512, 512, 1), (4096, 256, 3)):
            got, st = oix.dense_model(t, k, wmax=wmax, w0=w0, phases=ph)
            assert got.tobytes() == ref.tobytes(), (q, wmax, w0, ph)


def test_model_on_sub_ranges_and_ties():
    # identical documents: every score ties; doc-range items must keep the canonical (score desc, id asc) order
    n = 5000
    keys = np.zeros((2, 16), dtype=np.uint8)
    keys[:, 0] = [ord("a"), ord("b")]
    docs = np.arange(n, dtype=np.uint32)
    seg = vb.Segment.build(1.2, 0.75, np.full(n, 10, dtype=np.uint32), np.zeros((n, 3), dtype=np.uint16), keys,
                           np.array([0, n, 2 * n], dtype=np.uint64), np.r_[docs, docs], np.ones(2 * n, dtype=np.uint32))
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    t = np.array([0, 1], dtype=np.uint32)
    ref = oix.search_brute(t, 300)
    got, _ = oix.dense_model(t, 300, wmax=1024, w0=64)
    assert got.tobytes() == ref.tobytes()
    got, _ = oix.dense_model(t, 50, wmax=1024, w0=64, lo=1000, hi=3000)
    assert list(got["doc_id"]) == list(range(1000, 1050))


def test_block_skipping_skips_on_zipf():
    seg = vb.Segment.synth(300_000, 30_000, mean_len=100, len_mode=1, zipf_s=1.0, seed=3)
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import make_queries as bench_queries
    terms, off = bench_queries(seg, 30_000, 6, 10, seed=1, zipf_s=1.0)
    tested = skipped = cand = resc = 0
    for q in range(6):
        t = terms[off[q]:off[q + 1]]
        got, st = oix.dense_model(t, 100, wmax=16384, w0=256, phases=1)
        assert got.tobytes() == oix.search_brute(t, 100).tobytes()
        tested += st["tested"]
        skipped += st["skipped"]
        cand += st["candidates"]
        resc += st["rescored"]
    assert tested > 0 and skipped > 0.3 * tested, (tested, skipped)
    assert resc < cand, (cand, resc)  # the flush drops candidates the threshold has overtaken


_EDGE = {}


def _edge(name):
    if name not in _EDGE:
        _EDGE[name] = {
            "lognormal": lambda: make_corpus(40000, 3000, seed=7, length="lognormal", mean_len=60),
            "long": lambda: make_long_corpus(30000, 1500, seed=1),  # every fieldnorm code, tf <= 127
            "long_wide_tf": lambda: make_long_corpus(30000, 1500, seed=2, wide_tf=True),
            "short": lambda: make_short_corpus(30000, 400, seed=3),  # lengths 1..3 against a mean of ~10^5
            "tie": lambda: make_tie_corpus(60000, 150, seed=4),  # tf 1 or 2, head terms in 70 % of the documents
        }[name]()
    return _EDGE[name]


@pytest.mark.parametrize("k1,b", PARAMS, ids=[f"k1={k1}-b={b}" for k1, b in PARAMS])
@pytest.mark.parametrize("name", ["lognormal", "long", "long_wide_tf", "short", "tie"])
def test_model_across_bm25_parameters(name, k1, b):
    """The bound argument (s0 rounded up with 1 + 2^-19, s1 rounded down, acc >= scale x score, the histogram's lower bound) over
    the legal k1 / b range: at b = 1 S1 is 0 for fieldnorm 0 and tiny for short documents under a large mean, at b = 0 all
    documents share one S1 and scores tie in masses, the long corpora reach every fieldnorm code"""
    c = _edge(name)
    seg = vb.Segment.build(k1, b, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    terms, off = make_queries(c, 6, 3 if name in ("short", "tie") else 4, seed=9)
    rows = [terms[off[q]:off[q + 1]] for q in range(len(off) - 1)]
    if name == "tie":
        h = np.sort(c["token_to_term"][:3]).astype(np.uint32)  # (the head tokens: masses of equal scores)
        rows += [h[:2], h]
    for q, t in enumerate(rows):
        for k in (10, 100):
            ref = oix.search_brute(t, k)
            for wmax, w0, ph in ((16384, 256, 1), (1024, 64, 2), (8192, 0, 0)):
                got, _ = oix.dense_model(t, k, wmax=wmax, w0=w0, phases=ph)
                assert got.tobytes() == ref.tobytes(), (q, k, wmax, w0, ph)
