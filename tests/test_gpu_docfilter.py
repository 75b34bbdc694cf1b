"""Filtered search with per-query document bitmaps (vbm25_filter_*, vbm25_search_batch_filtered, vbm25_batch_set_filter) on every route
the host can choose: the records of a filtered query are byte for byte the first k entries of the oracle's unfiltered full ranking with
the rejected documents removed.  The adversarial filter rejects exactly the documents of a query's unfiltered top-(4k): a kernel that
started from theta0 (term_kth_ub, a bound over all documents) or let a rejected document raise its threshold returns short or wrong
lists under it.  -m gpu only."""
import ctypes

import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from parity import assert_bit_exact

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER


def _built(n_docs, vocab, seed, length="lognormal", mean_len=60, zipf=None):
    c = make_corpus(n_docs, vocab, seed=seed, length=length, mean_len=mean_len, zipf=zipf)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    return c, seg


def _synth(n_docs, vocab, seed, zipf_s=0.0):
    return vb.Segment.synth(n_docs, vocab, mean_len=100, len_mode=1, zipf_s=zipf_s, seed=seed)


def _bench_queries(seg, vocab, nq, nterms, seed, zipf_s=0.0):
    from bench import make_queries as mq
    return mq(seg, vocab, nq, nterms, seed=seed, zipf_s=zipf_s)


def _oracle(seg):
    return orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())


def _full(oix, terms, off):
    """per query the oracle's complete unfiltered ranking (asserted complete: fewer than 65535 matches)"""
    out = []
    for q in range(len(off) - 1):
        f = oix.search_brute(terms[off[q]:off[q + 1]], 65535)
        assert len(f) < 65535, "the reference ranking would be cut"
        out.append(f)
    return out


def _want(full, keep, k):
    """the filtered answer: full ranking, rejected documents removed, cut to k"""
    return full[:k] if keep is None else full[keep[full["doc_id"]]][:k]


def _check(hits, nh, fulls, keeps, sel, k, what):
    for q in range(len(fulls)):
        s = int(sel[q])
        want = fulls[q][:k] if s == NONE else _want(fulls[q], keeps[s], k)
        assert nh[q] == len(want), f"{what} q{q}: {nh[q]} hits, want {len(want)}"
        assert_bit_exact(want, hits[q, :nh[q]], what=f"{what} q{q}")


def _adversarial(n_docs, fulls, k):
    """per query: every document but those of its unfiltered top-(4k)"""
    keep = np.ones((len(fulls), n_docs), dtype=bool)
    for q, f in enumerate(fulls):
        keep[q, f["doc_id"][:4 * k]] = False
    return keep


def _run_batch(gix, terms, off, k, doc_filter, sel, route):
    nq = len(off) - 1
    b = vb.Batch(gix, nq, max(1, len(terms)), k)
    b.set_queries(terms, off)
    assert b.debug_route() == route, f"route {b.debug_route()} instead of {route}"
    b.set_filter(doc_filter, sel)
    b.run()
    hits, nh = b.fetch()
    return b, hits, nh


_CACHE = {}


def _corpus(name):
    """(index, n_docs, terms, off, full rankings) of the corpora below, made once per session"""
    if name in _CACHE:
        return _CACHE[name]
    if name == "A":  # 200 k documents, 4-term queries
        c, seg = _built(200_000, 3000, seed=2)
        terms, off = make_queries(c, 48, 4, seed=9)
    elif name == "A12":  # 9-16 terms: scan_range_kernel's 16-row instantiation (< 65535 documents: the reference is complete)
        c, seg = _built(60_000, 3000, seed=2)
        terms, off = make_queries(c, 32, 12, seed=13)
    elif name == "A20":  # more than 16 terms: scan_many_kernel
        c, seg = _built(60_000, 3000, seed=4)
        terms, off = make_queries(c, 16, 20, seed=14)
    elif name == "C3":  # C3's shape at reduced size: scan_win_kernel
        seg = _synth(700_000, 33_000, seed=7)
        terms, off = _bench_queries(seg, 33_000, 256, 5, seed=3)
    elif name == "Z":  # Zipf head terms: scan_dense_kernel
        seg = _synth(60_000, 20_000, seed=3, zipf_s=1.0)
        terms, off = _bench_queries(seg, 20_000, 48, 3, seed=5, zipf_s=1.0)
    else:
        raise KeyError(name)
    oix = _oracle(seg)
    r = (seg, seg.n_docs, terms, off, _full(oix, terms, off))
    _CACHE[name] = r
    return r


# (case, corpus, k, route, tuning, index tuning)
ROUTES = [
    ("plan_range", "A", 10, 0, dict(fused=0, arith=0, win=0), {}),
    ("plan_range_k100", "A", 100, 0, dict(fused=0, arith=0, win=0), {}),
    ("fused", "A", 10, 1, {}, {}),
    ("arith_k1", "A", 1, 2, dict(fused=0, win=0), {}),
    ("arith_k256", "A", 256, 2, dict(fused=0, win=0), {}),
    ("arith_no_maxscore", "A", 10, 2, dict(fused=0, win=0, ne=0), {}),
    ("terms_9_16", "A12", 10, 2, dict(fused=0, win=0, dense_x1000=10 ** 9), {}),
    ("terms_over_16", "A20", 10, 0, {}, {}),
    ("many_k300", "A", 300, 0, {}, {}),
    ("many_k1000", "A", 1000, 0, {}, {}),
    ("bigk_k2000", "A20", 2000, 4, {}, {}),
    ("win", "C3", 10, 3, dict(fused=0), {}),
    ("win_k100", "C3", 100, 3, dict(fused=0), {}),
    ("win_nofuse", "C3", 10, 3, dict(fused=0, win_fuse=0), {}),
    ("win_giveup", "A", 10, 3, dict(win_force=1, fused=0), {}),
    ("win_id16_decode", "C3", 10, 3, dict(fused=0), dict(id16_plane=0, rel16_plane=0)),
    ("dense", "Z", 10, 0, {}, {}),
    ("dense_k100", "Z", 100, 0, {}, {}),
]


@pytest.mark.parametrize("case,corpus,k,route,tune,index_tune", ROUTES, ids=[r[0] for r in ROUTES])
def test_adversarial_filter_on_every_route(tuning, case, corpus, k, route, tune, index_tune):
    seg, n_docs, terms, off, fulls = _corpus(corpus)
    nq = len(off) - 1
    if route == 1:  # (the one-launch route: a handful of queries)
        nq = 4
        off = off[:nq + 1]
        terms = terms[:off[-1]]
        fulls = fulls[:nq]
    if route == 4:
        nq = 3
        off = off[:nq + 1]
        terms = terms[:off[-1]]
        fulls = fulls[:nq]
    if index_tune:
        tuning(**index_tune)
    gix = vb.GpuIndex(seg)
    vb.reset_tuning()
    tuning(**tune)
    keep = _adversarial(n_docs, fulls, k)
    f = vb.DocFilter(gix, keep)
    sel = np.arange(nq, dtype=np.uint32)
    b, hits, nh = _run_batch(gix, terms, off, k, f, sel, route)
    _check(hits, nh, fulls, keep, sel, k, case)
    # the filter did bite: every query with more than 4k matches lost its unfiltered top-k
    for q in range(nq):
        if len(fulls[q]) > 4 * k:
            assert not np.isin(hits[q, :nh[q]]["doc_id"], fulls[q]["doc_id"][:4 * k]).any()
    if corpus == "Z":
        assert b.debug_routes()[4] > 0, "no item went to scan_dense_kernel"
    if case == "win_giveup":
        assert b.debug_counts()[1] > 0, "this shape is expected to give items up"
    # the same batch again (no stale threshold), and through vbm25_search_batch_filtered
    b.run()
    h2, n2 = b.fetch()
    assert h2.tobytes() == hits.tobytes() and np.array_equal(n2, nh)
    h3, n3 = vb.search_batch_masked(gix, terms, off, k, f, sel)
    _check(h3, n3, fulls, keep, sel, k, case + " (search_batch_masked)")


@pytest.mark.parametrize("corpus,tune", [("A", dict(fused=0, win=0)), ("C3", dict(fused=0))], ids=["range", "win"])
def test_filter_densities(tuning, corpus, tune):
    """keep-all: byte-identical to search_batch; keep-none: no hits; 1/2, 1/10, 1/300 and 1/100 000 of the documents (the last
    one far beyond what the over-fetch loop reaches in one round)."""
    seg, n_docs, terms, off, fulls = _corpus(corpus)
    gix = vb.GpuIndex(seg)
    tuning(**tune)
    nq, k = len(off) - 1, 10
    ids = np.arange(n_docs)
    keeps = np.stack([np.ones(n_docs, bool), np.zeros(n_docs, bool)] + [ids % m == 1 for m in (2, 10, 300, 100_000)])
    f = vb.DocFilter(gix, keeps)
    plain, n_plain = vb.search_batch(gix, terms, off, k)
    for i in range(len(keeps)):
        sel = np.full(nq, i, dtype=np.uint32)
        hits, nh = vb.search_batch_masked(gix, terms, off, k, f, sel)
        if i == 0:
            assert hits.tobytes() == plain.tobytes() and np.array_equal(nh, n_plain)
        elif i == 1:
            assert not nh.any()
        _check(hits, nh, fulls, keeps, sel, k, f"bitmap {i}")


def test_mixed_selectors_leave_unfiltered_queries_unchanged(tuning):
    """One batch of several bitmaps and NO_FILTER: the unfiltered queries' records are byte-identical to an unfiltered run (theta0
    stays on for them), the others follow their own bitmaps."""
    seg, n_docs, terms, off, fulls = _corpus("C3")
    gix = vb.GpuIndex(seg)
    tuning(fused=0)
    nq, k = len(off) - 1, 10
    ids = np.arange(n_docs)
    keeps = np.stack([ids % 2 == 0, ids % 10 == 3, _adversarial(n_docs, fulls[:1], k)[0]])
    f = vb.DocFilter(gix, keeps)
    sel = np.array([[0, 1, NONE, 2][q % 4] for q in range(nq)], dtype=np.uint32)
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_queries(terms, off)
    assert b.debug_route() == 3
    b.run()
    plain, n_plain = b.fetch()
    b.set_filter(f, sel)
    b.run()
    hits, nh = b.fetch()
    _check(hits, nh, fulls, keeps, sel, k, "mixed")
    for q in np.flatnonzero(sel == NONE):
        assert nh[q] == n_plain[q] and hits[q, :nh[q]].tobytes() == plain[q, :nh[q]].tobytes(), f"unfiltered q{q} changed"
    b.set_filter(None)  # ... and without the filter again
    b.run()
    h2, n2 = b.fetch()
    assert h2.tobytes() == plain.tobytes() and np.array_equal(n2, n_plain)


def test_resident_batch_follows_updated_bits(tuning):
    """A resident batch run, its bitmap replaced through update() and then through device_words (bits built by torch on the GPU),
    run again: the records follow the new bits each time (nothing of the previous run's threshold survives)."""
    import torch

    seg, n_docs, terms, off, fulls = _corpus("A")
    gix = vb.GpuIndex(seg)
    tuning(fused=0, win=0)
    nq, k = len(off) - 1, 10
    ids = np.arange(n_docs)
    keep0 = ids % 2 == 0
    f = vb.DocFilter(gix, keep0)
    sel = np.zeros(nq, dtype=np.uint32)
    b = vb.Batch(gix, nq, len(terms), k)
    b.set_queries(terms, off)
    b.set_filter(f, sel)
    b.run()
    hits, nh = b.fetch()
    _check(hits, nh, fulls, keep0[None], sel, k, "before")
    keep1 = ids % 2 == 1  # (disjoint from the first: a threshold kept from the first run would lose hits)
    f.update(0, keep1)
    b.run()
    hits, nh = b.fetch()
    _check(hits, nh, fulls, keep1[None], sel, k, "after update")
    # device_words: the bits of "d % 7 == 5" packed by torch on the GPU, copied into the filter's bitmap
    keep2 = ids % 7 == 5
    n_words = (n_docs + 63) // 64
    bits = torch.zeros(64 * n_words, dtype=torch.bool, device="cuda")
    d = torch.arange(n_docs, device="cuda")
    bits[:n_docs] = d % 7 == 5
    words = (bits.view(n_words, 64).to(torch.int64) << torch.arange(64, device="cuda")).sum(dim=1)
    assert np.array_equal(words.cpu().numpy().view(np.uint64), vb.DocFilter.pack(keep2, n_docs)[0])
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so.7")  # (the one HIP runtime of the process: torch's and the library's)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(f.device_words(0), words.data_ptr(), 8 * n_words, 3) == 0  # hipMemcpyDeviceToDevice
    b.run()
    hits, nh = b.fetch()
    _check(hits, nh, fulls, keep2[None], sel, k, "after device_words")


def test_c3_shape_with_a_filter_on_the_window_route():
    """Segment.synth at C3's shape, reduced (1024 queries x 5 terms), a filter keeping a tenth of the documents, the batched route 3."""
    seg = _synth(1_000_000, 33_000, seed=7)
    terms, off = _bench_queries(seg, 33_000, 1024, 5, seed=3)
    gix = vb.GpuIndex(seg)
    keep = np.arange(seg.n_docs) % 10 == 7
    f = vb.DocFilter(gix, keep)
    nq, k = 1024, 10
    sel = np.zeros(nq, dtype=np.uint32)
    b, hits, nh = _run_batch(gix, terms, off, k, f, sel, 3)
    oix = _oracle(seg)
    fulls = [oix.search_brute(terms[off[q]:off[q + 1]], 65535) for q in range(0, nq, 8)]
    _check(hits[::8], nh[::8], fulls, keep[None], sel[::8], k, "C3 1/10")


def test_argument_errors():
    seg, n_docs, terms, off, _ = _corpus("A")
    gix = vb.GpuIndex(seg)
    other = vb.GpuIndex(seg)
    f = vb.DocFilter(gix, np.ones((2, n_docs), bool))
    nq = len(off) - 1
    with pytest.raises(vb.Vbm25Error) as e:  # a filter of another index
        vb.search_batch_masked(other, terms, off, 10, f, np.zeros(nq, np.uint32))
    assert e.value.code == -1
    with pytest.raises(vb.Vbm25Error) as e:  # selector out of range
        vb.search_batch_masked(gix, terms, off, 10, f, np.full(nq, 2, np.uint32))
    assert e.value.code == -1
    b = vb.Batch(other, nq, len(terms), 10)
    with pytest.raises(vb.Vbm25Error):
        b.set_filter(f, np.zeros(nq, np.uint32))
    L = vb.lib()
    with pytest.raises(vb.Vbm25Error):  # NULL words
        vb.api.check(L.vbm25_filter_update(f.h, 0, None))
    with pytest.raises(vb.Vbm25Error):  # bitmap index out of range
        f.update(2, np.ones(n_docs, bool))
    with pytest.raises(vb.Vbm25Error):  # NULL q_filter
        vb.api.check(L.vbm25_search_batch_filtered(gix.h, f.h, None, vb.api._p(terms), off.ctypes.data_as(ctypes.c_void_p), nq, 10,
                                                   None, None))
    if n_docs % 64:  # a bit at or beyond n_docs
        words = vb.DocFilter.pack(np.ones(n_docs, bool), n_docs)
        words[0, -1] |= np.uint64(1) << np.uint64(63)
        with pytest.raises(vb.Vbm25Error):
            vb.api.check(L.vbm25_filter_update(f.h, 0, vb.api._p(words)))
    # after the errors the index still serves unfiltered searches
    h, n = vb.search_batch(gix, terms, off, 10)
    h2, n2 = vb.search_batch_masked(gix, terms, off, 10, f, np.full(nq, NONE, np.uint32))
    assert h.tobytes() == h2.tobytes() and np.array_equal(n, n2)
