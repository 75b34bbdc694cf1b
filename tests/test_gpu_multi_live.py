"""A live table behind vbm25_multi_* (vbm25_multi_batch_set_growing / _set_filter) on the one GPU of the test box: 2 to 4 replicas on
device 0, every replica with its OWN growing segment and filter built on vbm25_multi_index(m, i); the selectors are cut by the shard
bounds of the queries.  Records equal the single handle's vbm25_search_batch_growing_filtered byte for byte.  -m gpu only."""
import ctypes as C

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from growing_data import make_growing
from lifecycle_data import built
from test_gpu_growing_append import docs

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
INVALID, UNSUPPORTED = -1, -4
GUARD = 0xA5A5A5A5

_C = {}


def _base():
    if "A" not in _C:
        c = make_corpus(120_000, 3000, seed=11, length="lognormal", mean_len=60)
        seg = built(c)
        _C["A"] = (c, seg, vb.GpuIndex(seg))
    return _C["A"]


def _replicas(seg, n_rep, G, keeps, gkeeps):
    multi = vb.MultiIndex(seg, [0] * n_rep)
    gss = [vb.GrowingSegment(multi.index(i), **G) for i in range(n_rep)]
    fs = [vb.DocFilter(multi.index(i), keeps) for i in range(n_rep)]
    for f, gs in zip(fs, gss):
        f.set_growing(gs, gkeeps)
    return multi, gss, fs


def fetch_guarded(mb, nq, k):
    hits = np.zeros((nq + 1, k), dtype=vb.HIT_DTYPE)
    hits.view(np.uint8)[:] = 0xA5
    cnt = np.full(nq + 4, GUARD, dtype=np.uint32)
    vb.api.check(vb.lib().vbm25_multi_batch_fetch(mb.h, hits.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
    assert np.all(cnt[nq:] == GUARD), "vbm25_multi_batch_fetch wrote past n_hits[nq]"
    assert np.all(hits[nq:].view(np.uint8) == 0xA5), "vbm25_multi_batch_fetch wrote past hits[nq]"
    return hits[:nq], cnt[:nq]


def same(want, got, what):
    (wh, wn), (gh, gn) = want, got
    assert np.array_equal(wn, gn), f"{what}: counts differ"
    for q in range(len(wn)):
        assert wh[q, :wn[q]].tobytes() == gh[q, :gn[q]].tobytes(), f"{what} q{q}: records differ"


@pytest.mark.parametrize("n_rep,nq,k", [(2, 64, 10), (3, 101, 10), (2, 7, 10), (4, 3, 5), (3, 2, 10), (2, 41, 300), (2, 6, 2000)])
def test_replicas_with_their_own_segments_and_filters(n_rep, nq, k):
    """odd shard sizes, fewer queries than replicas (empty shards), the one-launch route inside a shard, k > 1024"""
    c, seg, single = _base()
    terms, off = make_queries(c, nq, 4, seed=5 + nq)
    n_grow = 8192 + 500
    G, _ = make_growing(seg.arrays()["term_key"], n_grow, seed=nq, pool=terms[terms < seg.n_terms], pool_p=0.4)
    rng = np.random.default_rng(k)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, np.arange(seg.n_docs) % 10 == 3])
    gkeeps = np.stack([rng.random(n_grow) < 0.5, np.arange(n_grow) % 7 == 2])
    gs1 = vb.GrowingSegment(single, **G)
    f1 = vb.DocFilter(single, keeps)
    f1.set_growing(gs1, gkeeps)
    sel = np.array([[0, NONE, 1][q % 3] for q in range(nq)], np.uint32)
    multi, gss, fs = _replicas(seg, n_rep, G, keeps, gkeeps)
    mb = vb.MultiBatch(multi, nq + 3, len(terms) + 8, k)
    # only the segments
    mb.set_growing(gss)
    mb.set_queries(terms, off)
    mb.run()
    want_g = vb.search_batch_growing(single, gs1, terms, off, k)
    same(want_g, fetch_guarded(mb, nq, k), "segments only")
    assert int((want_g[0]["doc_id"] > 0xFFFFFFFF - n_grow).sum()) > 0
    # segments and filters; run twice
    mb.set_filter(fs, sel)
    mb.set_queries(terms, off)
    want = vb.search_batch_growing_masked(single, gs1, terms, off, k, f1, sel)
    for i in range(2):
        mb.run()
        same(want, fetch_guarded(mb, nq, k), f"segments and filters, run {i}")
    # a shorter query set: the selectors are cut by ITS shard bounds
    nq2 = max(1, nq // 2)
    terms2, off2 = terms[:off[nq2]], off[:nq2 + 1]
    mb.set_queries(terms2, off2)
    mb.run()
    same(vb.search_batch_growing_masked(single, gs1, terms2, off2, k, f1, sel[:nq2]), fetch_guarded(mb, nq2, k), "a shorter query set")
    # only the filters
    mb.set_growing(None)
    mb.set_queries(terms, off)
    mb.run()
    same(vb.search_batch_masked(single, terms, off, k, f1, sel), fetch_guarded(mb, nq, k), "filters only")
    # nothing
    mb.set_filter(None)
    mb.run()
    same(vb.search_batch(single, terms, off, k), fetch_guarded(mb, nq, k), "detached")


def test_wrong_replica_and_pairing_errors():
    c, seg, single = _base()
    nq, k = 33, 10
    terms, off = make_queries(c, nq, 4, seed=2)
    n_grow = 3000
    G, _ = make_growing(seg.arrays()["term_key"], n_grow + 40, seed=1, pool=terms[terms < seg.n_terms], pool_p=0.4)
    GA = docs(G, 0, n_grow)
    rng = np.random.default_rng(1)
    keeps = np.stack([rng.random(seg.n_docs) < 0.5, rng.random(seg.n_docs) < 0.2])
    gkeeps = np.stack([rng.random(n_grow + 40) < 0.5, rng.random(n_grow + 40) < 0.2])
    sel = np.array([[0, 1, NONE][q % 3] for q in range(nq)], np.uint32)
    multi, gss, fs = _replicas(seg, 3, GA, keeps, gkeeps[:, :n_grow])
    gs1 = vb.GrowingSegment(single, **GA)
    f1 = vb.DocFilter(single, keeps)
    f1.set_growing(gs1, gkeeps[:, :n_grow])
    want = vb.search_batch_growing_masked(single, gs1, terms, off, k, f1, sel)
    mb = vb.MultiBatch(multi, nq, len(terms), k)
    mb.set_growing(gss)
    mb.set_filter(fs, sel)
    mb.set_queries(terms, off)
    mb.run()
    same(want, fetch_guarded(mb, nq, k), "before")

    def refused(code, fn, *args):
        with pytest.raises(vb.Vbm25Error) as e:
            fn(*args)
        assert e.value.code == code, str(e.value)
        mb.run()  # nothing changed on any replica
        same(want, fetch_guarded(mb, nq, k), "after a refused setter")

    # handles of the wrong replica (replicas 1 and 2 swapped), of the single index, a selector no filter has
    refused(INVALID, mb.set_growing, [gss[0], gss[2], gss[1]])
    refused(INVALID, mb.set_filter, [fs[0], fs[2], fs[1]], sel)
    refused(INVALID, mb.set_growing, [gss[0], gss[1], gs1])
    refused(INVALID, mb.set_filter, [fs[0], fs[1], f1], sel)
    refused(INVALID, mb.set_filter, fs, np.full(nq, 2, np.uint32))
    # pairing: a filter without growing bitmaps on one replica; bitmaps of another upload
    plain = vb.DocFilter(multi.index(2), keeps)
    refused(UNSUPPORTED, mb.set_filter, [fs[0], fs[1], plain], sel)
    gs_again = vb.GrowingSegment(multi.index(1), **GA)
    refused(INVALID, mb.set_growing, [gss[0], gs_again, gss[2]])
    # an append on one replica without an extend: set_queries and run refuse; after the extend (on every replica) they serve the new state
    delta = docs(G, n_grow, n_grow + 40)
    gss[1].append(**delta)
    with pytest.raises(vb.Vbm25Error) as e:
        mb.run()
    assert e.value.code == INVALID
    with pytest.raises(vb.Vbm25Error) as e:
        mb.set_queries(terms, off)
    assert e.value.code == INVALID
    for i in (0, 2):
        gss[i].append(**delta)
    gs1.append(**delta)
    for f, gs in zip(fs + [f1], gss + [gs1]):
        f.extend_growing(gs, gkeeps[:, n_grow:])
    mb.set_queries(terms, off)
    mb.run()
    same(vb.search_batch_growing_masked(single, gs1, terms, off, k, f1, sel), fetch_guarded(mb, nq, k), "after append and extend")
