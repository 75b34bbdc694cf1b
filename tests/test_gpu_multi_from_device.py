"""vbm25_multi_create_from_device: the replicas of a compacted device segment, all on device 0 (as tests/test_gpu_multi.py).  Their
records are byte-identical to a GpuIndex of the same device segment, with and without per-replica remapped filters; the segment is
left as it was.  -m gpu only."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus
from growing_data import make_growing

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER

_C = {}


def compacted():
    """a 20 000-document index, 5 % deleted, 2000 growing documents (a tenth deleted), compacted; a filter of the old index"""
    if "A" not in _C:
        c = make_corpus(20_000, 600, seed=1, length="lognormal", mean_len=40)
        seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
        gix = vb.GpuIndex(seg)
        G, _ = make_growing(seg.arrays()["term_key"], 2000, seed=5, deleted=0.1)
        rng = np.random.default_rng(3)
        deleted = rng.random(seg.n_docs) < 0.05
        bits = rng.random((3, seg.n_docs + 2000)) < 0.5
        f = vb.DocFilter(gix, bits[:, :seg.n_docs])
        gs = vb.GrowingSegment.from_dict(gix, G)
        f.set_growing(gs, bits[:, seg.n_docs:])
        ds = vb.DeviceSegment.maintain(gix, deleted, G)
        _C["A"] = (gix, gs, f, deleted, G, ds)
    return _C["A"]


def queries(n_terms, nq, nt, seed):
    rng = np.random.default_rng(seed)
    terms = np.sort(np.stack([rng.choice(n_terms, nt, replace=False) for _ in range(nq)]), axis=1).reshape(-1).astype(np.uint32)
    return terms, (np.arange(nq + 1) * nt).astype(np.uint32)


def assert_same_segment(a, b):
    assert a.meta() == b.meta()
    x, y = a.arrays(), b.arrays()
    for name in y:
        assert np.array_equal(x[name].reshape(-1), y[name].reshape(-1)), name


@pytest.mark.parametrize("n_rep,nq", [(2, 33), (3, 101), (3, 7)])
def test_replicas_of_a_compacted_segment_match_the_single_handle(n_rep, nq):
    gix, gs, f, deleted, G, ds = compacted()
    before = ds.download()
    single = vb.GpuIndex(ds)
    multi = vb.MultiIndex.from_device(ds, [0] * n_rep)
    assert multi.n_devices == n_rep
    terms, off = queries(ds.n_terms, nq, 3, seed=nq)
    for k in (10, 300):
        h1, n1 = vb.search_batch(single, terms, off, k)
        h2, n2 = multi.search_batch(terms, off, k)
        assert int(n1.sum()) > 0 and np.array_equal(n1, n2) and h1.tobytes() == h2.tobytes(), k
    # per-replica remapped filters on the resident batch against the single handle's filtered search
    k = 10
    filters = [f.remap(multi.index(i), deleted, G["g_deleted"]) for i in range(n_rep)]
    sf = f.remap(single, deleted, G["g_deleted"])
    for i in range(n_rep):
        assert all(filters[i].read(j).tobytes() == sf.read(j).tobytes() for j in range(3))
    sel = (np.arange(nq) % 4).astype(np.uint32)
    sel[sel == 3] = NONE
    mb = vb.MultiBatch(multi, nq, len(terms), k)
    mb.set_filter(filters, sel)
    mb.set_queries(terms, off)
    mb.run()
    h3, n3 = mb.fetch()
    h4, n4 = vb.search_batch_masked(single, terms, off, k, sf, sel)
    assert np.array_equal(n3, n4) and h3.tobytes() == h4.tobytes()
    hu, nu = vb.search_batch(single, terms, off, k)
    assert h4.tobytes() != hu.tobytes()  # (the filters do reject something)
    mb.set_filter(None)
    del mb, multi, filters
    # the segment is left as it was: still downloadable, the same bytes
    assert_same_segment(ds.download(), before)


def test_the_first_device_must_be_the_segments():
    gix, gs, f, deleted, G, ds = compacted()
    for devices in ([99], [99, 0], [1_000_000, 0, 0]):  # (out of range: no second GPU is needed)
        with pytest.raises(vb.Vbm25Error) as e:
            vb.MultiIndex.from_device(ds, devices)
        assert e.value.code == -1 and "devices[0]" in str(e.value)
    with pytest.raises(vb.Vbm25Error) as e:  # a later device out of range: refused as vbm25_multi_create refuses it
        vb.MultiIndex.from_device(ds, [0, 99])
    assert e.value.code == -1
    with pytest.raises(vb.Vbm25Error) as e:
        vb.MultiIndex.from_device(ds, [])
    assert e.value.code == -1
    # the segment still makes an index
    assert vb.GpuIndex(ds).n_docs == ds.n_docs
