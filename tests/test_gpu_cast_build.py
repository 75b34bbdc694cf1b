"""vbm25_device_segment_build_documents: DeviceSegment.from_documents(...).download() equals the host model's Segment.build of the same
vocabulary and mappings, byte for byte (arrays() and meta()), at every (k1, b) of the parameter range's corners; the grid stride of
the build kernels; the index of the result searches as the model's; the refusals.  -m gpu only."""
import numpy as np
import pytest

import cast_model as cm
import vectorchord_bm25_amd as vb

pytestmark = pytest.mark.gpu
INVALID = -1


def corpus():
    w = cm.words(50)
    docs = cm.corpus(w[:46], 300, seed=21)
    for d in docs:
        d.append((w[46], 1))                      # a lexeme in every document (but the three set below): a term of three 128-posting blocks
    docs[17].append((w[47], 4))                   # a lexeme in one document
    docs[40] = []                                 # a document without lexemes
    docs[41] = [(w[48], 2)]                       # a document whose only lexeme is unique to it
    docs[299] = [(w[49], 1), (w[49], 1)]
    return docs


@pytest.fixture(scope="module")
def cast():
    docs = corpus()
    pay = cm.payloads(len(docs))
    return vb.Documents.cast(docs, pay, seed=cm.SEED), cm.cast(docs, pay)


@pytest.mark.parametrize("k1", [1.2, 2.0])
@pytest.mark.parametrize("b", [0.0, 0.75, 1.0])
def test_segment_equals_the_host_build(cast, k1, b):
    h, model = cast
    dseg = vb.DeviceSegment.from_documents(h, k1, b)
    want = cm.build_segment(model, k1, b)
    assert (dseg.n_docs, dseg.n_terms) == (300, 50) and dseg.n_postings == len(model["g_tf"])
    cm.same_segment(dseg.download(), want, f"k1={k1} b={b}")
    a = want.arrays()
    assert int(a["term_df"].max()) == 297 and int(a["term_df"].min()) == 1  # (128 + 128 + 41 postings: three blocks)


def test_the_seventy_thousand_document_batch():
    docs, pay, model = cm.grid_stride_model(wide=False)
    dseg = vb.DeviceSegment.from_documents(vb.Documents.cast(docs, pay, seed=cm.SEED), 1.2, 0.75)
    cm.same_segment(dseg.download(), cm.build_segment(model, 1.2, 0.75), "70 000 documents")


def test_grid_stride_of_the_build_kernels():
    """more elements than the 2048 x 256 = 524 288 threads of one pass of build_key_kernel, build_flag_kernel and build_emit_kernel:
    their grid-stride loops take a second turn"""
    docs, pay, model = cm.grid_stride_model(wide=True)
    h = vb.Documents.cast(docs, pay, seed=cm.SEED)
    assert h.n_elements == len(model["g_tf"]) and h.n_elements > 2048 * 256
    dseg = vb.DeviceSegment.from_documents(h, 1.2, 0.75)
    cm.same_segment(dseg.download(), cm.build_segment(model, 1.2, 0.75), "70 000 documents of 8 lexemes")


def test_the_index_of_the_result_searches_as_the_models(cast):
    h, model = cast
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(h, 1.2, 0.75))
    ref = vb.GpuIndex(cm.build_segment(model, 1.2, 0.75))
    rng = np.random.default_rng(2)
    terms = np.concatenate([np.sort(rng.choice(50, 4, replace=False)) for _ in range(32)]).astype(np.uint32)
    off = (np.arange(33) * 4).astype(np.uint32)
    for k in (1, 10, 300):
        got, want = vb.search_batch(gix, terms, off, k), vb.search_batch(ref, terms, off, k)
        assert want[1].max() > 0
        cm.same_records(got, want, f"k={k}")


def test_refusals(cast):
    h, _ = cast
    docs = corpus()[:5]
    for bad, k1 in ((vb.Documents.cast(docs, None, seed=cm.SEED), 1.2), (vb.Documents.cast([], np.zeros((0, 3), np.uint16)), 1.2), (h, 1.0)):
        with pytest.raises(vb.Vbm25Error) as e:
            vb.DeviceSegment.from_documents(bad, k1, 0.75)
        assert e.value.code == INVALID
    with pytest.raises(vb.Vbm25Error, match="k1 must be in"):
        vb.DeviceSegment.from_documents(h, 1.0, 0.75)
    with pytest.raises(vb.Vbm25Error, match="without payloads"):
        vb.DeviceSegment.from_documents(vb.Documents.cast(docs, None, seed=cm.SEED), 1.2, 0.75)
    vb.DeviceSegment.from_documents(h, 1.2, 0.75)  # (and the handle still builds)
