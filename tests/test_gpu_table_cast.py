"""One short life of a table driven from lexemes only -- from_documents, index, Resolver queries, append_documents, search, maintain
with the downloaded CSR, search -- against the same life driven through the host model's arrays.  -m gpu only."""
import numpy as np
import pytest

import cast_model as cm
import vectorchord_bm25_amd as vb

pytestmark = pytest.mark.gpu


def test_a_table_from_lexemes():
    lexemes, later = cm.words(80), cm.words(30, tag=b"later")
    docs0, docs1 = cm.corpus(lexemes, 2000, seed=31, mean=9), cm.corpus(lexemes + later, 700, seed=32, mean=9)
    pay0, pay1 = cm.payloads(2000, seed=31), cm.payloads(700, seed=32)
    m0, m1 = cm.cast(docs0, pay0), cm.cast(docs1, pay1)
    # 1, 2: the index
    h0 = vb.Documents.cast(docs0, pay0, seed=cm.SEED)
    dseg = vb.DeviceSegment.from_documents(h0, 1.2, 0.75)
    mseg = cm.build_segment(m0, 1.2, 0.75)
    cm.same_segment(dseg.download(), mseg, "the built segment")
    gix, mix = vb.GpuIndex(dseg), vb.GpuIndex(mseg)
    # 3: queries from lexemes
    rng = np.random.default_rng(33)
    pool = lexemes + later[:6] + [b"nowhere"]
    queries = [[pool[j] for j in rng.integers(0, len(pool), int(rng.integers(1, 6)))] for _ in range(40)]
    r = vb.Resolver(gix, 1, len(queries), 256, 1 << 14, seed=cm.SEED)
    r.submit(queries)
    terms, off = r.collect()
    want_terms = [np.unique(i[i != 0xFFFFFFFF]) for i in (mix.lookup_terms([cm._intern(t, cm.SEED) for t in q]) for q in queries)]
    assert np.array_equal(terms, np.concatenate(want_terms)) and np.array_equal(np.diff(off), [len(t) for t in want_terms])
    for k in (1, 10):
        cm.same_records(vb.search_batch(gix, terms, off, k), vb.search_batch(mix, terms, off, k), f"sealed k={k}")
    # 4, 5: the insert
    empty = cm.cast([], np.zeros((0, 3), np.uint16))
    gs = vb.GrowingSegment.from_dict(gix, empty)
    h1 = vb.Documents.cast(docs1, pay1, seed=cm.SEED)
    gs.append_documents(h1)
    mgs = vb.GrowingSegment.from_dict(mix, m1)
    assert gs.n_docs == 700
    for k in (1, 10, 1500):
        cm.same_records(vb.search_batch_growing(gix, gs, terms, off, k), vb.search_batch_growing(mix, mgs, terms, off, k), f"growing k={k}")
    # 6, 7: the compaction, with the CSR the handle gives back
    gone = rng.random(2000) < 0.2
    csr = h1.download()
    cm.assert_same(csr, m1, "the downloaded CSR")
    new, relabel = vb.DeviceSegment.maintain(gix, gone, csr, return_relabel=True)
    mnew, mrelabel = vb.DeviceSegment.maintain(mix, gone, m1, return_relabel=True)
    assert np.array_equal(relabel, mrelabel)
    cm.same_segment(new.download(), mnew.download(), "the compacted segment")
    gix2, mix2 = vb.GpuIndex(new), vb.GpuIndex(mnew)
    r2 = vb.Resolver(gix2, 1, len(queries), 256, 1 << 14, seed=cm.SEED)
    r2.submit(queries)
    terms2, off2 = r2.collect()
    assert len(terms2) >= len(terms)  # (the later lexemes are in the vocabulary now)
    for k in (1, 10):
        cm.same_records(vb.search_batch(gix2, terms2, off2, k), vb.search_batch(mix2, terms2, off2, k), f"compacted k={k}")
