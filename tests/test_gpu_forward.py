"""The forward index of an index's own documents on the GPU (csrc/forward.hip): GpuIndex.bind array for array against Documents.bind
of the documents the index was made from and against a numpy transpose of the mappings a host-built index was made from -- every class
of the per-document sort and its edges, every codec shape, an index read from pages, an index after a compaction --, its scores bit
for bit against vb.evaluate, the scorer and the reranker ring byte for byte against the documents-bound handle, ctids from the index's
own payload plane, the refusals with code and message, buffers and threads.  -m gpu only."""
import ctypes as C
import threading

import numpy as np
import pytest

import cast_model as cm
import test_gpu_evaluate_documents as ev
import vectorchord_bm25_amd as vb
from codec_data import (TAIL_DOCS, WIDTH_DOCS, assert_tail_blocks, assert_width_blocks, build_args, list_keys, tail_lists, wide_tf_lists,
                        wide_tf_tail, width_lists)
from maintain_model import maintain
from test_gpu_rerank import lists_csr
from test_gpu_reranker import CAPS, ctid_lists, ctid_world, same, through

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
WAVE_MAX, GROUP_MAX = 64, 2048


# ---- helpers


def fieldnorms(dt):
    """(the handle's fieldnorm codes, whether vbm25_index_bind made it): vbm25_debug_doc_terms_fieldnorm, not in the header"""
    f = vb.lib().vbm25_debug_doc_terms_fieldnorm
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 3
    out, flag = np.zeros(max(dt.n_docs, 1), np.uint8), C.c_uint32()
    assert f(dt.h, out.ctypes.data, C.byref(flag)) == 0
    return out[:dt.n_docs], bool(flag.value)


def bind_stats():
    """(kernel ms, documents of the wave class, of the workgroup class, of the segmented sort) of this thread's last GpuIndex.bind:
    vbm25_debug_forward, not in the header"""
    f = vb.lib().vbm25_debug_forward
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 4
    ms, n = C.c_double(), [C.c_uint64() for _ in range(3)]
    assert f(C.byref(ms), *[C.byref(x) for x in n]) == 0
    return ms.value, tuple(x.value for x in n)


def class_counts(lengths, wave_max=WAVE_MAX, group_max=GROUP_MAX):
    lengths = np.asarray(lengths)
    wave = int((lengths <= wave_max).sum())
    group = int((lengths <= group_max).sum()) - wave
    return wave, group, len(lengths) - wave - group


def transpose(n_docs, term_start, post_doc, post_tf):
    """mappings in term order -> (start, term, tf) in document order: a stable sort by (doc, term)"""
    term_start = np.asarray(term_start).astype(np.int64)
    post_doc = np.asarray(post_doc).astype(np.int64)
    term = np.repeat(np.arange(len(term_start) - 1, dtype=np.int64), np.diff(term_start))
    order = np.lexsort((term, post_doc))
    start = np.concatenate([[0], np.cumsum(np.bincount(post_doc, minlength=n_docs))]).astype(np.uint64)
    return start, term[order].astype(np.uint32), np.asarray(post_tf)[order].astype(np.uint32)


def transpose_lists(n_docs, lists):
    term_start = np.cumsum([0] + [len(d) for d, _ in lists])
    return transpose(n_docs, term_start, np.concatenate([np.asarray(d) for d, _ in lists]), np.concatenate([np.asarray(t) for _, t in lists]))


def assert_arrays(got, want, what):
    for g, w, name in zip(got, want, ("start", "term", "tf")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs"


def assert_forward(dt, want, doc_fieldnorm, what):
    """the handle's four arrays against the model's three and the segment's fieldnorm codes (0 for a document without a posting)"""
    got = dt.download()
    assert_arrays(got, want, what)
    n = np.diff(want[0].astype(np.int64))
    fn, from_index = fieldnorms(dt)
    assert from_index
    assert np.array_equal(fn, np.where(n > 0, np.asarray(doc_fieldnorm), 0)), f"{what}: fieldnorm codes differ"
    assert (dt.n_docs, dt.n_known) == (len(n), len(want[1]))
    assert dt.device_bytes() >= 8 * dt.n_known + 9 * dt.n_docs


class DocWorld:
    """documents, cast; the index ambuild makes of them on the device, so its resolver knows every key; both bound handles"""

    def __init__(self, docs, pay=None, k1=1.2, b=0.75):
        self.docs = docs
        pay = cm.payloads(len(docs)) if pay is None else pay  # (an index needs them)
        self.h = vb.Documents.cast(docs, pay, seed=cm.SEED)
        self.dseg = vb.DeviceSegment.from_documents(self.h, k1, b)
        self.gix = vb.GpuIndex(self.dseg)
        self.resolver = vb.Resolver(self.gix, 1, 64, 4096, 1 << 18, seed=cm.SEED)
        self.from_docs = self.h.bind(self.resolver)
        self.from_index = self.gix.bind()

    def resolve(self, queries):
        self.resolver.submit(queries)
        return self.resolver.collect()


@pytest.fixture(scope="module")
def big():
    """the documents of tests/test_gpu_evaluate_documents.py: about 300 of 0 .. 5000 elements"""
    return DocWorld(ev.scored_docs(), cm.payloads(len(ev.scored_docs())))


# ---- 1. against the documents route


def test_the_bind_equals_the_documents_route(big):
    w = big
    got, want = w.from_index.download(), w.from_docs.download()
    assert_arrays(got, want, "index against documents")
    n = np.diff(want[0].astype(np.int64))
    assert [n[ev.EDGE[f"{k} elements"]] for k in (63, 64, 65, 2048, 5000)] == [63, 64, 65, 2048, 5000] and n[ev.EDGE["no elements"]] == 0
    assert n[ev.EDGE["1 element"]] == 1 and w.from_index.n_known == w.h.n_elements  # (the resolver knows every key)
    fn_ix, flag_ix = fieldnorms(w.from_index)
    fn_docs, flag_docs = fieldnorms(w.from_docs)
    assert flag_ix and not flag_docs
    assert np.array_equal(fn_ix[n > 0], fn_docs[n > 0]) and (fn_ix[n == 0] == 0).all()
    assert np.array_equal(fn_docs, w.h.download()["g_fieldnorm"])
    assert (w.from_index.n_docs, w.from_index.n_known, w.from_index.device) == (w.from_docs.n_docs, w.from_docs.n_known, w.from_docs.device)
    w.gix.bind()
    ms, counts = bind_stats()
    assert ms > 0 and counts == class_counts(n) and counts[2] >= 1 and counts[1] >= 2


def test_an_index_of_no_documents_binds_to_a_handle_of_no_documents():
    gix, keep = ev.empty_index()
    dt = gix.bind()
    assert (dt.n_docs, dt.n_known) == (0, 0) and bind_stats()[1] == (0, 0, 0)
    start, term, tf = dt.download()
    assert start.tolist() == [0] and len(term) == 0 and len(tf) == 0 and fieldnorms(dt)[1]
    assert dt.device_bytes() > 0
    with pytest.raises(vb.Vbm25Error, match="evaluate on an index without sealed documents") as e:  # (as a handle bound to such an index)
        dt.evaluate(np.zeros(1, np.uint32), np.array([0, 1], np.uint32))
    assert e.value.code == INVALID


# ---- 2. against numpy: host-built indexes from mappings


def mapping_lists(n_docs, holes):
    """posting lists over n_docs documents: terms of 1, 128 and 129 postings (one block, a full block, a block and a tail of one) as
    far as the documents allow, one document (the middle one) in every list; holes: documents 0, n_docs - 1 and two interior ones
    hold nothing"""
    rng = np.random.default_rng(n_docs * 2 + holes)
    every = n_docs // 2
    empty = [0, n_docs - 1, every - 1, n_docs // 3] if holes else []
    pool = np.setdiff1d(np.arange(n_docs), empty + [every])
    lists = []
    for size in (1, 128, 129, 2, 17, n_docs, 1, 64, 65):
        size = min(size, len(pool) + 1)
        others = rng.choice(pool, size - 1, replace=False) if size > 1 else np.zeros(0, np.int64)
        lists.append((np.sort(np.r_[others, every]).astype(np.int64), rng.integers(1, 9, size)))
    return lists, every


# (a single document cannot both hold every term and hold none: n_docs = 1 comes without holes)
@pytest.mark.parametrize("n_docs,holes", [(1, False)] + [(n, h) for n in (63, 64, 65, 129, 300) for h in (False, True)])
def test_host_built_indexes_against_a_numpy_transpose(n_docs, holes):
    lists, every = mapping_lists(n_docs, holes)
    seg = vb.Segment.build(1.2, 0.75, *build_args(n_docs, lists, seed=n_docs))
    gix = vb.GpuIndex(seg)
    want = transpose_lists(n_docs, lists)
    n = np.diff(want[0].astype(np.int64))
    assert n[every] == len(lists)
    sizes = {len(d) for d, _ in lists}
    if n_docs == 300 or (n_docs == 129 and not holes):
        assert {1, 128, 129} <= sizes
    if holes:
        assert n[0] == 0 and n[n_docs - 1] == 0 and n[every - 1] == 0 and n[n_docs // 3] == 0
    dt = gix.bind()
    assert_forward(dt, want, seg.arrays()["doc_fieldnorm"], f"{n_docs} documents, holes {holes}")
    assert bind_stats()[1] == class_counts(n)


# ---- 3. class edges

EDGE_RUNS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 5000)


@pytest.fixture(scope="module")
def edge_index():
    """one index whose documents hold 0, 1, 63 .. 5000 postings: document d holds a random set of EDGE_RUNS[d] of 5000 terms (the last
    one all of them)"""
    rng = np.random.default_rng(41)
    n_terms = max(EDGE_RUNS)
    holds = np.zeros((len(EDGE_RUNS), n_terms), bool)
    for d, run in enumerate(EDGE_RUNS):
        holds[d, rng.choice(n_terms, run, replace=False)] = True
    lists = [(np.flatnonzero(holds[:, t]), rng.integers(1, 1000, int(holds[:, t].sum()))) for t in range(n_terms)]
    keys = np.zeros((n_terms, 16), np.uint8)
    keys[:, :4] = np.arange(n_terms, dtype=">u4").view(np.uint8).reshape(-1, 4)
    args = build_args(len(EDGE_RUNS), lists, seed=3)
    seg = vb.Segment.build(1.2, 0.75, args[0], args[1], keys, *args[3:])
    want = transpose_lists(len(EDGE_RUNS), lists)
    assert np.diff(want[0].astype(np.int64)).tolist() == list(EDGE_RUNS)
    return seg, vb.GpuIndex(seg), want


SETTINGS = [dict(), dict(fwd_wave_max=8, fwd_group_max=65), dict(fwd_grid=1), dict(fwd_grid=3), dict(fwd_grid=1, fwd_wave_max=8, fwd_group_max=65),
            dict(fwd_wave_max=0, fwd_group_max=0), dict(fwd_wave_max=0), dict(fwd_wave_max=1, fwd_group_max=2047)]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k[4:]}={v}" for k, v in s.items()) or "defaults")
def test_the_class_edges_under_every_setting(edge_index, tuning, setting):
    seg, gix, want = edge_index
    tuning(**setting)
    dt = gix.bind()
    counts = bind_stats()[1]
    vb.reset_tuning()
    assert_forward(dt, want, seg.arrays()["doc_fieldnorm"], str(setting))
    assert counts == class_counts(EDGE_RUNS, setting.get("fwd_wave_max", WAVE_MAX), setting.get("fwd_group_max", GROUP_MAX))
    if not setting:
        assert counts == (4, 3, 2)
    if setting == dict(fwd_wave_max=8, fwd_group_max=65):
        assert counts == (2, 3, 4)


def test_the_bytes_are_identical_across_the_settings(edge_index, tuning):
    seg, gix, want = edge_index
    first = [a.tobytes() for a in gix.bind().download()] + [fieldnorms(gix.bind())[0].tobytes()]
    for setting in SETTINGS[1:]:
        vb.reset_tuning()
        tuning(**setting)
        dt = gix.bind()
        assert [a.tobytes() for a in dt.download()] + [fieldnorms(dt)[0].tobytes()] == first, setting


# ---- 4. every codec shape


def test_every_bit_width_of_full_blocks():
    lists = width_lists(1) + wide_tf_lists(1)
    seg = vb.Segment.build(1.2, 0.75, *build_args(WIDTH_DOCS, lists, 1))
    a = seg.arrays()
    assert_width_blocks(a)
    first = a["term_first_block"]
    assert [int(a["blk_meta_tf"][first[26 + i]]) for i in range(14)] == list(range(18, 32))
    dt = vb.GpuIndex(seg).bind()
    assert_forward(dt, transpose_lists(WIDTH_DOCS, lists), a["doc_fieldnorm"], "document widths 1 .. 25, tf widths 1 .. 31")


def test_byte_packed_tails():
    lists = tail_lists() + [wide_tf_tail()]
    seg = vb.Segment.build(1.2, 0.75, *build_args(TAIL_DOCS, lists))
    a = seg.arrays()
    assert_tail_blocks(a)
    j = a["term_first_block"][5]
    assert a["blk_meta_tf"][j] == 0x84 and a["blk_meta_doc"][j] == 0x83 and a["blk_n"][j] == 9
    dt = vb.GpuIndex(seg).bind()
    assert_forward(dt, transpose_lists(TAIL_DOCS, lists), a["doc_fieldnorm"], "byte-packed tails")


# ---- 5. from pages


def test_an_index_read_from_pages_binds_as_its_source(big):
    pages = big.dseg.to_relation(seed=cm.SEED)
    gix = vb.GpuIndex(vb.DeviceSegment.from_pages(pages))
    dt = gix.bind()
    assert_arrays(dt.download(), big.from_index.download(), "from pages")
    assert np.array_equal(fieldnorms(dt)[0], fieldnorms(big.from_index)[0])


# ---- 6. scores


def small_docs():
    """80 documents: a corpus over 46 lexemes and documents of 0, 1, 63, 64, 65, 130 and 2049 elements"""
    docs = cm.corpus(ev.KNOWN[:46], 73, seed=19)
    for n in (0, 1, 63, 64, 65, 130, 2049):
        docs.append([(t, 1 + i % 3) for i, t in enumerate(ev.KNOWN[:n])])
    return docs


def small_queries():
    rng = np.random.default_rng(29)

    def pick(n, top):
        return [ev.KNOWN[int(i)] for i in rng.choice(top, n, replace=False)]

    return [[], [ev.KNOWN[0]], [ev.UNKNOWN[3]], pick(5, 12), pick(5, 12) + [ev.UNKNOWN[1]], pick(8, 30), pick(8, 46), pick(3, 20), pick(64, 2049),
            pick(65, 300), pick(1, 5), pick(5, 8)]


def host_scores(seg, dl, term_ids, q_off, n_docs):
    """vb.evaluate for the cross product -> float64 [nq, n_docs]: the documents from Documents.download(), the queries from the ids' keys"""
    vocab = [bytes(k) for k in seg.arrays()["term_key"].reshape(-1, 16)]
    key = np.asarray(dl["g_key"]).reshape(-1, 16)
    start = dl["g_start"].astype(np.int64)
    docs = [([bytes(k) for k in key[start[d]:start[d + 1]]], dl["g_tf"][start[d]:start[d + 1]]) for d in range(n_docs)]
    out = np.zeros((len(q_off) - 1, n_docs), np.float64)
    for q in range(len(q_off) - 1):
        query = vb.Query([vocab[t] for t in term_ids[q_off[q]:q_off[q + 1]] if t < len(vocab)])
        for d in range(n_docs):
            out[q, d] = vb.evaluate(seg, docs[d][0], docs[d][1], query)
    return out


@pytest.mark.parametrize("k1", [1.2, 2.0])
@pytest.mark.parametrize("b", [0.0, 0.75, 1.0])
def test_scores_equal_the_host_function_on_the_source_documents(k1, b):
    docs = small_docs()
    w = DocWorld(docs, None, k1, b)
    term_ids, q_off = w.resolve(small_queries())
    nq, n_docs = len(q_off) - 1, len(docs)
    want = host_scores(w.dseg.download(), w.h.download(), term_ids, q_off, n_docs)
    assert (want != 0).mean() > 0.2
    cross = w.from_index.evaluate(term_ids, q_off)
    assert cross.shape == want.shape and np.array_equal(ev.bits(cross), ev.bits(want))
    rng = np.random.default_rng(5)
    sizes = [0, 1, 63, 64, 65, n_docs]
    lists = [np.arange(n_docs) if sizes[q % 6] == n_docs else rng.choice(n_docs, sizes[q % 6], replace=False) for q in range(nq)]
    q_cand, cand_doc = lists_csr(lists)
    got = w.from_index.evaluate(term_ids, q_off, q_cand, cand_doc)
    q_of = np.repeat(np.arange(nq), [len(l) for l in lists])
    assert np.array_equal(ev.bits(got), ev.bits(want[q_of, cand_doc]))
    assert np.array_equal(ev.bits(got), ev.bits(w.from_docs.evaluate(term_ids, q_off, q_cand, cand_doc)))


@pytest.mark.parametrize("k", [1, 10, 1024])
def test_the_scorer_and_the_ring_on_the_index_bound_handle(big, k):
    w = big
    queries = ev.query_batch()
    term_ids, q_off = w.resolve(queries)
    q_cand, cand_doc = ev.candidate_lists(len(queries), len(w.docs))
    with w.from_docs.scorer() as s_docs, w.from_index.scorer() as s_ix:
        for lists in ((q_cand, cand_doc), (None, None)):
            want = s_docs.topk(term_ids, q_off, k, *lists)
            same(s_ix.topk(term_ids, q_off, k, *lists), want, f"scorer k={k}")
            with w.from_index.reranker(w.resolver, 2, **CAPS) as r_ix, w.from_docs.reranker(w.resolver, 2, **CAPS) as r_docs:
                got = through(r_ix, queries, k, *lists)
                same(got, want, f"ring k={k}")
                same(got, through(r_docs, queries, k, *lists), f"ring against ring k={k}")
    assert np.array_equal(ev.bits(w.from_index.evaluate(term_ids, q_off)), ev.bits(w.from_docs.evaluate(term_ids, q_off)))


# ---- 7. ctids


@pytest.mark.parametrize("n", [1, 4, 65, 5000])
def test_ctids_from_the_index_equal_ctids_from_the_documents(n):
    """the ctid lists of tests/test_gpu_reranker.py: absent ctids first, last and alone, repeats, two documents sharing a payload, the
    two extreme keys"""
    docs, pay = ctid_world(n)
    w = DocWorld(docs, pay)
    assert_arrays(w.from_index.download(), w.from_docs.download(), f"{n} documents")
    q_cand, cand_tid = ctid_lists(pay, np.random.default_rng(n))
    queries = [ev.query_batch()[q] for q in (7, 1, 8, 13, 27, 35, 9, 10, 5)]
    ids, off = w.resolve(queries)
    with w.from_index.reranker(w.resolver, 2, from_index=True, **CAPS) as r_ix, w.from_docs.reranker(w.resolver, 2, documents=w.h, **CAPS) as r_docs:
        assert r_ix.device_bytes() == r_docs.device_bytes()
        for k in (10, 300):
            got = through(r_ix, queries, k, q_cand, cand_tid=cand_tid)
            same(got, through(r_docs, queries, k, q_cand, cand_tid=cand_tid), f"{n} documents, k={k}")
        assert got[1][1] == 1 and got[1][6] == 0 and got[1][7] == 0 and got[1][2] == 58
        r_ix.submit_ids(ids, off, 10, q_cand, cand_tid=cand_tid)
        r_docs.submit_ids(ids, off, 10, q_cand, cand_tid=cand_tid)
        same(r_ix.collect(), r_docs.collect(), f"{n} documents, ids and ctids")
    # vbm25_reranker_create itself on the index-bound handle without payloads: a ring without ctids
    with w.from_index.reranker(w.resolver, 1, **CAPS) as plain:
        with pytest.raises(vb.Vbm25Error, match="cand_tid on a reranker created without payloads"):
            plain.submit(queries, 10, q_cand, cand_tid=cand_tid)


# ---- 8. after a compaction


def test_the_bind_after_a_compaction(big):
    seg = big.dseg.download()
    rng = np.random.default_rng(13)
    deleted = rng.random(seg.n_docs) < 0.3
    deleted[ev.EDGE["5000 elements"]] = False
    deleted[ev.EDGE["2048 elements"]] = True
    ds = vb.DeviceSegment.maintain(big.gix, deleted)
    args, _ = maintain(seg.arrays(), seg.meta(), deleted, None)
    want_seg = vb.Segment.build(*args)
    n_docs = int((~deleted).sum())
    assert ds.n_docs == n_docs == want_seg.n_docs
    want = transpose(n_docs, args[5], args[6], args[7])
    dt = vb.GpuIndex(ds).bind()
    assert_forward(dt, want, want_seg.arrays()["doc_fieldnorm"], "after maintain")
    assert 0 < dt.n_known < big.from_index.n_known


# ---- 9. refusals


def last_error():
    return vb.lib().vbm25_last_error().decode()


def test_refusals_with_code_and_message(big):
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_index_bind(None, C.byref(out)) == INVALID and not out.value and last_error() == "NULL argument"
    assert L.vbm25_index_bind(big.gix.h, None) == INVALID and last_error() == "out is NULL"
    caps = [2, 64, 4096, 1 << 18, 40000, 1024]

    def create(t, r, *c, out=True):
        h = C.c_void_p(1)
        rc = L.vbm25_reranker_create_from_index(t, r, *c, C.byref(h) if out else None)
        assert not out or not h.value
        return rc, last_error()

    assert create(big.from_index.h, big.resolver.h, *caps, out=False) == (INVALID, "out is NULL")
    assert create(None, big.resolver.h, *caps) == (INVALID, "NULL argument")
    assert create(big.from_index.h, None, *caps) == (INVALID, "NULL argument")
    assert create(big.from_docs.h, big.resolver.h, *caps) == (INVALID, "the bound documents were not made by vbm25_index_bind: their ctids are not the index's")
    with pytest.raises(vb.Vbm25Error) as e:
        big.from_docs.reranker(big.resolver, 2, from_index=True, **CAPS)
    assert e.value.code == INVALID
    # every other check is vbm25_reranker_create's, with its words
    assert create(big.from_index.h, big.resolver.h, 17, *caps[1:]) == (INVALID, "depth 17 is outside 1 .. 16")
    assert create(big.from_index.h, big.resolver.h, *caps[:5], 1025) == (UNSUPPORTED, "k is 1025: a scorer returns at most 1024 candidates a query")
    other = DocWorld(small_docs()[:10])
    assert create(big.from_index.h, other.resolver.h, *caps) == (INVALID, "the documents are bound to another index than the resolver's")
    gix, keep = ev.empty_index()
    r0 = vb.Resolver(gix, 1, 4, 16, 256, seed=cm.SEED)
    assert create(gix.bind().h, r0.h, *caps) == (INVALID, "evaluate on an index without sealed documents")


@pytest.mark.parametrize("name,bound", [("fwd_grid", 2048), ("fwd_wave_max", 64), ("fwd_group_max", 2048)])
def test_each_tuning_bound(name, bound):
    try:
        for value in (0, 1, bound):
            vb.set_tuning(name, value)
        for value in (-1, bound + 1, 1 << 40):
            with pytest.raises(vb.Vbm25Error, match=rf"{name} {value} is outside 0 \.\. {bound}") as e:
                vb.set_tuning(name, value)
            assert e.value.code == INVALID
    finally:
        vb.reset_tuning()


# ---- 10. buffers and threads


def test_two_binds_of_one_index_are_equal(big):
    a, b = big.gix.bind(), big.gix.bind()
    assert [x.tobytes() for x in a.download()] == [x.tobytes() for x in b.download()]
    assert fieldnorms(a)[0].tobytes() == fieldnorms(b)[0].tobytes()
    assert a.device_bytes() == b.device_bytes() == big.from_index.device_bytes()
    assert a.device_bytes() == 8 * (a.n_docs + 1) + 8 * a.n_known + a.n_docs


def test_two_threads_bind_two_indexes_at_once(big, edge_index):
    seg, gix, want = edge_index
    worlds = [(big.gix, big.from_index.download()), (gix, want)]
    errors = []

    def work(i):
        try:
            for _ in range(3):
                assert_arrays(worlds[i][0].bind().download(), worlds[i][1], f"thread {i}")
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
