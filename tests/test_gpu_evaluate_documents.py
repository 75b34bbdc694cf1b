"""The `<&>` operator from cast documents on the GPU (csrc/evaluate.hip): Documents.bind array for array against lookup_terms on the
host, DocTerms.evaluate bit for bit against vb.evaluate (the host function) on the downloaded documents and the resolved ids' keys --
candidate lists and the cross product, several grid turns, the fieldnorm and length edges, every (k1, b) corner, both routes into the
index, the refusals message for message, two threads on one handle.  -m gpu only."""
import threading

import numpy as np
import pytest

import cast_model as cm
import vectorchord_bm25_amd as vb

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
MISS = 0xFFFFFFFF

KNOWN = cm.words(6000)                                        # the index's vocabulary
UNKNOWN = cm.words(40, b"u") + [b"\x01a", b"\x01b"]           # lexemes the index lacks; the last two sort in front of every known key
LATER = [b"\xff\xff\xff-%d" % i for i in range(4)]            # ... and these behind every known key


def index_docs(known, n_docs=250):
    """documents that hold every lexeme of `known` at least once, the first ones often"""
    docs = cm.corpus(known[:50], n_docs, seed=3)
    for i, d in enumerate(docs):
        d.extend((known[j], 1 + j % 3) for j in range(i, len(known), n_docs))
    return docs


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class World:
    """one index (host segment + GpuIndex + Resolver) and what the tests need of it"""

    def __init__(self, known, k1=1.2, b=0.75, device_route=False):
        docs = index_docs(known)
        pay = cm.payloads(len(docs))
        self.model = cm.shared(("eval index", len(known), known[0], known[-1]), lambda: cm.cast(docs, pay))
        self.seg = cm.build_segment(self.model, k1, b)  # (the host segment: vb.evaluate's statistics, whichever way the index was made)
        if device_route:
            self.gix = vb.GpuIndex(vb.DeviceSegment.from_documents(vb.Documents.cast(docs, pay, seed=cm.SEED), k1, b))
        else:
            self.gix = vb.GpuIndex(self.seg)
        self.vocab = [bytes(k) for k in self.seg.arrays()["term_key"].reshape(-1, 16)]
        assert len(self.vocab) == len(known)
        self.resolver = vb.Resolver(self.gix, 1, 64, 4096, 1 << 18, seed=cm.SEED)

    def resolve(self, queries):
        self.resolver.submit(queries)
        return self.resolver.collect()

    def reference(self, dl, term_ids, q_off, pairs):
        """vb.evaluate for (query, document) pairs -> float64, the document from Documents.download(), the query from the ids' keys"""
        key = np.asarray(dl["g_key"]).reshape(-1, 16)
        start = dl["g_start"].astype(np.int64)
        doc_cache, query_cache, out = {}, {}, np.zeros(len(pairs), dtype=np.float64)
        for i, (q, d) in enumerate(pairs):
            if d not in doc_cache:
                doc_cache[d] = ([bytes(k) for k in key[start[d]:start[d + 1]]], dl["g_tf"][start[d]:start[d + 1]])
            if q not in query_cache:
                query_cache[q] = vb.Query([self.vocab[t] for t in term_ids[q_off[q]:q_off[q + 1]]])
            out[i] = vb.evaluate(self.seg, doc_cache[d][0], doc_cache[d][1], query_cache[q])
        return out


def bind_model(dl, gix):
    """Documents.download() + GpuIndex.lookup_terms, the misses dropped -> (start, term, tf)"""
    key = np.ascontiguousarray(np.asarray(dl["g_key"]).reshape(-1, 16))
    uniq, inv = np.unique(key.view("V16").ravel(), return_inverse=True)
    ids = gix.lookup_terms([bytes(u) for u in uniq])[inv.ravel()] if len(uniq) else np.zeros(0, np.uint32)
    known = ids != MISS
    prefix = np.concatenate([[0], np.cumsum(known)]).astype(np.uint64)
    return prefix[dl["g_start"].astype(np.int64)], ids[known].astype(np.uint32), dl["g_tf"][known]


def assert_bound(dt, dl, gix, what):
    start, term, tf = dt.download()
    want = bind_model(dl, gix)
    for got, w, name in zip((start, term, tf), want, ("start", "term", "tf")):
        assert got.dtype == w.dtype and np.array_equal(got, w), f"{what}: {name} differs"
    assert dt.n_docs == len(dl["g_start"]) - 1 and dt.n_known == len(want[1])
    assert dt.device_bytes() >= 8 * (dt.n_docs + 1) + 8 * dt.n_known + dt.n_docs
    for d in range(dt.n_docs):  # what the kernel's bisection relies on
        run = term[int(start[d]):int(start[d + 1])].astype(np.int64)
        assert (np.diff(run) > 0).all(), f"{what}: document {d}'s ids do not ascend strictly"


EDGE = {}  # name -> index among the scored documents


def scored_docs():
    """about 300 documents: a Zipf-ish corpus over known and unknown lexemes interleaved, and the edge documents"""
    pool = []
    for i in range(46):
        pool.append(KNOWN[i])
        if i % 5 == 2:
            pool.append(UNKNOWN[i // 5])
    docs = cm.corpus(pool, 285, seed=11)
    edge = [
        ("no elements", []),
        ("all unknown", [(u, 2) for u in UNKNOWN[:7]]),
        ("unknown first", [(UNKNOWN[40], 3), (UNKNOWN[41], 1), (KNOWN[0], 2), (KNOWN[1], 1)]),
        ("unknown last", [(KNOWN[0], 1), (KNOWN[3], 2), (LATER[0], 4), (LATER[1], 1)]),
        ("unknown interleaved", [(t, 1 + i % 2) for i, t in enumerate(sum(([KNOWN[i], UNKNOWN[i]] for i in range(12)), []))]),
        ("1 element", [(KNOWN[1], 7)]),
        ("63 elements", [(t, 1) for t in KNOWN[:63]]),
        ("64 elements", [(t, 2) for t in KNOWN[:64]]),
        ("65 elements", [(t, 1) for t in KNOWN[:65]]),
        ("2048 elements", [(t, 1 + i % 3) for i, t in enumerate(KNOWN[:2048])]),
        ("5000 elements", [(t, 1 + i % 2) for i, t in enumerate(KNOWN[:4990] + UNKNOWN[:10])]),
    ]
    for name, d in edge:
        EDGE[name] = len(docs)
        docs.append(d)
    return docs


def query_batch():
    """about 40 queries of 0, 1, 5, 8, 64, 65 and 300 lexemes, some lexemes unknown, some behind the vocabulary"""
    rng = np.random.default_rng(17)

    def pick(n, top):
        return [KNOWN[int(i)] for i in rng.choice(top, n, replace=False)]

    qs = [[], [KNOWN[0]], [UNKNOWN[3]], [LATER[2]], UNKNOWN[:5] + LATER[:2]]
    for _ in range(8):
        qs.append(pick(5, 12))
    for _ in range(6):
        qs.append(pick(3, 20) + [UNKNOWN[int(rng.integers(40))], LATER[int(rng.integers(4))]])
    for _ in range(6):
        qs.append(pick(8, 30))
    for _ in range(4):
        qs.append(pick(60, 300) + UNKNOWN[:3] + [LATER[3]])   # 64
    for _ in range(4):
        qs.append(pick(65, 5000))
    for _ in range(3):
        qs.append(pick(250, 6000) + UNKNOWN[:40] + LATER + UNKNOWN[40:] + KNOWN[:4])  # 300, the frequent lexemes among them
    qs += [pick(1, 5), pick(1, 6000), [], pick(5, 8)]
    return qs


def candidate_lists(nq, n_docs):
    """per query a list of 0, 1, 63, 64, 65 or all documents; one list descending, one with repeats"""
    rng = np.random.default_rng(23)
    sizes = [0, 1, 63, 64, 65, n_docs]
    lists = []
    for q in range(nq):
        n = sizes[q % len(sizes)]
        lists.append(np.arange(n_docs) if n == n_docs else rng.choice(n_docs, n, replace=False))
    lists[8] = np.sort(lists[8])[::-1]                                  # 63 documents, descending
    lists[9] = np.concatenate([lists[9][:32], lists[9][:32]])            # 64 entries, every document twice
    lists[11] = rng.permutation(n_docs)                                  # all documents, shuffled
    # the edge documents are in the lists that hold every document; put them into a short one as well
    lists[10] = np.concatenate([lists[10][:65 - len(EDGE)], np.array(sorted(EDGE.values()))])
    q_cand = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    return q_cand, np.concatenate(lists).astype(np.uint32)


@pytest.fixture(scope="module")
def world():
    return World(KNOWN)


@pytest.fixture(scope="module")
def main(world):
    """the main batch: handle, download, bound handle, resolved queries, candidate lists and the reference's cross product (computed
    once; the candidate lists' reference is read out of it)"""
    docs = scored_docs()
    h = vb.Documents.cast(docs, None, seed=cm.SEED)
    dl = h.download()
    dt = h.bind(world.resolver)
    term_ids, q_off = world.resolve(query_batch())
    nq, n_docs = len(q_off) - 1, len(docs)
    ref = world.reference(dl, term_ids, q_off, [(q, d) for q in range(nq) for d in range(n_docs)]).reshape(nq, n_docs)
    ref.setflags(write=False)
    q_cand, cand_doc = candidate_lists(nq, n_docs)
    return dict(h=h, dl=dl, dt=dt, term_ids=term_ids, q_off=q_off, nq=nq, n_docs=n_docs, ref=ref, q_cand=q_cand, cand_doc=cand_doc)


def list_reference(m):
    q_of = np.repeat(np.arange(m["nq"]), np.diff(m["q_cand"].astype(np.int64)))
    return m["ref"][q_of, m["cand_doc"]]


def test_the_bind_equals_lookup_terms_on_the_host(world, main):
    assert_bound(main["dt"], main["dl"], world.gix, "the main batch")
    start, term, _ = main["dt"].download()
    n = np.diff(start.astype(np.int64))
    assert n[EDGE["no elements"]] == 0 and n[EDGE["all unknown"]] == 0 and n[EDGE["unknown first"]] == 2 and n[EDGE["unknown last"]] == 2
    assert n[EDGE["unknown interleaved"]] == 12 and n[EDGE["1 element"]] == 1
    assert [n[EDGE[f"{k} elements"]] for k in (63, 64, 65, 2048, 5000)] == [63, 64, 65, 2048, 4990]
    assert main["dt"].n_known < main["h"].n_elements


def test_a_handle_of_no_documents_binds_and_scores_nothing(world):
    h = vb.Documents.cast([], None, seed=cm.SEED)
    dt = h.bind(world.resolver)
    assert (dt.n_docs, dt.n_known) == (0, 0)
    start, term, tf = dt.download()
    assert start.tolist() == [0] and len(term) == 0 and len(tf) == 0
    term_ids, q_off = world.resolve([[KNOWN[0]], []])
    assert dt.evaluate(term_ids, q_off).shape == (2, 0)
    assert len(dt.evaluate(term_ids, q_off, np.zeros(3, np.uint64), np.zeros(0, np.uint32))) == 0


def test_the_bind_kernels_second_grid_turn(tuning):
    """70 000 two-lexeme documents, every bind kernel capped to 8 workgroups: 2048 lanes for 140 000 elements, 32 waves for 70 000
    documents -- many grid-stride turns of each"""
    known = [b"w%d" % i for i in range(0, 977, 2)] + [b"x%d" % i for i in range(0, 31, 3)]
    w = World(known)
    tuning(eval_grid=8)
    h = vb.Documents.cast(cm.grid_stride_docs(), None, seed=cm.SEED)
    dt = h.bind(w.resolver)
    vb.reset_tuning()
    dl = h.download(with_length=False)
    start, term, tf = dt.download()
    want = bind_model(dl, w.gix)
    assert np.array_equal(start, want[0]) and np.array_equal(term, want[1]) and np.array_equal(tf, want[2])
    assert 0 < dt.n_known < h.n_elements


def test_candidate_lists_score_as_the_host_function(main):
    m = main
    got = m["dt"].evaluate(m["term_ids"], m["q_off"], m["q_cand"], m["cand_doc"])
    want = list_reference(m)
    assert got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), f"{(bits(got) != bits(want)).sum()} of {len(want)} scores differ"
    sizes = set(np.diff(m["q_cand"].astype(np.int64)).tolist())
    assert {0, 1, 63, 64, 65, m["n_docs"]} <= sizes


def test_the_cross_product_scores_as_the_host_function(main):
    m = main
    got = m["dt"].evaluate(m["term_ids"], m["q_off"])
    assert got.shape == (m["nq"], m["n_docs"])
    assert np.array_equal(bits(got), bits(m["ref"]))
    nonzero = m["ref"] != 0.0
    assert nonzero.mean() >= 1 / 3, f"only {nonzero.mean():.2f} of the reference's pairs score"
    assert (bits(got)[~nonzero] == 0).all()  # (exactly +0.0: an absent term adds nothing)
    # the generator's queries have the lengths the issue asks for, before and after the resolver
    assert np.diff(m["q_off"].astype(np.int64)).max() > 64


@pytest.mark.parametrize("grid", [1, 3])
def test_many_grid_turns_give_identical_bytes(main, tuning, grid):
    m = main
    tuning(eval_grid=grid)
    lists = m["dt"].evaluate(m["term_ids"], m["q_off"], m["q_cand"], m["cand_doc"])
    cross = m["dt"].evaluate(m["term_ids"], m["q_off"])
    assert np.array_equal(bits(lists), bits(list_reference(m))) and np.array_equal(bits(cross), bits(m["ref"]))


SMALL = cm.words(50)


def fieldnorm_docs():
    """one-lexeme documents whose counts are the FIELDNORM_TO_LENGTH entries (the entry 0 is the document without lexemes), 2^32 - 1,
    two lexemes whose counts saturate the sum, and a document whose length comes mostly from unknown keys"""
    table = cm.fieldnorm_table()
    docs = [[(SMALL[1], int(c))] if c else [] for c in table]
    docs.append([(SMALL[1], cm.U32_MAX)])
    docs.append([(SMALL[1], 0x80000000), (SMALL[2], 0x80000005)])
    docs.append([(SMALL[1], 1), (UNKNOWN[0], 4000), (UNKNOWN[41], 999)])
    docs.append([(SMALL[1], 1)])
    return docs


@pytest.mark.parametrize("k1", [1.2, 2.0])
@pytest.mark.parametrize("b", [0.0, 0.75, 1.0])
def test_fieldnorm_length_and_the_bm25_parameters(k1, b):
    w = World(SMALL, k1, b)
    docs = fieldnorm_docs()
    h = vb.Documents.cast(docs, None, seed=cm.SEED)
    dl = h.download()
    assert len(set(dl["g_fieldnorm"][:256].tolist())) == 256 and dl["length"][256] == cm.U32_MAX and dl["length"][257] == cm.U32_MAX
    assert dl["g_fieldnorm"][258] != dl["g_fieldnorm"][259]  # (the unknown keys' 4999 positions count for the length)
    dt = h.bind(w.resolver)
    term_ids, q_off = w.resolve([[SMALL[1]], [SMALL[2], SMALL[1], UNKNOWN[0]], [SMALL[0], SMALL[2]]])
    got = dt.evaluate(term_ids, q_off)
    want = w.reference(dl, term_ids, q_off, [(q, d) for q in range(3) for d in range(len(docs))]).reshape(3, len(docs))
    assert np.array_equal(bits(got), bits(want))
    # documents 258 and 259 hold the query's lexeme once each and differ in their length only: b decides whether that shows
    assert got[0, 258] != got[0, 259] if b else got[0, 258] == got[0, 259]
    assert (got[0, 1:258] > 0).all() and got[0, 0] == 0


def test_an_index_from_documents_scores_as_a_host_built_one(world, main):
    m = main
    dev = World(KNOWN, device_route=True)
    dt = m["h"].bind(dev.resolver)
    assert_bound(dt, m["dl"], dev.gix, "the index from documents")
    term_ids, q_off = dev.resolve(query_batch())
    assert np.array_equal(term_ids, m["term_ids"]) and np.array_equal(q_off, m["q_off"])
    assert np.array_equal(bits(dt.evaluate(term_ids, q_off)), bits(m["ref"]))


def empty_index():
    arrays = {k: np.zeros(0, dtype=t) for k, t in vb.api._DESC_ARRAYS}
    arrays["term_first_block"] = np.zeros(1, dtype=np.uint32)
    arrays["blk_off8"] = np.zeros(1, dtype=np.uint32)
    desc, keep = vb.api.desc_from_arrays(dict(n_docs=0, n_terms=0, n_blocks=0, sum_len=0, k1=1.2, b=0.75), arrays)
    return vb.GpuIndex(desc), keep


def test_refusals_message_for_message(world, main):
    m = main
    dt, ids, off, qc, cd = m["dt"], m["term_ids"], m["q_off"], m["q_cand"], m["cand_doc"]

    def refused(match, *args):
        with pytest.raises(vb.Vbm25Error, match=match) as e:
            dt.evaluate(*args)
        assert e.value.code == INVALID

    q = 7  # (a query of five ids)
    bad = ids.copy()
    bad[off[q] + 1], bad[off[q] + 2] = ids[off[q] + 2], ids[off[q] + 1]
    refused(rf"query {q}: term ids must be strictly ascending", bad, off, qc, cd)
    dup = ids.copy()
    dup[off[q] + 1] = ids[off[q]]
    refused(rf"query {q}: term ids must be strictly ascending", dup, off)
    far = cd.copy()
    at = int(qc[5])  # (the first candidate of query 5, the first list of every document)
    far[at + 2] = m["n_docs"]
    refused(rf"query 5: candidate {m['n_docs']} is outside the handle's {m['n_docs']} documents", ids, off, qc, far)
    o = off.copy()
    o[0] = 1
    refused(r"q_off\[0\] is 1, not 0", ids, o, qc, cd)
    o = off.copy()
    assert o[3] >= 1
    o[4] = o[3] - 1
    refused(r"q_off is not monotone at query 3", ids, o, qc, cd)
    c = qc.copy()
    c[0] = 2
    refused(r"q_cand\[0\] is 2, not 0", ids, off, c, cd)
    c = qc.copy()
    c[3] = c[2] - 1
    refused(r"q_cand is not monotone at query 2", ids, off, c, cd)
    refused(r"cand_doc is NULL while q_cand is not", ids, off, qc, None)
    L = vb.lib()
    one = np.zeros(1, np.float64)
    assert L.vbm25_evaluate_documents(dt.h, None, off.ctypes.data, m["nq"], None, None, one.ctypes.data) == INVALID
    assert b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_evaluate_documents(dt.h, ids.ctypes.data, off.ctypes.data, m["nq"], None, None, None) == INVALID
    # 2^31 pairs or more: counted from the offsets, before any array is looked at
    huge, none = np.array([0, 1 << 31], dtype=np.uint64), np.zeros(2, np.uint32)
    assert L.vbm25_evaluate_documents(dt.h, none.ctypes.data, none.ctypes.data, 1, huge.ctypes.data, none.ctypes.data, one.ctypes.data) == UNSUPPORTED
    assert b"2147483648 pairs: one call scores fewer than 2^31" in L.vbm25_last_error()
    # nq == 0 and queries without candidates are legal and write nothing
    assert L.vbm25_evaluate_documents(dt.h, None, None, 0, None, None, None) == 0
    assert len(dt.evaluate(ids, off, np.zeros(m["nq"] + 1, np.uint64), np.zeros(0, np.uint32))) == 0
    # after the refused calls the handle scores as before
    got = dt.evaluate(ids, off, qc, cd)
    assert np.array_equal(bits(got), bits(list_reference(m)))


def test_an_index_without_sealed_documents_is_refused(main):
    gix, keep = empty_index()
    r = vb.Resolver(gix, 1, 4, 16, 256, seed=cm.SEED)
    dt = main["h"].bind(r)
    assert dt.n_docs == main["n_docs"] and dt.n_known == 0
    r.submit([[KNOWN[0]]])
    term_ids, q_off = r.collect()
    with pytest.raises(vb.Vbm25Error, match="evaluate on an index without sealed documents") as e:
        dt.evaluate(term_ids, q_off)
    assert e.value.code == INVALID
    with pytest.raises(vb.Vbm25Error, match="evaluate on an index without sealed documents"):  # (vbm25_evaluate_batch's words)
        vb.evaluate_batch(gix, np.zeros(1, np.uint32), np.array([0, 1], np.uint64), np.zeros(1, np.uint32), np.ones(1, np.uint32))


def test_a_resolver_on_another_device_is_refused(main):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    other = World(SMALL)
    other_gix = vb.GpuIndex(other.seg, device=1)
    r = vb.Resolver(other_gix, 1, 4, 16, 256, seed=cm.SEED)
    with pytest.raises(vb.Vbm25Error, match="the documents are on device 0, the resolver's index is on device 1") as e:
        main["h"].bind(r)
    assert e.value.code == INVALID


def test_two_threads_score_on_one_handle(main):
    m = main
    half = m["nq"] // 2
    off, qc = m["q_off"], m["q_cand"]

    def part(lo, hi):
        return (m["term_ids"][off[lo]:off[hi]], off[lo:hi + 1] - off[lo], qc[lo:hi + 1] - qc[lo], m["cand_doc"][int(qc[lo]):int(qc[hi])])

    parts = [part(0, half), part(half, m["nq"])]
    single = [m["dt"].evaluate(*p) for p in parts]
    out, errors = [None, None], []

    def work(i):
        try:
            for _ in range(4):
                out[i] = m["dt"].evaluate(*parts[i])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert np.array_equal(bits(out[i]), bits(single[i]))
    assert np.array_equal(bits(np.concatenate(single)), bits(list_reference(m)))
