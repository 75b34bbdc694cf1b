"""The rerank step on the GPU (csrc/rerank.hip): a Scorer's evaluate bit for bit DocTerms.evaluate, and its topk byte for byte a stable
descending sort of DocTerms.evaluate's scores cut at k -- score bits, pos, doc, n_ranks and the zero tail -- over every k and list
length at which the selection takes another path, ties at the k-th place, many parts, many cuts, many grid turns, the BM25 corners,
one scorer across growing and shrinking shapes, threads, and the refusals message for message.  The world is the one of
tests/test_gpu_evaluate_documents.py, whose helpers this file imports.  -m gpu only."""
import ctypes as C
import threading

import numpy as np
import pytest

import cast_model as cm
import test_gpu_evaluate_documents as ev
import vectorchord_bm25_amd as vb

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
KS = [1, 2, 10, 63, 64, 65, 256, 1000, 1024]
bits = ev.bits


def reference_topk(scores, q_cand, cand_doc, k, n_docs=None):
    """np.argsort(-scores, kind="stable")[:k] per query of DocTerms.evaluate's output -> (ranks, n_ranks)"""
    nq = len(scores) if q_cand is None else len(q_cand) - 1
    ranks, n_ranks = np.zeros((nq, k), dtype=vb.RANK_DTYPE), np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        if q_cand is None:
            s, docs = scores[q], np.arange(n_docs, dtype=np.uint32)
        else:
            lo, hi = int(q_cand[q]), int(q_cand[q + 1])
            s, docs = scores[lo:hi], np.asarray(cand_doc[lo:hi], dtype=np.uint32)
        order = np.argsort(-s, kind="stable")[:k]
        n_ranks[q] = len(order)
        ranks["score"][q, :len(order)] = s[order]
        ranks["pos"][q, :len(order)] = order
        ranks["doc"][q, :len(order)] = docs[order]
    return ranks, n_ranks


def assert_topk(scorer, dt, term_ids, q_off, k, q_cand=None, cand_doc=None, what=""):
    """Scorer.topk against the reference, byte for byte (RANK_DTYPE has no padding: the bytes are score bits, pos, doc, zero tail)"""
    scores = dt.evaluate(term_ids, q_off, q_cand, cand_doc)
    want, want_n = reference_topk(scores, q_cand, cand_doc, k, dt.n_docs)
    got, got_n = scorer.topk(term_ids, q_off, k, q_cand, cand_doc)
    assert got.dtype == vb.RANK_DTYPE and got.shape == want.shape and got_n.dtype == np.uint32
    assert np.array_equal(got_n, want_n), f"{what} k={k}: n_ranks differ at queries {np.flatnonzero(got_n != want_n)[:8]}"
    if got.tobytes() != want.tobytes():
        for q in range(len(want_n)):
            if got[q].tobytes() != want[q].tobytes():
                i = int(np.flatnonzero(got[q].view("V16") != want[q].view("V16"))[0])
                raise AssertionError(f"{what} k={k}: query {q} ({want_n[q]} ranks) differs first at entry {i}: got {got[q, i]}, want {want[q, i]}")
    return got, got_n


def take_queries(term_ids, q_off, idx):
    """the CSR of the queries `idx`, in that order"""
    ids = [term_ids[q_off[q]:q_off[q + 1]] for q in idx]
    off = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.uint32)
    return (np.concatenate(ids) if ids else np.zeros(0)).astype(np.uint32), off


def lists_csr(lists):
    q_cand = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    return q_cand, (np.concatenate(lists) if lists else np.zeros(0)).astype(np.uint32)


@pytest.fixture(scope="module")
def world():
    return ev.World(ev.KNOWN)


@pytest.fixture(scope="module")
def rr(world):
    """the documents and queries of the evaluate tests, bound, and one scorer for the module"""
    docs = ev.scored_docs()
    h = vb.Documents.cast(docs, None, seed=cm.SEED)
    dt = h.bind(world.resolver)
    term_ids, q_off = world.resolve(ev.query_batch())
    nq, n_docs = len(q_off) - 1, len(docs)
    q_cand, cand_doc = ev.candidate_lists(nq, n_docs)
    cross = dt.evaluate(term_ids, q_off)
    cross.setflags(write=False)
    # the queries that score most documents differently: for the lists that need many distinct scores
    distinct = [len(np.unique(cross[q])) for q in range(nq)]
    return dict(h=h, dt=dt, scorer=dt.scorer(), term_ids=term_ids, q_off=q_off, nq=nq, n_docs=n_docs, q_cand=q_cand, cand_doc=cand_doc,
                cross=cross, rich=int(np.argmax(distinct)), distinct=distinct)


def test_scorer_evaluate_has_the_bits_of_the_plain_call(rr):
    m = rr
    lists = m["scorer"].evaluate(m["term_ids"], m["q_off"], m["q_cand"], m["cand_doc"])
    want = m["dt"].evaluate(m["term_ids"], m["q_off"], m["q_cand"], m["cand_doc"])
    assert lists.shape == want.shape and np.array_equal(bits(lists), bits(want))
    cross = m["scorer"].evaluate(m["term_ids"], m["q_off"])
    assert cross.shape == (m["nq"], m["n_docs"]) and np.array_equal(bits(cross), bits(m["cross"]))
    assert (m["cross"] != 0).mean() >= 1 / 3
    assert len(m["scorer"].evaluate(m["term_ids"], m["q_off"], np.zeros(m["nq"] + 1, np.uint64), np.zeros(0, np.uint32))) == 0


@pytest.mark.parametrize("k", KS)
def test_topk_of_the_main_batch(rr, k):
    """candidate lists of 0, 1, 63, 64, 65 and all documents, one descending, one with every document twice, one shuffled; then the
    cross product"""
    m = rr
    _, n = assert_topk(m["scorer"], m["dt"], m["term_ids"], m["q_off"], k, m["q_cand"], m["cand_doc"], "lists")
    sizes = np.diff(m["q_cand"].astype(np.int64))
    assert np.array_equal(n, np.minimum(sizes, k)) and {0, 1, 63, 64, 65, m["n_docs"]} <= set(sizes.tolist())
    got, n = assert_topk(m["scorer"], m["dt"], m["term_ids"], m["q_off"], k, what="cross")
    assert (n == min(k, m["n_docs"])).all() and np.array_equal(got["pos"], got["doc"])


@pytest.mark.parametrize("k", KS)
def test_list_lengths_around_k(rr, k):
    """lists of 0, 1, 63, 64, 65, k - 1, k, k + 1, 2k and 2k + 1 entries, drawn with repetition (they outgrow the documents)"""
    m = rr
    rng = np.random.default_rng(100 + k)
    sizes = [0, 1, 63, 64, 65, k - 1, k, k + 1, 2 * k, 2 * k + 1]
    queries = [m["rich"], 7, 20, 27, 31, 35, 1, 12, 24, 33]  # (5, 8, 64, 65 and 300 lexemes among them)
    ids, off = take_queries(m["term_ids"], m["q_off"], queries)
    q_cand, cand_doc = lists_csr([rng.integers(0, m["n_docs"], n) for n in sizes])
    _, n = assert_topk(m["scorer"], m["dt"], ids, off, k, q_cand, cand_doc, "lengths around k")
    assert n.tolist() == [min(s, k) for s in sizes]


@pytest.mark.parametrize("k", [10, 64, 1024])
def test_5000_entries_with_repetition(rr, k):
    """many ties across many 64-candidate items (and, at the default part size, several parts whose lists are merged)"""
    m = rr
    rng = np.random.default_rng(5)
    ids, off = take_queries(m["term_ids"], m["q_off"], [m["rich"], 8])
    q_cand, cand_doc = lists_csr([rng.integers(0, m["n_docs"], 5000), rng.integers(0, 300, 5000) % m["n_docs"]])
    got, n = assert_topk(m["scorer"], m["dt"], ids, off, k, q_cand, cand_doc, "5000 entries")
    assert n.tolist() == [k, k]
    assert len(np.unique(got["score"][0])) < k  # (5000 draws of about 300 documents: ties inside the row)


def test_a_query_of_unknown_terms_returns_the_first_positions(rr):
    m = rr
    ids, off = take_queries(m["term_ids"], m["q_off"], [2, 4])  # ([UNKNOWN[3]] and a query of unknown and later lexemes)
    rng = np.random.default_rng(6)
    q_cand, cand_doc = lists_csr([rng.integers(0, m["n_docs"], 3000), rng.integers(0, m["n_docs"], 3000)])
    got, n = assert_topk(m["scorer"], m["dt"], ids, off, 10, q_cand, cand_doc, "all-zero scores")
    assert n.tolist() == [10, 10]
    for q in range(2):
        assert got["pos"][q].tolist() == list(range(10)) and (bits(got["score"][q]) == 0).all()
        assert np.array_equal(got["doc"][q], cand_doc[int(q_cand[q]):int(q_cand[q]) + 10])


@pytest.mark.parametrize("k", [1, 10, 64])
def test_a_tie_straddles_the_kth_place(rr, k):
    """the k-th and the (k + 1)-th best entry are the same document at two positions: the smaller position is in, the larger out --
    with the pair close together, 300 entries apart (other waves, another round) and in different parts"""
    m = rr
    q = m["rich"]
    s = m["cross"][q]
    values, first = np.unique(s, return_index=True)  # ascending scores, one document each
    assert len(values) >= k + 40, f"query {q} has {len(values)} distinct scores"
    by_score = first[::-1]  # one document per distinct score, best first
    top, tied, rest = by_score[:k - 1], int(by_score[k - 1]), by_score[k:k + 39]
    rng = np.random.default_rng(40 + k)
    ids, off = take_queries(m["term_ids"], m["q_off"], [q, q, q])
    lists, places = [], []
    for gap, total in ((1, 0), (300, 700), (1500, 2600)):
        filler = rng.choice(rest, max(total - (k - 1) - 2, len(rest)))  # entries that score below the tied document
        body = rng.permutation(np.concatenate([top, filler]))
        p1 = int(rng.integers(0, len(body) - gap + 1))
        body = np.insert(body, p1, tied)
        body = np.insert(body, p1 + gap, tied)
        lists.append(body)
        places.append((p1, p1 + gap))
    q_cand, cand_doc = lists_csr(lists)
    got, n = assert_topk(m["scorer"], m["dt"], ids, off, k, q_cand, cand_doc, "tie at the k-th place")
    for i, (p1, p2) in enumerate(places):
        assert n[i] == k and got["pos"][i, k - 1] == p1 and got["doc"][i, k - 1] == tied
        assert p2 not in got["pos"][i].tolist()
    # and with one more place both are in, the smaller position first
    got, _ = assert_topk(m["scorer"], m["dt"], ids, off, k + 1, q_cand, cand_doc, "tie inside the row")
    for i, (p1, p2) in enumerate(places):
        assert got["pos"][i, k - 1:k + 1].tolist() == [p1, p2]


def test_queries_without_candidates_between_queries_with_them(rr):
    m = rr
    rng = np.random.default_rng(8)
    lists = [rng.integers(0, m["n_docs"], n) for n in ([0, 0, 5, 0, 300, 0, 0, 1200, 0] + [0] * (m["nq"] - 9))]
    q_cand, cand_doc = lists_csr(lists)
    got, n = assert_topk(m["scorer"], m["dt"], m["term_ids"], m["q_off"], 10, q_cand, cand_doc, "empty lists between")
    assert n[:9].tolist() == [0, 0, 5, 0, 10, 0, 0, 10, 0] and not got[0].tobytes().strip(b"\0") and not got[8].tobytes().strip(b"\0")


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("part", [64, 128, 1000])
def test_parts_cuts_and_grid_turns_give_identical_bytes(rr, tuning, part, grid):
    """the smallest settings with several parts a query, several cuts a part and several grid turns"""
    m = rr
    tuning(rerank_part=part, rerank_buf=2, eval_grid=grid)
    rng = np.random.default_rng(9)
    ids2, off2 = take_queries(m["term_ids"], m["q_off"], [m["rich"], 2])
    q_cand2, cand_doc2 = lists_csr([np.sort(rng.integers(0, m["n_docs"], 5000)), rng.integers(0, m["n_docs"], 3000)])
    # ascending scores: every entry beats the threshold, the buffer is cut again and again
    rising = np.argsort(m["cross"][m["rich"]], kind="stable")
    q_cand3, cand_doc3 = lists_csr([np.concatenate([rising, rising, rising])])
    ids3, off3 = take_queries(m["term_ids"], m["q_off"], [m["rich"]])
    for k in (10, 100):
        assert_topk(m["scorer"], m["dt"], m["term_ids"], m["q_off"], k, m["q_cand"], m["cand_doc"], f"lists part={part} grid={grid}")
        assert_topk(m["scorer"], m["dt"], m["term_ids"], m["q_off"], k, what=f"cross part={part} grid={grid}")
        assert_topk(m["scorer"], m["dt"], ids2, off2, k, q_cand2, cand_doc2, f"5000 entries part={part} grid={grid}")
        assert_topk(m["scorer"], m["dt"], ids3, off3, k, q_cand3, cand_doc3, f"rising scores part={part} grid={grid}")
    got = m["scorer"].evaluate(m["term_ids"], m["q_off"], m["q_cand"], m["cand_doc"])
    vb.reset_tuning()
    assert np.array_equal(bits(got), bits(m["dt"].evaluate(m["term_ids"], m["q_off"], m["q_cand"], m["cand_doc"])))


@pytest.mark.parametrize("k1", [1.2, 2.0])
@pytest.mark.parametrize("b", [0.0, 0.75, 1.0])
def test_fieldnorm_length_and_the_bm25_parameters(k1, b):
    w = ev.World(ev.SMALL, k1, b)
    docs = ev.fieldnorm_docs()
    dt = vb.Documents.cast(docs, None, seed=cm.SEED).bind(w.resolver)
    term_ids, q_off = w.resolve([[ev.SMALL[1]], [ev.SMALL[2], ev.SMALL[1], ev.UNKNOWN[0]], [ev.SMALL[0], ev.SMALL[2]]])
    with dt.scorer() as s:
        assert np.array_equal(bits(s.evaluate(term_ids, q_off)), bits(dt.evaluate(term_ids, q_off)))
        for k in (10, 256, 300):
            got, n = assert_topk(s, dt, term_ids, q_off, k, what=f"k1={k1} b={b}")
            assert (n == min(k, len(docs))).all()
        q_cand, cand_doc = lists_csr([np.arange(len(docs))[::-1], [258, 259, 259, 258], np.arange(0, len(docs), 2)])
        got, _ = assert_topk(s, dt, term_ids, q_off, 4, q_cand, cand_doc, f"lists k1={k1} b={b}")
    # documents 258 and 259 hold the query's lexeme once each and differ in their length only: with b = 0 they tie, the position decides
    if b == 0:
        assert got["pos"][1].tolist() == [0, 1, 2, 3]
    else:
        assert got["score"][1, 0] > got["score"][1, 2]


def test_one_scorer_across_growing_and_shrinking_shapes(rr):
    m = rr
    dt = m["dt"]
    rng = np.random.default_rng(12)
    small = (*take_queries(m["term_ids"], m["q_off"], [7, 8]), *lists_csr([rng.integers(0, m["n_docs"], 20), rng.integers(0, m["n_docs"], 70)]))
    big = (m["term_ids"], m["q_off"], *lists_csr([rng.integers(0, m["n_docs"], 2500 if q % 3 == 0 else 40) for q in range(m["nq"])]))
    with dt.scorer() as s:
        assert s.device_bytes() == 0
        seen = {}
        for name, (ids, off, qc, cd), k in (("small", small, 5), ("big", big, 100), ("small", small, 5), ("big", big, 100), ("small", small, 64),
                                            ("big", big, 100)):
            assert_topk(s, dt, ids, off, k, qc, cd, name)
            assert np.array_equal(bits(s.evaluate(ids, off, qc, cd)), bits(dt.evaluate(ids, off, qc, cd)))
            if name == "big" and "big" in seen:
                assert s.device_bytes() == seen["big"], "a repeat of a shape already seen changed the buffers"
            seen.setdefault(name, s.device_bytes())
        held = s.device_bytes()
        assert held >= seen["small"] > 0 and held == seen["big"]
        assert_topk(s, dt, small[0], small[1], 5, what="cross after lists")  # (cross product: no candidate arrays in the block)
        assert s.device_bytes() == held
        # refused calls leave the scorer as it was
        far = small[3].copy()
        far[3] = m["n_docs"]
        with pytest.raises(vb.Vbm25Error, match=rf"query 0: candidate {m['n_docs']} is outside"):
            s.topk(small[0], small[1], 5, small[2], far)
        with pytest.raises(vb.Vbm25Error, match="k is 1025"):
            s.topk(small[0], small[1], 1025, small[2], small[3])
        with pytest.raises(vb.Vbm25Error, match=rf"query 0: candidate {m['n_docs']} is outside"):
            s.evaluate(small[0], small[1], small[2], far)
        assert_topk(s, dt, *small[:2], 5, *small[2:], "after the refusals")
        assert_topk(s, dt, *big[:2], 100, *big[2:], "after the refusals")
        assert s.device_bytes() == held
        s.close()
        assert s.device_bytes() == 0
        s.close()


def test_two_threads_on_one_scorer_and_two_scorers_at_once(rr):
    m = rr
    dt = m["dt"]
    rng = np.random.default_rng(13)
    half = m["nq"] // 2
    batches = []
    for lo, hi, k in ((0, half, 10), (half, m["nq"], 100)):
        ids, off = take_queries(m["term_ids"], m["q_off"], range(lo, hi))
        qc, cd = lists_csr([rng.integers(0, m["n_docs"], int(n)) for n in rng.integers(0, 1500, hi - lo)])
        batches.append((ids, off, k, qc, cd))
    want = [reference_topk(dt.evaluate(b[0], b[1], b[3], b[4]), b[3], b[4], b[2]) for b in batches]

    def run(scorers):
        out, errors = [None, None], []

        def work(i):
            try:
                for _ in range(4):
                    out[i] = scorers[i].topk(*batches[i])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for i in range(2):
            assert out[i][0].tobytes() == want[i][0].tobytes() and np.array_equal(out[i][1], want[i][1])

    run([m["scorer"], m["scorer"]])  # (serialised by the scorer's mutex)
    with dt.scorer() as other:
        run([m["scorer"], other])


def test_refusals_message_for_message(rr):
    """every refusal of vbm25_evaluate_documents through both new calls with the same text, then k and the result arrays"""
    m = rr
    dt, s, ids, off, qc, cd = m["dt"], m["scorer"], m["term_ids"], m["q_off"], m["q_cand"], m["cand_doc"]
    calls = [lambda *a: s.evaluate(*a), lambda ids, off, qc=None, cd=None: s.topk(ids, off, 10, qc, cd)]

    def refused(match, *args, code=INVALID):
        with pytest.raises(vb.Vbm25Error) as plain:
            dt.evaluate(*args)
        assert plain.value.code == code
        for call in calls:
            with pytest.raises(vb.Vbm25Error, match=match) as e:
                call(*args)
            assert e.value.code == code and str(e.value) == str(plain.value)

    q = 7  # (a query of five ids)
    bad = ids.copy()
    bad[off[q] + 1], bad[off[q] + 2] = ids[off[q] + 2], ids[off[q] + 1]
    refused(rf"query {q}: term ids must be strictly ascending", bad, off, qc, cd)
    dup = ids.copy()
    dup[off[q] + 1] = ids[off[q]]
    refused(rf"query {q}: term ids must be strictly ascending", dup, off)
    far = cd.copy()
    far[int(qc[5]) + 2] = m["n_docs"]
    refused(rf"query 5: candidate {m['n_docs']} is outside the handle's {m['n_docs']} documents", ids, off, qc, far)
    o = off.copy()
    o[0] = 1
    refused(r"q_off\[0\] is 1, not 0", ids, o, qc, cd)
    o = off.copy()
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
    one, rank, cnt = np.zeros(1, np.float64), np.zeros(m["nq"] * 10, vb.RANK_DTYPE), np.zeros(m["nq"], np.uint32)

    def last(code, rc, text):
        assert rc == code and text in L.vbm25_last_error(), (rc, L.vbm25_last_error())

    nq = m["nq"]
    last(INVALID, L.vbm25_scorer_evaluate(s.h, None, off.ctypes.data, nq, None, None, one.ctypes.data), b"NULL argument")
    last(INVALID, L.vbm25_scorer_evaluate(s.h, ids.ctypes.data, off.ctypes.data, nq, None, None, None), b"NULL argument")
    last(INVALID, L.vbm25_scorer_evaluate(None, ids.ctypes.data, off.ctypes.data, nq, None, None, one.ctypes.data), b"NULL argument")
    last(INVALID, L.vbm25_scorer_topk(s.h, None, off.ctypes.data, nq, None, None, 10, rank.ctypes.data, cnt.ctypes.data), b"NULL argument")
    last(INVALID, L.vbm25_scorer_topk(s.h, ids.ctypes.data, off.ctypes.data, nq, None, None, 10, None, cnt.ctypes.data), b"NULL argument")
    last(INVALID, L.vbm25_scorer_topk(s.h, ids.ctypes.data, off.ctypes.data, nq, None, None, 10, rank.ctypes.data, None), b"NULL argument")
    last(INVALID, L.vbm25_scorer_topk(None, ids.ctypes.data, off.ctypes.data, nq, None, None, 10, rank.ctypes.data, cnt.ctypes.data), b"NULL argument")
    # 2^31 pairs or more: counted from the offsets, before any array is looked at
    huge, none = np.array([0, 1 << 31], dtype=np.uint64), np.zeros(2, np.uint32)
    last(UNSUPPORTED, L.vbm25_scorer_evaluate(s.h, none.ctypes.data, none.ctypes.data, 1, huge.ctypes.data, none.ctypes.data, one.ctypes.data),
         b"2147483648 pairs: one call scores fewer than 2^31")
    last(UNSUPPORTED, L.vbm25_scorer_topk(s.h, none.ctypes.data, none.ctypes.data, 1, huge.ctypes.data, none.ctypes.data, 10, rank.ctypes.data,
                                          cnt.ctypes.data), b"2147483648 pairs: one call scores fewer than 2^31")
    # k
    with pytest.raises(vb.Vbm25Error, match="k is 0") as e:
        s.topk(ids, off, 0, qc, cd)
    assert e.value.code == INVALID
    with pytest.raises(vb.Vbm25Error, match="k is 1025: a scorer returns at most 1024 candidates a query") as e:
        s.topk(ids, off, 1025, qc, cd)
    assert e.value.code == UNSUPPORTED
    # a scorer from a NULL handle
    out = C.c_void_p(1)
    last(INVALID, L.vbm25_scorer_create(None, C.byref(out)), b"NULL argument")
    assert not out.value
    last(INVALID, L.vbm25_scorer_create(dt.h, None), b"out is NULL")
    assert L.vbm25_scorer_device_bytes(None) == 0
    L.vbm25_scorer_free(None)
    # nq == 0 and queries without candidates are legal
    assert L.vbm25_scorer_evaluate(s.h, None, None, 0, None, None, None) == 0
    assert L.vbm25_scorer_topk(s.h, None, None, 0, None, None, 10, None, None) == 0
    got, n = s.topk(ids, off, 10, np.zeros(nq + 1, np.uint64), np.zeros(0, np.uint32))
    assert not n.any() and not got.tobytes().strip(b"\0")
    # after the refused calls the scorer gives exact results
    assert_topk(s, dt, ids, off, 10, qc, cd, "after the refusals")


def test_an_index_without_sealed_documents_is_refused(rr):
    gix, keep = ev.empty_index()
    r = vb.Resolver(gix, 1, 4, 16, 256, seed=cm.SEED)
    dt = rr["h"].bind(r)
    r.submit([[ev.KNOWN[0]]])
    term_ids, q_off = r.collect()
    with dt.scorer() as s:
        for call in (lambda: s.evaluate(term_ids, q_off), lambda: s.topk(term_ids, q_off, 3)):
            with pytest.raises(vb.Vbm25Error, match="evaluate on an index without sealed documents") as e:
                call()
            assert e.value.code == INVALID


def test_a_handle_of_no_documents(world):
    dt = vb.Documents.cast([], None, seed=cm.SEED).bind(world.resolver)
    term_ids, q_off = world.resolve([[ev.KNOWN[0]], []])
    with dt.scorer() as s:
        assert s.evaluate(term_ids, q_off).shape == (2, 0)
        got, n = s.topk(term_ids, q_off, 5)
        assert got.shape == (2, 5) and n.tolist() == [0, 0] and not got.tobytes().strip(b"\0")
        got, n = s.topk(term_ids, q_off, 5, np.zeros(3, np.uint64), np.zeros(0, np.uint32))
        assert n.tolist() == [0, 0] and not got.tobytes().strip(b"\0")
        with pytest.raises(vb.Vbm25Error, match="query 0: candidate 0 is outside the handle's 0 documents"):
            s.topk(term_ids, q_off, 5, np.array([0, 1, 1], np.uint64), np.zeros(1, np.uint32))
