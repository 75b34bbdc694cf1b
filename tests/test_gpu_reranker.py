"""The reranker ring on the GPU (csrc/reranker.hip): lexeme queries (or term ids) and candidate lists -- document indices, ctids, or
none -- in, the k best rows out, byte for byte what the parent's route gives: Resolver.submit / collect followed by Scorer.topk.
Both pack paths, the ring at depths 1 .. 3, parts and grid turns, ctids through the payload directory at every directory shape, the
refusals with code and message, threads.  The world is the one of tests/test_gpu_evaluate_documents.py.  -m gpu only."""
import ctypes as C
import threading

import numpy as np
import pytest

import cast_model as cm
import test_gpu_evaluate_documents as ev
import vectorchord_bm25_amd as vb
from test_gpu_rerank import lists_csr
from vectorchord_bm25_amd._lib import check

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
PATH_WAVE, PATH_RADIX = 1, 2
CAPS = dict(max_queries=64, max_lexemes=4096, max_bytes=1 << 18, max_candidates=40000, max_k=1024)


def pack_path(reranker):
    """the pack path of the last accepted submit (vbm25_debug_reranker, not in the header): 0 none, 1 one wave a query, 2 the radix sort"""
    f = vb.lib().vbm25_debug_reranker
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 4
    path = C.c_uint32()
    assert f(reranker.h, None, C.byref(path), None) == 0
    return path.value


def same(got, want, what):
    assert got[0].shape == want[0].shape and got[0].dtype == vb.RANK_DTYPE and got[1].dtype == np.uint32, what
    assert np.array_equal(got[1], want[1]), f"{what}: n_ranks differ at queries {np.flatnonzero(got[1] != want[1])[:8]}"
    if got[0].tobytes() != want[0].tobytes():
        for q in range(len(want[1])):
            if got[0][q].tobytes() != want[0][q].tobytes():
                i = int(np.flatnonzero(got[0][q].view("V16") != want[0][q].view("V16"))[0])
                raise AssertionError(f"{what}: query {q} ({want[1][q]} ranks) differs first at entry {i}: got {got[0][q, i]}, want {want[0][q, i]}")


@pytest.fixture(scope="module")
def world():
    return ev.World(ev.KNOWN)


@pytest.fixture(scope="module")
def rr(world):
    """the documents (with payloads) and queries of the evaluate tests, bound; one scorer (the reference) and one reranker of two slots"""
    docs = ev.scored_docs()
    h = vb.Documents.cast(docs, cm.payloads(len(docs)), seed=cm.SEED)
    dt = h.bind(world.resolver)
    queries = ev.query_batch()
    nq, n_docs = len(queries), len(docs)
    q_cand, cand_doc = ev.candidate_lists(nq, n_docs)
    m = dict(world=world, h=h, dt=dt, scorer=dt.scorer(), queries=queries, nq=nq, n_docs=n_docs, q_cand=q_cand, cand_doc=cand_doc)
    m["reranker"] = dt.reranker(world.resolver, 2, **CAPS)
    m["ids"], m["off"] = world.resolve(queries)
    return m


def reference(m, queries, k, q_cand=None, cand_doc=None):
    """the parent's route: the resolver ring, its ids through the host, the scorer"""
    ids, off = m["world"].resolve(queries)
    return m["scorer"].topk(ids, off, k, q_cand, cand_doc)


def through(reranker, queries, k, q_cand=None, cand_doc=None, cand_tid=None):
    reranker.submit(queries, k, q_cand, cand_doc, cand_tid)
    return reranker.collect()


# ---- 1. lexemes


@pytest.mark.parametrize("k", [1, 10, 64, 65, 1024])
def test_the_main_batch_from_lexemes(rr, k):
    """lists of 0, 1, 63, 64, 65 and all documents (one descending, one with repeats, one shuffled), then the cross product"""
    m = rr
    got = through(m["reranker"], m["queries"], k, m["q_cand"], m["cand_doc"])
    assert pack_path(m["reranker"]) == PATH_RADIX  # (queries of 300 lexemes)
    same(got, reference(m, m["queries"], k, m["q_cand"], m["cand_doc"]), f"lists k={k}")
    sizes = np.diff(m["q_cand"].astype(np.int64))
    assert np.array_equal(got[1], np.minimum(sizes, k)) and {0, 1, 63, 64, 65, m["n_docs"]} <= set(sizes.tolist())
    got = through(m["reranker"], m["queries"], k)
    same(got, reference(m, m["queries"], k), f"cross k={k}")
    assert (got[1] == min(k, m["n_docs"])).all() and np.array_equal(got[0]["pos"], got[0]["doc"])


@pytest.mark.parametrize("longest,path", [(64, PATH_WAVE), (65, PATH_RADIX)])
def test_both_pack_paths(rr, longest, path):
    """a batch whose longest query has exactly 64 lexemes packs one wave a query, one with 65 sorts; queries of 0 lexemes and of only
    unknown lexemes score 0 everywhere: their rows are the first positions"""
    m = rr
    queries = [q for q in m["queries"] if len(q) <= longest]
    lengths = [len(q) for q in queries]
    assert max(lengths) == longest and 0 in lengths
    rng = np.random.default_rng(longest)
    q_cand, cand_doc = lists_csr([rng.integers(0, m["n_docs"], 30 + 7 * i) for i in range(len(queries))])
    for k in (10, 100):
        got = through(m["reranker"], queries, k, q_cand, cand_doc)
        assert pack_path(m["reranker"]) == path
        same(got, reference(m, queries, k, q_cand, cand_doc), f"longest {longest}, k={k}")
    ranks, n = got
    zero = [i for i, q in enumerate(queries) if not q or all(t in ev.UNKNOWN or t in ev.LATER for t in q)]
    assert len(zero) >= 4
    for i in zero:
        assert ranks["pos"][i, :n[i]].tolist() == list(range(n[i])) and not ranks["score"][i].view(np.uint64).any()


# ---- 2. the ring


@pytest.fixture(scope="module")
def ring_batches(rr):
    """batches of different nq, k and list shapes, each with its reference (computed once)"""
    m = rr
    rng = np.random.default_rng(31)
    qs = m["queries"]
    shapes = [(qs[5:14], 10, lists_csr([rng.integers(0, m["n_docs"], n) for n in (0, 1, 63, 64, 65, 300, 1200, 5, 0)])),
              (qs[20:27], 64, None),
              (qs[:33], 3, lists_csr([rng.integers(0, m["n_docs"], int(n)) for n in rng.integers(0, 200, 33)])),
              (qs[1:3], 7, (np.zeros(3, np.uint64), np.zeros(0, np.uint32)))]  # (no query has a candidate: nothing is enqueued)
    out = []
    for queries, k, lists in shapes:
        qc, cd = lists if lists else (None, None)
        out.append((queries, k, qc, cd, reference(m, queries, k, qc, cd)))
    return out


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_the_ring_first_in_first_out(rr, ring_batches, depth):
    m, batches = rr, ring_batches
    with m["dt"].reranker(m["world"].resolver, depth, **CAPS) as r:
        made, held = r.allocations(), r.device_bytes()
        assert made > 0 and held > 0
        for b in batches[:depth]:
            r.submit(*b[:4])
        assert r.in_flight() == depth
        with pytest.raises(vb.Vbm25Error, match=rf"the reranker's {depth} slots are all in flight: collect first") as e:
            r.submit(*batches[3][:4])
        assert e.value.code == INVALID and r.in_flight() == depth
        for i, b in enumerate(batches[:depth]):
            got = r.collect()
            assert got[0].shape == (len(b[0]), b[1])  # (each batch with its own nq and k)
            same(got, b[4], f"depth {depth}, batch {i}")
        with pytest.raises(vb.Vbm25Error, match="nothing is in flight on the reranker") as e:
            r.collect()
        assert e.value.code == INVALID and r.in_flight() == 0
        # a refused submit between two good ones
        r.submit(*batches[0][:4])
        with pytest.raises(vb.Vbm25Error, match="k is 0" if depth > 1 else "slots are all in flight"):  # (a full ring is refused first)
            r.submit(batches[1][0], 0)
        assert r.in_flight() == 1
        if depth == 1:
            same(r.collect(), batches[0][4], "before the refusal")
        r.submit(*batches[3][:4])  # (the batch that enqueues nothing keeps its place)
        if depth > 1:
            same(r.collect(), batches[0][4], "before the refusal")
        same(r.collect(), batches[3][4], "after the refusal")
        assert not batches[3][4][0].tobytes().strip(b"\0") and not batches[3][4][1].any()
        # 20 rounds, the ring kept full
        pending = []
        for i in range(20):
            if len(pending) == depth:
                same(r.collect(), pending.pop(0), f"round {i}")
            b = batches[i % len(batches)]
            r.submit(*b[:4])
            pending.append(b[4])
        while pending:
            same(r.collect(), pending.pop(0), "draining")
        assert r.allocations() == made and r.device_bytes() == held


@pytest.mark.parametrize("depth", [1, 16])
def test_the_ring_wraps_at_the_extreme_depths(rr, depth):
    """2 * depth + 1 batches of two to four queries through a ring of `depth` slots: full, then collect one and submit one until none
    is left, then drained -- the cursor passes its end twice.  Lists, the cross product and a batch that enqueues nothing in turns,
    every batch against Resolver + Scorer.topk"""
    m = rr
    rng = np.random.default_rng(40 + depth)
    qs = m["queries"]
    batches = []
    for i in range(2 * depth + 1):
        nq, k = 2 + i % 3, (10, 3, 7)[i % 3]
        at = int(rng.integers(0, len(qs) - nq))
        if i % 7 == 3:  # (no query has a candidate: the batch keeps its place and collects as zero rows)
            qc, cd = np.zeros(nq + 1, np.uint64), np.zeros(0, np.uint32)
        elif i % 4 == 1:
            qc, cd = None, None
        else:
            qc, cd = lists_csr([rng.integers(0, m["n_docs"], int(n)) for n in rng.integers(0, 80, nq)])
        batches.append((qs[at:at + nq], k, qc, cd))
    want = [reference(m, *b) for b in batches]
    with m["dt"].reranker(m["world"].resolver, depth, max_queries=4, max_lexemes=4096, max_bytes=1 << 18, max_candidates=4096, max_k=10) as r:
        made = (r.allocations(), r.device_bytes())
        got = []
        for i, b in enumerate(batches):
            if r.in_flight() == depth:
                got.append(r.collect())
            r.submit(*b)
            assert r.in_flight() == min(i + 1, depth)
        while r.in_flight():
            got.append(r.collect())
        assert len(got) == len(batches)
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, f"depth {depth}, batch {i}")
        assert (r.allocations(), r.device_bytes()) == made
        with pytest.raises(vb.Vbm25Error, match="nothing is in flight on the reranker"):
            r.collect()


# ---- 3. term ids


def test_submit_ids_against_the_scorer(rr):
    m = rr
    ids, off = [], [0]
    for q in range(m["nq"]):  # ids at and beyond the term count, where a query may hold them: anywhere, they are skipped
        run = m["ids"][m["off"][q]:m["off"][q + 1]].tolist()
        if q % 3 == 0:
            run = run[:1] + [0xFFFFFFFF, 6000] + run[1:] + [6001]
        ids += run
        off.append(len(ids))
    ids, off = np.array(ids, np.uint32), np.array(off, np.uint32)
    r = m["reranker"]
    for k in (10, 65):
        r.submit_ids(ids, off, k, m["q_cand"], m["cand_doc"])
        r.submit_ids(ids, off, k)
        assert pack_path(r) == 0
        same(r.collect(), m["scorer"].topk(ids, off, k, m["q_cand"], m["cand_doc"]), f"ids, lists k={k}")
        same(r.collect(), m["scorer"].topk(ids, off, k), f"ids, cross k={k}")
    same(m["scorer"].topk(ids, off, 10), m["scorer"].topk(m["ids"], m["off"], 10), "the ids beyond the vocabulary score nothing")


# ---- 4. parts and grid turns


@pytest.mark.parametrize("grid", [1, 3])
def test_parts_and_grid_turns_give_identical_bytes(rr, tuning, grid):
    m = rr
    rng = np.random.default_rng(9)
    queries = [m["queries"][q] for q in (7, 31, 35, 2)]
    q_cand, cand_doc = lists_csr([rng.integers(0, m["n_docs"], n) for n in (65, 129, 5000, 5000)])
    want = {k: reference(m, queries, k, q_cand, cand_doc) for k in (10, 100)}
    cross = reference(m, m["queries"], 10)
    tuning(rerank_part=64, eval_grid=grid)
    with m["dt"].reranker(m["world"].resolver, 2, **CAPS) as r:
        for k in (10, 100):
            same(through(r, queries, k, q_cand, cand_doc), want[k], f"part 64, grid {grid}, k={k}")
        same(through(r, m["queries"], 10), cross, f"cross, part 64, grid {grid}")


# ---- 5. ctids


EXTREMES = np.array([[0, 0, 0], [0xFFFF, 0xFFFF, 0xFFFF]], dtype=np.uint16)
HANDLES = [1, 3, 4, 5, 63, 64, 65, 129, 5000]
WITH_EXTREMES = {4, 64, 129, 5000}


def ctid_world(n):
    """n documents with distinct payloads drawn from fields 1 .. 0xFFFE; documents n - 1 and 0 share one (n >= 2); some handles hold
    the two extreme keys"""
    rng = np.random.default_rng(1000 + n)
    pay = np.zeros((0, 3), np.uint16)
    while len(pay) < n:
        pay = np.unique(np.concatenate([pay, rng.integers(1, 0xFFFF, (n, 3)).astype(np.uint16)]), axis=0)
    pay = rng.permutation(pay)[:n]
    if n in WITH_EXTREMES:
        pay[1], pay[2] = EXTREMES
    if n >= 2:
        pay[n - 1] = pay[0]
    pool = [ev.KNOWN[i] for i in range(46)]
    return cm.corpus(pool, n, seed=11), np.ascontiguousarray(pay)


def ctid_lists(pay, rng):
    """lists of 0, 1, 63, 64, 65 and 257 ctids: absent ones first, last, interleaved and alone, repeats, the shared payload, the extremes"""
    n = len(pay)

    def present(k):
        return pay[rng.integers(0, n, k)]

    def absent(k):  # (field 0 is 0 or 0xFFFF only in the extremes, which every field of the drawn payloads avoids)
        a = rng.integers(1, 0xFFFF, (k, 3)).astype(np.uint16)
        a[:, 0] = 0
        a[:, 2] |= 1
        return a

    mixed = np.concatenate([present(120), absent(60), np.repeat(present(5), 6, axis=0), pay[:1], pay[n - 1:], EXTREMES, EXTREMES,
                            present(257)])[:257]
    inter = np.empty((65, 3), np.uint16)
    inter[0::2], inter[1::2] = present(33), absent(32)
    lists = [np.zeros((0, 3), np.uint16), present(1), np.concatenate([absent(5), present(58)]), np.concatenate([present(60), absent(4)]),
             inter, rng.permutation(mixed), absent(3), absent(1), EXTREMES]
    q_cand = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    return q_cand, np.ascontiguousarray(np.concatenate(lists))


def expect_from_ctids(scorer, ids, off, k, q_cand, cand_tid, pay):
    """on the host: each ctid to the lowest document with that payload, the misses dropped, Scorer.topk on the kept entries, pos mapped
    back through the kept entries' original positions"""
    first = {}
    for d, key in enumerate(vb.TidSet.keys(pay).tolist()):
        first.setdefault(key, d)
    keys = vb.TidSet.keys(cand_tid).tolist()
    kept_docs, kept_pos = [], []
    for q in range(len(q_cand) - 1):
        lo, hi = int(q_cand[q]), int(q_cand[q + 1])
        at = [i for i in range(lo, hi) if keys[i] in first]
        kept_docs.append(np.array([first[keys[i]] for i in at], np.uint32))
        kept_pos.append(np.array([i - lo for i in at], np.uint32))
    qc, cd = lists_csr(kept_docs)
    ranks, n = scorer.topk(ids, off, k, qc, cd)
    for q in range(len(n)):
        ranks["pos"][q, :n[q]] = kept_pos[q][ranks["pos"][q, :n[q]]]
    return ranks, n, [len(p) for p in kept_pos]


@pytest.mark.parametrize("n", HANDLES)
def test_candidates_as_ctids(rr, tuning, n):
    """handles of 1 .. 5000 documents under tid_dir 0 (one entry), 2 (four entries: stride 1 up to 4 documents, then runs, the last one
    shorter) and the default; then eval_grid 1, where the lookup strides its grid"""
    m = rr
    docs, pay = ctid_world(n)
    h = vb.Documents.cast(docs, pay, seed=cm.SEED)
    dt = h.bind(m["world"].resolver)
    q_cand, cand_tid = ctid_lists(pay, np.random.default_rng(n))
    queries = [m["queries"][q] for q in (7, 1, 8, 13, 27, 35, 9, 10, 5)]
    ids, off = m["world"].resolve(queries)
    with dt.scorer() as scorer:
        want = {k: expect_from_ctids(scorer, ids, off, k, q_cand, cand_tid, pay) for k in (10, 300)}
    kept = want[10][2]
    assert kept[0] == 0 and kept[1] == 1 and kept[2] == 58 and kept[3] == 60 and kept[4] == 33 and kept[6] == 0 and kept[7] == 0
    assert kept[8] == (2 if n in WITH_EXTREMES else 0)
    for tid_dir, grid in ((0, None), (2, None), (None, None), (None, 1)):
        vb.reset_tuning()
        if tid_dir is not None:
            tuning(tid_dir=tid_dir)
        if grid is not None:
            tuning(eval_grid=grid)
        with dt.reranker(m["world"].resolver, 2, documents=h, **CAPS) as r:
            for k in (10, 300):
                got = through(r, queries, k, q_cand, cand_tid=cand_tid)
                same(got, want[k][:2], f"{n} documents, tid_dir {tid_dir}, grid {grid}, k={k}")
            assert got[1].tolist() == kept  # (k = 300 is beyond every list: the eligible entries, counted)
            for q in (0, 6, 7):  # no ctid, or only absent ones: every row zero
                assert not got[0][q].tobytes().strip(b"\0")
            r.submit_ids(ids, off, 10, q_cand, cand_tid=cand_tid)
            same(r.collect(), want[10][:2], f"{n} documents, ids and ctids")


# ---- 6. refusals


def last_error():
    return vb.lib().vbm25_last_error().decode()


def test_create_refusals(rr):
    m = rr
    L, dt, rs = vb.lib(), m["dt"], m["world"].resolver
    caps = [2, 64, 4096, 1 << 18, 40000, 1024]

    def create(t, r, p, *c, out=True):
        h = C.c_void_p(1)
        rc = L.vbm25_reranker_create(t, r, p, *c, C.byref(h) if out else None)
        assert not out or not h.value
        return rc, last_error()

    assert create(dt.h, rs.h, None, *caps, out=False) == (INVALID, "out is NULL")
    assert create(None, rs.h, None, *caps) == (INVALID, "NULL argument")
    assert create(dt.h, None, None, *caps) == (INVALID, "NULL argument")
    for depth in (0, 17):
        assert create(dt.h, rs.h, None, depth, *caps[1:]) == (INVALID, f"depth {depth} is outside 1 .. 16")
    for i in (1, 2, 4, 5):
        c = list(caps)
        c[i] = 0
        assert create(dt.h, rs.h, None, *c) == (INVALID, "max_queries, max_lexemes, max_candidates or max_k is 0")
    with pytest.raises(vb.Vbm25Error) as scorer_says:
        m["scorer"].topk(m["ids"], m["off"], 1025)
    rc, text = create(dt.h, rs.h, None, *caps[:5], 1025)
    assert rc == UNSUPPORTED == scorer_says.value.code and text == "k is 1025: a scorer returns at most 1024 candidates a query"
    assert str(scorer_says.value).endswith(text)
    plain = vb.Documents.cast(ev.scored_docs(), None, seed=cm.SEED)
    assert create(dt.h, rs.h, plain.h, *caps) == (INVALID, "the documents given for the ctid lookup carry no payloads")
    fewer = vb.Documents.cast(ev.scored_docs()[:10], cm.payloads(10), seed=cm.SEED)
    assert create(dt.h, rs.h, fewer.h, *caps) == (INVALID, f"the documents given for the ctid lookup are 10, the bound documents {m['n_docs']}")
    other = ev.World(ev.KNOWN[:100])
    assert create(dt.h, other.resolver.h, None, *caps) == (INVALID, "the documents are bound to another index than the resolver's")
    # an index without sealed documents: vbm25_evaluate_documents' words
    gix, keep = ev.empty_index()
    r0 = vb.Resolver(gix, 1, 4, 16, 256, seed=cm.SEED)
    dt0 = m["h"].bind(r0)
    with pytest.raises(vb.Vbm25Error) as plain_says:
        dt0.evaluate(np.zeros(1, np.uint32), np.array([0, 0], np.uint32))
    rc, text = create(dt0.h, r0.h, None, *caps)
    assert rc == INVALID == plain_says.value.code and text == "evaluate on an index without sealed documents" and str(plain_says.value).endswith(text)
    assert L.vbm25_reranker_device_bytes(None) == 0 and L.vbm25_reranker_in_flight(None) == 0
    L.vbm25_reranker_free(None)
    assert L.vbm25_reranker_info(None, None, None, None, None) == INVALID
    depth, n_docs, has, made = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    assert L.vbm25_reranker_info(m["reranker"].h, C.byref(depth), C.byref(n_docs), C.byref(has), C.byref(made)) == 0
    assert (depth.value, n_docs.value, has.value) == (2, m["n_docs"], 0) and made.value == m["reranker"].allocations()


def test_submit_and_collect_refusals(rr, tuning):
    m = rr
    L, s, world = vb.lib(), m["scorer"], m["world"]
    queries = m["queries"][5:12]
    data, lex_off, q_lex = vb.pack_lexemes(queries)
    nq = len(queries)
    ids, off = world.resolve(queries)
    qc, cd = lists_csr([np.arange(20 + q) for q in range(nq)])
    tids = np.zeros((int(qc[nq]), 3), np.uint16)
    want = s.topk(ids, off, 10, qc, cd)
    r = m["reranker"]

    def p(a):
        return None if a is None else a.ctypes.data

    def lex(data=data, lex_off=lex_off, q_lex=q_lex, nq=nq, qc=qc, cd=cd, ct=None, k=10, h=None):
        return L.vbm25_reranker_submit_lexemes(h or r.h, p(data), p(lex_off), p(q_lex), nq, p(qc), p(cd), p(ct), k)

    def by_ids(ids=ids, off=off, nq=nq, qc=qc, cd=cd, ct=None, k=10, h=None):
        return L.vbm25_reranker_submit_ids(h or r.h, p(ids), p(off), nq, p(qc), p(cd), p(ct), k)

    def got(rc):
        return rc, last_error()

    def refused(mine, expect, text=None, handle=r):
        """`mine`: (code, message) of the reranker's call, taken before the old call ran; `expect`: the old call's, or the pair itself"""
        assert mine == expect and (text is None or mine[1] == text), (mine, expect, text)
        assert handle.in_flight() == 0

    def old(call, *args):
        """the same bad input through the old call: its code and message"""
        with pytest.raises(vb.Vbm25Error) as e:
            call(*args)
        return e.value.code, str(e.value).split(": ", 1)[1]

    assert L.vbm25_reranker_submit_lexemes(None, p(data), p(lex_off), p(q_lex), nq, None, None, None, 10) == INVALID and last_error() == "NULL argument"
    assert L.vbm25_reranker_submit_ids(None, p(ids), p(off), nq, None, None, None, 10) == INVALID and last_error() == "NULL argument"
    refused(got(lex(ct=tids)), (INVALID, "cand_doc and cand_tid are both given: a batch's candidates come one way"))
    refused(got(lex(qc=None)), (INVALID, "cand_doc is given without q_cand"))
    refused(got(by_ids(qc=None, cd=None, ct=tids)), (INVALID, "cand_tid is given without q_cand"))
    refused(got(lex(cd=None, ct=tids)), (INVALID, "cand_tid on a reranker created without payloads"))
    # the lexeme arrays: the resolver's checks and messages
    refused(got(lex(q_lex=None)), (INVALID, "NULL argument"))
    refused(got(lex(lex_off=None)), (INVALID, "NULL argument"))
    refused(got(lex(data=None)), (INVALID, "NULL argument"))
    bad = q_lex.copy()
    bad[0] = 1
    refused(got(lex(q_lex=bad)), old(world.resolver.submit, (data, lex_off, bad)), "q_lex[0] is 1, not 0")
    bad = q_lex.copy()
    bad[3] = bad[2] - 1
    refused(got(lex(q_lex=bad)), old(world.resolver.submit, (data, lex_off, bad)), "q_lex is not monotone at query 2")
    bad = lex_off.copy()
    bad[4] = bad[3] - 1
    refused(got(lex(lex_off=bad)), old(world.resolver.submit, (data, bad, q_lex)), "lex_off is not monotone at lexeme 3")
    # the ids and the candidates: the scorer's checks and messages
    refused(got(by_ids(ids=None)), old(lambda: check(L.vbm25_scorer_topk(s.h, None, p(off), nq, p(qc), p(cd), 10, p(want[0]), p(want[1])))), "NULL argument")
    q = 2  # (a query of five ids)
    bad = ids.copy()
    bad[off[q]], bad[off[q] + 1] = ids[off[q] + 1], ids[off[q]]
    refused(got(by_ids(ids=bad)), old(s.topk, bad, off, 10, qc, cd), f"query {q}: term ids must be strictly ascending")
    bad = off.copy()
    bad[0] = 1
    refused(got(by_ids(off=bad)), old(s.topk, ids, bad, 10, qc, cd))
    bad = off.copy()
    bad[4] = bad[3] - 1
    refused(got(by_ids(off=bad)), old(s.topk, ids, bad, 10, qc, cd), "q_off is not monotone at query 3")
    for call in (lex, by_ids):
        bad = qc.copy()
        bad[0] = 2
        refused(got(call(qc=bad)), old(s.topk, ids, off, 10, bad, cd), "q_cand[0] is 2, not 0")
        bad = qc.copy()
        bad[3] = bad[2] - 1
        refused(got(call(qc=bad)), old(s.topk, ids, off, 10, bad, cd), "q_cand is not monotone at query 2")
        refused(got(call(cd=None)), old(s.topk, ids, off, 10, qc, None), "cand_doc is NULL while q_cand is not")
        bad = cd.copy()
        bad[int(qc[5]) + 2] = m["n_docs"]
        refused(got(call(cd=bad)), old(s.topk, ids, off, 10, qc, bad), f"query 5: candidate {m['n_docs']} is outside the handle's {m['n_docs']} documents")
        refused(got(call(k=0)), old(s.topk, ids, off, 0, qc, cd), "k is 0")
    # the capacities, each named
    with m["dt"].reranker(world.resolver, 1, 4, 16, 1024, 6000, 8) as small:
        refused(got(lex(h=small.h)), (INVALID, f"{nq} queries exceed the reranker's max_queries 4"), handle=small)
        refused(got(by_ids(h=small.h)), (INVALID, f"{nq} queries exceed the reranker's max_queries 4"), handle=small)
        d4, o4, l4 = vb.pack_lexemes(queries[:4])
        i4, f4 = world.resolve(queries[:4])
        c4 = lists_csr([np.arange(5)] * 4)
        refused(got(lex(data=d4, lex_off=o4, q_lex=l4, nq=4, qc=c4[0], cd=c4[1], h=small.h)), (INVALID, f"{l4[4]} lexemes exceed the reranker's max_lexemes 16"), handle=small)
        refused(got(by_ids(ids=i4, off=f4, nq=4, qc=c4[0], cd=c4[1], h=small.h)), (INVALID, f"{f4[4]} term ids exceed the reranker's max_lexemes 16"), handle=small)
        d2, o2, l2 = vb.pack_lexemes([[b"x" * 300] * 4, []])
        c2 = lists_csr([np.arange(5)] * 2)
        refused(got(lex(data=d2, lex_off=o2, q_lex=l2, nq=2, qc=c2[0], cd=c2[1], h=small.h)), (INVALID, "1200 bytes exceed the reranker's max_bytes 1024"), handle=small)
        d1, o1, l1 = vb.pack_lexemes([queries[0]])
        refused(got(lex(data=d1, lex_off=o1, q_lex=l1, nq=1, qc=None, cd=None, k=9, h=small.h)), (INVALID, "k 9 exceeds the reranker's max_k 8"), handle=small)
        far = lists_csr([np.zeros(6001, np.uint32)])
        refused(got(lex(data=d1, lex_off=o1, q_lex=l1, nq=1, qc=far[0], cd=far[1], k=8, h=small.h)), (INVALID, "6001 candidates exceed the reranker's max_candidates 6000"), handle=small)
        c3 = lists_csr([np.arange(200) % m["n_docs"]] * 3)
        # rerank_part lowered after create: a list of 5000 needs 79 part lists, the slot has room for 9
        long_list = lists_csr([np.arange(5000) % m["n_docs"]])
        small.submit([queries[0]], 8, *long_list)
        before = small.collect()
        tuning(rerank_part=64)
        refused(got(lex(data=d1, lex_off=o1, q_lex=l1, nq=1, qc=long_list[0], cd=long_list[1], k=8, h=small.h)), (INVALID, "the batch needs 79 part lists, a slot of the reranker holds 9: rerank_part was lowered after create"), handle=small)
        vb.reset_tuning()
        small.submit([queries[0]], 8, *long_list)
        same(small.collect(), before, "after the part-list refusal")
        same(before, s.topk(*world.resolve([queries[0]]), 8, *long_list), "the long list")
        small.submit(queries[:3], 8, *c3)
        same(small.collect(), s.topk(*world.resolve(queries[:3]), 8, *c3), "the small reranker after its refusals")
    # collect
    ranks, n = np.zeros((nq, 10), vb.RANK_DTYPE), np.zeros(nq, np.uint32)
    got_nq, got_k = C.c_uint32(), C.c_uint32()
    assert L.vbm25_reranker_collect(None, p(ranks), p(n), C.byref(got_nq), C.byref(got_k)) == INVALID and last_error() == "NULL argument"
    assert L.vbm25_reranker_collect(r.h, p(ranks), p(n), C.byref(got_nq), C.byref(got_k)) == INVALID
    assert last_error() == "nothing is in flight on the reranker"
    assert lex() == 0 and r.in_flight() == 1
    assert L.vbm25_reranker_collect(r.h, p(ranks), p(n), None, C.byref(got_k)) == INVALID and last_error() == "NULL argument"
    assert L.vbm25_reranker_collect(r.h, None, p(n), C.byref(got_nq), C.byref(got_k)) == INVALID and last_error() == "NULL argument"
    assert r.in_flight() == 1  # (a refused collect leaves the batch in the ring)
    assert L.vbm25_reranker_collect(r.h, p(ranks), p(n), C.byref(got_nq), C.byref(got_k)) == 0 and (got_nq.value, got_k.value) == (nq, 10)
    same((ranks, n), want, "after every refusal")
    same(through(r, queries, 10, qc, cd), want, "the next good batch")


def test_two_to_the_31_pairs_are_unsupported(rr):
    """max_candidates above 2^31, so that the pair check fires and not the capacity check; validation is on the host, the arrays
    behind the offsets are never looked at"""
    m = rr
    L = vb.lib()
    huge, none = np.array([0, 1 << 31], dtype=np.uint64), np.zeros(2, np.uint32)
    ranks, n = np.zeros(1, vb.RANK_DTYPE), np.zeros(1, np.uint32)
    assert L.vbm25_scorer_topk(m["scorer"].h, none.ctypes.data, none.ctypes.data, 1, huge.ctypes.data, none.ctypes.data, 1, ranks.ctypes.data,
                               n.ctypes.data) == UNSUPPORTED
    scorer_says = last_error()
    assert scorer_says == "2147483648 pairs: one call scores fewer than 2^31"
    with m["dt"].reranker(m["world"].resolver, 1, 1, 1, 64, (1 << 31) + 1024, 1) as r:
        made = r.allocations()
        assert L.vbm25_reranker_submit_ids(r.h, none.ctypes.data, none.ctypes.data, 1, huge.ctypes.data, none.ctypes.data, None, 1) == UNSUPPORTED
        assert last_error() == scorer_says
        data, lex_off, q_lex = vb.pack_lexemes([[]])
        assert L.vbm25_reranker_submit_lexemes(r.h, None, lex_off.ctypes.data, q_lex.ctypes.data, 1, huge.ctypes.data, none.ctypes.data, None,
                                               1) == UNSUPPORTED
        assert last_error() == scorer_says and r.in_flight() == 0
        same(through(r, [m["queries"][1]], 1), reference(m, [m["queries"][1]], 1), "after the refusal")
        assert r.allocations() == made


# ---- 7. concurrency


def test_a_reranker_beside_a_scorer_and_a_stream_and_two_rerankers(rr):
    m = rr
    world, dt = m["world"], m["dt"]
    rng = np.random.default_rng(13)
    qc, cd = lists_csr([rng.integers(0, m["n_docs"], int(n)) for n in rng.integers(0, 1500, m["nq"])])
    want = reference(m, m["queries"], 10, qc, cd)
    want_cross = reference(m, m["queries"], 100)
    short = [q for q in range(m["nq"]) if 0 < m["off"][q + 1] - m["off"][q] <= 8]
    s_ids = np.concatenate([m["ids"][m["off"][q]:m["off"][q + 1]] for q in short]).astype(np.uint32)
    s_off = np.concatenate([[0], np.cumsum([m["off"][q + 1] - m["off"][q] for q in short])]).astype(np.uint32)
    want_hits = vb.search_batch(world.gix, s_ids, s_off, 10)
    stream = vb.Stream(world.gix, 2, len(short), len(s_ids), 10)
    out, errors = {}, []

    def guarded(name, fn):
        def run():
            try:
                out[name] = fn()
            except Exception as e:  # noqa: BLE001
                errors.append((name, e))
        return threading.Thread(target=run)

    def search():
        stream.submit(s_ids, s_off)
        return m["scorer"].topk(m["ids"], m["off"], 100), stream.collect()

    with dt.reranker(world.resolver, 2, **CAPS) as other:
        for pair in ((guarded("ring", lambda: through(m["reranker"], m["queries"], 10, qc, cd)), guarded("old", search)),
                     (guarded("ring", lambda: through(m["reranker"], m["queries"], 10, qc, cd)),
                      guarded("ring2", lambda: through(other, m["queries"], 100)))):
            for t in pair:
                t.start()
            for t in pair:
                t.join()
            assert not errors, errors
            same(out["ring"], want, "the reranker beside another handle")
    same(out["old"][0], want_cross, "the scorer beside the reranker")
    cm.same_records(out["old"][1], want_hits, "the stream beside the reranker")
    same(out["ring2"], want_cross, "the second reranker")
