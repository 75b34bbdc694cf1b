"""The query resolver on the GPU (csrc/resolve.hip): intern_batch byte for byte against vb.intern, Resolver.collect array for array
against Query.from_tokens + lookup_terms + drop on the host, through the lexeme and the keys entry and through both paths of the
per-query step (the wave path: every query <= 64 lexemes; the general path: one longer query in the batch), the ring's order and
refusals, and lexemes -> hits end to end."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = bytes((7 * i + 3) % 256 for i in range(32))
MISS = 0xFFFFFFFF

_INTERN = {}


def host_intern(lex, seed=SEED):
    k = (lex, seed)
    if k not in _INTERN:
        _INTERN[k] = vb.intern(lex, seed)
    return _INTERN[k]


def vocab_lexeme(i):
    """the vocabulary's lexemes: short ones (the padded path), long ones (the hash) and short ones with a NUL (the hash)"""
    return (b"w%d" % i, b"a-long-lexeme-number-%d" % i, b"n\0%d" % i)[i % 3]


_INDEX = {}


def index_of(n_terms):
    """an index whose vocabulary is the keys of vocab_lexeme(0 .. n_terms): one posting a term -> (GpuIndex, sorted keys as bytes)"""
    if n_terms == 0 and 0 not in _INDEX:  # the empty sealed segment (an index over an empty table)
        arrays = {k: np.zeros(0, dtype=dt) for k, dt in vb.api._DESC_ARRAYS}
        arrays["term_first_block"] = np.zeros(1, dtype=np.uint32)
        arrays["blk_off8"] = np.zeros(1, dtype=np.uint32)
        desc, keep = vb.api.desc_from_arrays(dict(n_docs=0, n_terms=0, n_blocks=0, sum_len=0, k1=1.2, b=0.75), arrays)
        _INDEX[0] = (vb.GpuIndex(desc), [], keep)
    if n_terms not in _INDEX:
        keys = sorted(host_intern(vocab_lexeme(i)) for i in range(n_terms))
        n_docs = min(n_terms, 500)   # (no terms: the empty sealed segment)
        post_doc = (np.arange(n_terms) % max(n_docs, 1)).astype(np.uint32)
        doc_len = np.bincount(post_doc, minlength=n_docs).astype(np.uint32)
        seg = vb.Segment.build(1.2, 0.75, doc_len, np.zeros((n_docs, 3), np.uint16),
                               np.frombuffer(b"".join(keys), dtype=np.uint8), np.arange(n_terms + 1, dtype=np.uint64), post_doc,
                               np.ones(n_terms, np.uint32))
        _INDEX[n_terms] = (vb.GpuIndex(seg), keys)
    return _INDEX[n_terms][:2]


def expected(gix, queries, seed=SEED, interned=False):
    """Query.from_tokens + lookup_terms + drop, per query -> (term_ids, q_off); interned: the queries hold 16-byte keys, not lexemes"""
    ids, off = [], [0]
    for q in queries:
        keys = sorted({bytes(t) if interned else host_intern(t, seed) for t in q})
        assert vb.Query(keys).keys == keys
        got = gix.lookup_terms(keys)
        got = got[got != MISS]
        assert (np.diff(got.astype(np.int64)) > 0).all()  # (ascending keys of an ascending vocabulary: ascending ids)
        ids.append(got)
        off.append(off[-1] + len(got))
    return np.concatenate(ids).astype(np.uint32) if ids else np.zeros(0, np.uint32), np.array(off, dtype=np.uint32)


def keys_of(queries, seed=SEED):
    flat = [host_intern(t, seed) for q in queries for t in q]
    q_key = np.cumsum([0] + [len(q) for q in queries]).astype(np.uint32)
    return np.frombuffer(b"".join(flat), dtype=np.uint8) if flat else np.zeros(0, np.uint8), q_key


def resolve_both(gix, queries, depth=1, seed=SEED):
    """the batch through the lexeme entry and through the keys entry; asserts the two agree byte for byte"""
    n_lex = sum(len(q) for q in queries)
    r = vb.Resolver(gix, depth, max(1, len(queries)), max(1, n_lex), sum(len(t) for q in queries for t in q), seed=seed)
    r.submit(queries)
    ids, off = r.collect()
    r.submit_keys(*keys_of(queries, seed))
    ids_k, off_k = r.collect()
    assert ids.tobytes() == ids_k.tobytes() and off.tobytes() == off_k.tobytes()
    assert r.in_flight == 0 and r.device_bytes >= 16 * gix.n_terms
    return ids, off


def query_mix(n_terms, rng):
    """queries of 0, 1, 5, 63 and 64 lexemes, known and unknown, with duplicates, every lexeme unknown, descending key order, hashed and
    short mixed -- every one at most 64 lexemes"""
    def known(n):
        return [vocab_lexeme(int(i)) for i in rng.integers(0, max(n_terms, 1), n)] if n_terms else [b"w%d" % i for i in range(n)]

    def unknown(n):
        return [(b"zz%d" % i, b"an-unknown-long-lexeme-%d" % i)[i % 2] for i in rng.integers(0, 10**6, n)]

    qs = [[], known(1), unknown(1), known(5), known(3) + unknown(2), known(63), known(64), known(40) + unknown(24)]
    dup = known(7)
    qs.append(dup + dup[::-1] + dup[:3])                                    # duplicates
    qs.append(unknown(9))                                                    # every lexeme unknown
    d = known(30) + unknown(5)
    qs.append(sorted(set(d), key=lambda t: host_intern(t), reverse=True))    # descending key order
    qs.append([vocab_lexeme(i) for i in range(min(n_terms, 12))] + [b"short", b"exactly-16-bytes", b"x" * 15, b"", b"nul\0in"])
    qs.append([])
    return qs


# ---------------------------------------------------------------- intern

def edge_lexemes():
    """the CPU harness's list: every length 0 .. 130 and the chunk / tree edges at every start alignment 0 .. 15 of the pool (a filler
    lexeme in front sets the alignment and is checked too), NULs at the first, a middle and the last byte, a hash with byte 15 == 0"""
    out, pos = [], 0

    def put(lex, align):
        nonlocal pos
        fill = (align - pos) % 16
        out.append(b"f" * fill)
        out.append(lex)
        pos += fill + len(lex)

    lens = list(range(131)) + [1023, 1024, 1025, 2046, 2047, 2048, 2049, 3072, 3073, 4096, 4097, 8192, 8193]
    for n in lens:
        for align in range(16):
            put(bytes((i % 251) for i in range(n)) if align % 2 else bytes(1 + (i * 7 + n) % 255 for i in range(n)), align)
    for n in (1, 2, 3, 8, 15, 16, 17, 64, 65, 1024, 1025):
        for at in {0, n // 2, n - 1}:
            put(b"a" * at + b"\0" + b"a" * (n - at - 1), (3 * n + at) % 16)
    L = C.CDLL(vb.library_path())
    h = (C.c_uint8 * 32)()
    for i in range(100000):
        lex = b"byte15-is-zero-%d" % i
        assert L.vbm25_blake3(SEED, lex, C.c_size_t(len(lex)), h) == 0
        if h[15] == 0:
            put(lex, 5)
            assert host_intern(lex)[15] == 1
            break
    else:
        raise AssertionError("no lexeme with hash byte 15 == 0")
    return out


def test_intern_batch_edge_list_equals_host_intern():
    lex = edge_lexemes()
    got = vb.intern_batch(lex, SEED)
    want = np.frombuffer(b"".join(vb.intern(t, SEED) for t in lex), dtype=np.uint8).reshape(-1, 16)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(int(i), len(lex[i])) for i in bad[:10]]


def test_intern_batch_70000_random_lexemes():
    """more than one pass of the kernel's grid (1024 blocks x 64 lanes)"""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 40, 70_000)
    raw = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    raw[rng.random(len(raw)) < 0.9] |= 1  # (few NULs: most short lexemes take the padded path)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    got = vb.intern_batch((raw, off), SEED)
    data = raw.tobytes()
    want = np.frombuffer(b"".join(vb.intern(data[int(off[i]):int(off[i + 1])], SEED) for i in range(len(lens))), dtype=np.uint8).reshape(-1, 16)
    assert np.array_equal(got, want)


def test_intern_batch_without_seed():
    lex = [b"", b"a", b"0123456789abcde", b"w1"]
    got = vb.intern_batch(lex, None)
    assert got.tobytes() == b"".join(vb.intern(t) for t in lex)
    with pytest.raises(vb.Vbm25Error, match="needs the index's seed") as e:
        vb.intern_batch(lex + [b"0123456789abcdef"], None)
    assert e.value.code == -1
    assert vb.intern_batch([], None).shape == (0, 16)


# ---------------------------------------------------------------- resolver identity

@pytest.mark.parametrize("n_terms", [0, 1, 2, 1000, 200_000])
def test_resolver_equals_host_query_step_on_both_paths(n_terms):
    gix, keys = index_of(n_terms)
    rng = np.random.default_rng(n_terms + 1)
    qs = query_mix(n_terms, rng)
    assert max(len(q) for q in qs) == 64
    want_ids, want_off = expected(gix, qs)
    ids, off = resolve_both(gix, qs)                      # the wave path
    assert np.array_equal(off, want_off) and np.array_equal(ids, want_ids)
    if n_terms >= 1000:
        assert off[-1] > 100  # (the batch finds something)
    # one 65-lexeme query added: the general path, the shared queries' output identical
    q65 = [vocab_lexeme(int(i)) for i in rng.integers(0, max(n_terms, 1), 60)] + [b"unknown-%d" % i for i in range(5)]
    qs2 = qs + [q65]
    want_ids2, want_off2 = expected(gix, qs2)
    ids2, off2 = resolve_both(gix, qs2)
    assert np.array_equal(off2, want_off2) and np.array_equal(ids2, want_ids2)
    assert off2[:len(off)].tobytes() == off.tobytes() and ids2[:len(ids)].tobytes() == ids.tobytes()
    # a query of 3000 lexemes between short ones
    q3000 = [vocab_lexeme(int(i)) for i in rng.integers(0, max(n_terms, 1) + 50, 3000)]
    qs3 = [qs[3], q3000, [], qs[5]]
    want_ids3, want_off3 = expected(gix, qs3)
    ids3, off3 = resolve_both(gix, qs3)
    assert np.array_equal(off3, want_off3) and np.array_equal(ids3, want_ids3)


def test_resolver_empty_batches_and_capacity():
    gix, keys = index_of(1000)
    r = vb.Resolver(gix, 2, 7, 64, 1024, seed=SEED)
    r.submit([])                         # nq = 0
    r.submit([[], [], []])               # only empty queries
    for want_nq in (0, 3):
        ids, off = r.collect()
        assert len(ids) == 0 and off.tolist() == [0] * (want_nq + 1)
    r.submit_keys(np.zeros(0, np.uint8), np.zeros(1, np.uint32))
    ids, off = r.collect()
    assert len(ids) == 0 and off.tolist() == [0]
    qs = [[vocab_lexeme(i), vocab_lexeme(i + 1), b"nope"] for i in range(7)]  # nq = max_queries
    r.submit(qs)
    ids, off = r.collect()
    want_ids, want_off = expected(gix, qs)
    assert np.array_equal(ids, want_ids) and np.array_equal(off, want_off) and off[-1] == 14
    with pytest.raises(vb.Vbm25Error, match="max_queries"):
        r.submit(qs + [[]])
    assert r.in_flight == 0


# ---------------------------------------------------------------- ring

def batch_for(i, n_terms=1000):
    rng = np.random.default_rng(1000 + i)
    nq = 1 + i % 5
    return [[vocab_lexeme(int(t)) for t in rng.integers(0, n_terms + 30, int(rng.integers(0, 9)))] for _ in range(nq)]


@pytest.mark.parametrize("depth", [1, 3])
def test_ring_order_full_and_empty(depth):
    gix, keys = index_of(1000)
    r = vb.Resolver(gix, depth, 8, 256, 8192, seed=SEED)
    with pytest.raises(vb.Vbm25Error, match="nothing is in flight") as e:
        r.collect()
    assert e.value.code == -1
    batches = [batch_for(i) for i in range(depth)]
    for b in batches:
        r.submit(b)
    assert r.in_flight == depth
    with pytest.raises(vb.Vbm25Error, match="collect first") as e:   # full: refused, the ring unchanged
        r.submit(batches[0])
    assert e.value.code == -1 and r.in_flight == depth
    with pytest.raises(vb.Vbm25Error, match="collect first"):
        r.submit_keys(*keys_of(batches[0]))
    for b in batches:                                                 # submission order
        ids, off = r.collect()
        want_ids, want_off = expected(gix, b)
        assert np.array_equal(ids, want_ids) and np.array_equal(off, want_off)
    assert r.in_flight == 0
    with pytest.raises(vb.Vbm25Error, match="nothing is in flight"):
        r.collect()


def test_ring_50_rounds_on_one_resolver():
    gix, keys = index_of(1000)
    r = vb.Resolver(gix, 3, 8, 256, 8192, seed=SEED)
    pending = []
    for i in range(50):
        b = batch_for(i)
        if r.in_flight == 3:
            ids, off = r.collect()
            want = pending.pop(0)
            assert np.array_equal(ids, want[0]) and np.array_equal(off, want[1])
        if i % 2:
            r.submit_keys(*keys_of(b))
        else:
            r.submit(b)
        pending.append(expected(gix, b))
    while pending:
        ids, off = r.collect()
        want = pending.pop(0)
        assert np.array_equal(ids, want[0]) and np.array_equal(off, want[1])


@pytest.mark.parametrize("depth", [1, 16])
def test_ring_wraps_at_the_extreme_depths(depth):
    """2 * depth + 1 batches through a ring of `depth` slots: full, then collect one and submit one until none is left, then drained
    -- the cursor passes its end twice; the lexeme and the keys entry in turns, every batch against the host's query step"""
    gix, keys = index_of(1000)
    r = vb.Resolver(gix, depth, 8, 256, 8192, seed=SEED)
    bytes_at_create = r.device_bytes
    rng = np.random.default_rng(200 + depth)  # two to four queries of 0 .. 8 lexemes a batch, some of them unknown
    batches = [[[vocab_lexeme(int(t)) for t in rng.integers(0, 1030, int(rng.integers(0, 9)))] for _ in range(2 + i % 3)]
               for i in range(2 * depth + 1)]
    want = [expected(gix, b) for b in batches]
    got = []
    for i, b in enumerate(batches):
        if r.in_flight == depth:
            got.append(r.collect())
        if i % 2:
            r.submit_keys(*keys_of(b))
        else:
            r.submit(b)
        assert r.in_flight == min(i + 1, depth)
    while r.in_flight:
        got.append(r.collect())
    assert len(got) == len(batches)
    for i, ((ids, off), (want_ids, want_off)) in enumerate(zip(got, want)):
        assert np.array_equal(ids, want_ids) and np.array_equal(off, want_off), f"depth {depth}, batch {i}"
    assert r.device_bytes == bytes_at_create
    with pytest.raises(vb.Vbm25Error, match="nothing is in flight"):
        r.collect()


def test_refused_submit_then_a_good_one():
    gix, keys = index_of(1000)
    r = vb.Resolver(gix, 2, 4, 16, 64, seed=None)
    good = [[b"w0", b"w3", b"w3", b"zz"], [b"w999"]]
    L = vb.lib()
    refusals = [
        (lambda: r.submit([[b"w1"] * 17]), "max_lexemes"),                                   # over capacity: lexemes
        (lambda: r.submit([[b"w" * 15] * 5]), "max_bytes"),                                  # ... bytes
        (lambda: r.submit([[]] * 5), "max_queries"),                                         # ... queries
        (lambda: r.submit((np.zeros(4, np.uint8), np.array([0, 3, 2], np.uint64), np.array([0, 2], np.uint32))), "not monotone"),
        (lambda: r.submit((np.zeros(4, np.uint8), np.array([0, 2, 4], np.uint64), np.array([1, 2], np.uint32))), "not 0"),
        (lambda: r.submit((np.zeros(4, np.uint8), np.array([0, 2, 4], np.uint64), np.array([0, 2, 1], np.uint32))), "not monotone"),
        (lambda: r.submit_keys(np.zeros(32, np.uint8), np.array([0, 2, 1], np.uint32)), "not monotone"),
        (lambda: r.submit([[b"a-lexeme-of-more-than-16-bytes"]]), "needs the index's seed"),  # hash without seed
        (lambda: r.submit([[b"nul\0"]]), "needs the index's seed"),
    ]
    for call, text in refusals:
        with pytest.raises(vb.Vbm25Error, match=text) as e:
            call()
        assert e.value.code == -1 and r.in_flight == 0
    assert L.vbm25_resolver_submit_lexemes(r.h, None, None, None, 1) == -1 and r.in_flight == 0
    with pytest.raises(vb.Vbm25Error, match="depth"):
        vb.Resolver(gix, 0, 4, 16, 64)
    with pytest.raises(vb.Vbm25Error, match="depth"):
        vb.Resolver(gix, 17, 4, 16, 64)
    r.submit(good)
    ids, off = r.collect()
    want_ids, want_off = expected(gix, good, seed=None)
    assert np.array_equal(ids, want_ids) and np.array_equal(off, want_off) and off.tolist() == [0, 2, 3]


def test_four_threads_with_a_resolver_each_on_one_index():
    gix, keys = index_of(1000)
    batches = [[batch_for(100 * t + i) for i in range(12)] for t in range(4)]
    want = [[expected(gix, b) for b in bs] for bs in batches]
    errors = []

    def work(t):
        try:
            r = vb.Resolver(gix, 2, 8, 256, 8192, seed=SEED)
            got = []
            for b in batches[t]:
                if r.in_flight == 2:
                    got.append(r.collect())
                r.submit(b)
            while r.in_flight:
                got.append(r.collect())
            for (ids, off), (wi, wo) in zip(got, want[t]):
                assert np.array_equal(ids, wi) and np.array_equal(off, wo)
            assert len(got) == 12
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---------------------------------------------------------------- end to end

def test_sqllogictest_orders_through_search_batch_lexemes():
    from test_oracle_pins import _slt_index
    fixture = json.load(open(os.path.join(GOLD, "slt_corpus.json")))
    for case in fixture["expect"]:
        sel = {"all": range(1, 11), "even": range(2, 11, 2), "odd": range(1, 11, 2)}[case["ids"]]
        oix, q, ids = _slt_index(set(sel), fixture)
        desc, keep = vb.api.desc_from_arrays(
            dict(n_docs=oix.n_docs, n_terms=oix.n_terms, n_blocks=oix.n_blocks, sum_len=oix.sum_len, k1=oix.k1, b=oix.b), oix.arrays)
        gix = vb.GpuIndex(desc)
        lex = [t.encode() for t in fixture["query"]]
        hits, n = vb.search_batch_lexemes(gix, [lex], case["k"])
        assert [int(h["payload"][2]) for h in hits[0, :n[0]]] == case["order"], case["name"]
        ref = vb.search(gix, case["k"], vb.Query.from_tokens(lex))
        assert hits[0, :n[0]].tobytes() == ref.tobytes()


_SYNTH = {}


def synth():
    if not _SYNTH:
        seg = vb.Segment.synth(100_000, 5000, mean_len=60, len_mode=1, seed=3)
        rng = np.random.default_rng(5)
        toks = np.stack([rng.choice(5000, 5, replace=False) for _ in range(256)]).astype(np.uint32)
        terms = np.sort(seg.token_terms(toks.reshape(-1)).reshape(256, 5), axis=1)
        queries = [[b"%d" % t for t in row] for row in toks]  # (the synthetic vocabulary's lexemes are the tokens' decimal strings)
        _SYNTH.update(seg=seg, gix=vb.GpuIndex(seg), terms=terms, queries=queries)
    return _SYNTH


def test_lexemes_through_resolver_ring_into_stream_ring():
    s = synth()
    gix, terms, queries = s["gix"], s["terms"], s["queries"]
    assert (terms != MISS).all()
    k, per = 10, 32
    ref_hits, ref_n = vb.search_batch(gix, terms.reshape(-1), (np.arange(257) * 5).astype(np.uint32), k)
    batches = [queries[i:i + per] for i in range(0, 256, per)]
    res = vb.Resolver(gix, 2, per, per * 5, per * 5 * 8)
    stream = vb.Stream(gix, 3, per, per * 5, k)
    out_hits, out_n = [], []
    nxt = 0
    while nxt < 2:                                  # batch n + 1 resolves while batch n scans
        res.submit(batches[nxt])
        nxt += 1
    for _ in batches:
        ids, off = res.collect()
        if nxt < len(batches):
            res.submit(batches[nxt])
            nxt += 1
        if stream.in_flight == 3:
            h, n = stream.collect()
            out_hits.append(h)
            out_n.append(n)
        stream.submit(ids, off)
    while stream.in_flight:
        h, n = stream.collect()
        out_hits.append(h)
        out_n.append(n)
    got_hits, got_n = np.concatenate(out_hits), np.concatenate(out_n)
    # the id path: the same batches as term ids through the same kind of ring
    stream2 = vb.Stream(gix, 3, per, per * 5, k)
    id_hits, id_n = [], []
    for i in range(0, 256, per):
        if stream2.in_flight == 3:
            h, n = stream2.collect()
            id_hits.append(h)
            id_n.append(n)
        stream2.submit(terms[i:i + per].reshape(-1), (np.arange(per + 1) * 5).astype(np.uint32))
    while stream2.in_flight:
        h, n = stream2.collect()
        id_hits.append(h)
        id_n.append(n)
    # every byte of every record's fields (a record's two trailing padding bytes belong to no field; whether a scan writes them
    # depends on its route)
    for want_hits, want_n in ((np.concatenate(id_hits), np.concatenate(id_n)), (ref_hits, ref_n)):
        assert got_n.tobytes() == want_n.tobytes() and (want_n == k).all()
        assert got_hits["score"].tobytes() == want_hits["score"].tobytes()
        assert got_hits["doc_id"].tobytes() == want_hits["doc_id"].tobytes()
        assert got_hits["payload"].tobytes() == want_hits["payload"].tobytes()
    # the one-call form
    h1, n1 = vb.search_batch_lexemes(gix, queries, k)
    assert h1.tobytes() == ref_hits.tobytes() and n1.tobytes() == ref_n.tobytes()


def test_lexemes_into_search_batch_growing():
    import growing_data
    s = synth()
    seg, gix, terms, queries = s["seg"], s["gix"], s["terms"], s["queries"]
    grow, _ = growing_data.make_growing(seg.arrays()["term_key"], 300, seed=9, pool=np.unique(terms[:64]))
    gs = vb.GrowingSegment.from_dict(gix, grow)
    off = (np.arange(65) * 5).astype(np.uint32)
    ref_hits, ref_n = vb.search_batch_growing(gix, gs, terms[:64].reshape(-1), off, 10)
    res = vb.Resolver(gix, 1, 64, 320, 4096)
    res.submit(vb.pack_lexemes(queries[:64]))       # (the prepacked form)
    ids, q_off = res.collect()
    assert np.array_equal(ids, terms[:64].reshape(-1)) and np.array_equal(q_off, off)
    hits, n = vb.search_batch_growing(gix, gs, ids, q_off, 10)
    assert hits.tobytes() == ref_hits.tobytes() and n.tobytes() == ref_n.tobytes()
