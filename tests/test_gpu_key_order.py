"""16-byte key order on every device path, with keys where the LOW half decides (tests/key_order_data.py): the reference orders token
keys with memcmp, the device code compares two big-endian 64-bit halves in five places (cast_lane.h, resolve_lane.h,
growing_build.h, maintain.hip, vectors_parse.h) and sorts whole keys as two stable 64-bit radix passes in two (cast.hip's
build_documents, maintain.hip's new keys).  Every other GPU test's vocabulary has a zero low half or halves that never collide, so
none of them makes "first halves equal, look at the second" decide anything; here it decides everywhere.  Every comparison is exact
(bytes or bits) against the host side or a numpy model; the helpers are the older files' own.  -m gpu only."""
import numpy as np
import pytest

import cast_model as cm
import key_order_data as K
import orc
import pages_write_data as W
import vectorchord_bm25_amd as vb
import vectors_device_data as V
from parity import assert_bit_exact
from test_gpu_evaluate_documents import assert_bound, bits
from test_gpu_growing import check_both
from test_gpu_growing_append import attach, check_step, concat
from test_gpu_growing_append import docs as csr_docs
from test_gpu_maintain import compact_and_check
from test_gpu_resolve import SEED, expected
from test_gpu_vectors_device import assert_refused_like_the_composition

pytestmark = pytest.mark.gpu
MISS = K.MISS
K_ALL = 400  # more records than a query can match here (200 sealed documents and fewer than 200 growing ones)


@pytest.fixture(scope="module")
def sealed():
    """the sealed index over K.SEALED: (build arguments, host segment, GpuIndex)"""
    args = K.sealed_args()
    seg = vb.Segment.build(1.2, 0.75, *args)
    return args, seg, vb.GpuIndex(seg)


@pytest.fixture(scope="module")
def grown():
    return K.growing()[0]


def term_queries(n_terms, seed=5):
    """one query per sealed term, six of 3 to 8 terms, one with ids >= n_terms behind its terms -> (terms, off)"""
    rng = np.random.default_rng(seed)
    rows = [[t] for t in range(n_terms)]
    rows += [sorted(rng.choice(n_terms, n, replace=False).tolist()) for n in (3, 4, 5, 6, 7, 8)]
    rows.append(rows[-3] + [n_terms + 3, 0xFFFFFFFF])
    return np.array([t for r in rows for t in r], np.uint32), np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint32)


def test_lookup_terms_on_the_host_agrees_with_lexsort(sealed):
    """the yardstick of the resolver and bind tests first: every sealed key at its lexsort rank, every absent one missed"""
    _, seg, gix = sealed
    assert gix.lookup_terms(K.SEALED).tolist() == list(range(len(K.SEALED)))
    assert gix.lookup_terms(K.ABSENT).tolist() == [MISS] * len(K.ABSENT)
    mixed = K.KEYS[::-1]
    rank = {k: i for i, k in enumerate(K.SEALED)}
    assert gix.lookup_terms(mixed).tolist() == [rank.get(k, MISS) for k in mixed]


# ---- CREATE INDEX from documents: build_documents' two radix passes, build_flag_kernel's key_equal, the cast's key_less

@pytest.mark.parametrize("k1,b", [(1.2, 0.75), (2.0, 0.0)])
def test_create_index_from_documents(k1, b):
    docs = K.lexeme_docs()
    pay = cm.payloads(len(docs))
    model = cm.shared("key order: cast", lambda: cm.cast(docs, pay))
    want = cm.build_segment(model, k1, b)
    vocab = [bytes(k) for k in want.arrays()["term_key"].reshape(-1, 16)]
    assert vocab == sorted(K.pad(l) for l in K.LEXEMES)
    assert K.adjacent_pairs_sharing(vocab, 0) >= 12 and K.adjacent_pairs_sharing(vocab, 1) >= 4 and K.across_the_sign_bit(vocab) >= 6
    h = vb.Documents.cast(docs, pay, seed=cm.SEED)
    cm.assert_same(h.download(), model, "the cast")
    dseg = vb.DeviceSegment.from_documents(h, k1, b)
    assert (dseg.n_docs, dseg.n_terms) == (len(docs), len(K.LEXEMES))
    cm.same_segment(dseg.download(), want, f"k1={k1} b={b}")


# ---- growing upload and search: key_cmp in grow_map_kernel

def test_growing_upload_and_search(sealed, grown):
    _, seg, gix = sealed
    G = grown
    assert len(K.misled_terms(G)) >= 10 and len(G["g_start"]) - 1 < 200
    gs = vb.GrowingSegment(gix, **G)
    terms, off = term_queries(seg.n_terms)
    for k in (10, K_ALL):
        want = check_both(seg, gix, gs, terms, off, k, G, f"k={k}")
    # at K_ALL every match is a record: the growing records of a one-term query are exactly the live documents that hold the key
    docs = K.documents_of(G)
    for t, key in enumerate(K.SEALED):
        got = sorted(int(0xFFFFFFFF - d) for d in want[t]["doc_id"] if d > 0xFFFFFFFF - len(docs))
        assert got == [g for g, d in enumerate(docs) if key in d and not G["g_deleted"][g]], f"term {t}"
    assert max(len(w) for w in want) < K_ALL


# ---- append: key_cmp in grow_append_map_kernel, the cast's order in append_documents

def test_append_of_a_csr_and_of_cast_documents(sealed, grown):
    _, seg, gix = sealed
    G = grown
    n = len(G["g_start"]) - 1
    n0 = n // 3
    terms, off = term_queries(seg.n_terms)
    gs = vb.GrowingSegment(gix, **csr_docs(G, 0, n0))
    batches = attach(gix, gs, terms, off, [10, K_ALL])
    gs.append(**csr_docs(G, n0, n))
    check_step(seg, gix, gs, batches, terms, off, csr_docs(G, 0, n), "a prefix plus append of the rest")
    docs = K.lexeme_docs(n_random=20, seed=9)   # sealed and absent lexemes mixed in every document
    pay = cm.payloads(len(docs), seed=9)
    gs.append_documents(vb.Documents.cast(docs, pay, seed=cm.SEED))
    now = concat(csr_docs(G, 0, n), cm.cast(docs, pay))
    assert len(now["g_start"]) - 1 < 300
    assert len(K.misled_terms(cm.cast(docs, pay))) >= 6
    check_step(seg, gix, gs, batches, terms, off, now, "append_documents of cast lexemes", ks=[10, K_ALL, 2 * K_ALL])


# ---- compaction, twice on one lineage: mt_key_split / mt_lower_bound / mt_unique_flag / mt_merge and the two-pass sort of new keys

def test_compaction_twice_on_one_lineage():
    first, second = K.SEALED[0::2], K.SEALED[1::2]
    args = K.sealed_args(first, seed=4)
    seg = vb.Segment.build(1.2, 0.75, *args)
    gix = vb.GpuIndex(seg)
    # 1: the growing segment brings the other half of SEALED in, every 4th sealed document goes
    G1, _ = K.growing(first, second, n_random=60, seed=6)
    ds1, got1, _ = compact_and_check(gix, seg, np.arange(seg.n_docs) % 4 == 1, G1, "first compaction")
    vocab1 = [bytes(k) for k in got1.arrays()["term_key"].reshape(-1, 16)]
    assert vocab1 == K.SEALED
    assert K.adjacent_pairs_sharing(vocab1, 0) >= 12 and K.absent_sharing_first_half(second, first) >= 6
    # 2: ABSENT against sealed keys whose low halves are not zero, and against each other
    gix1 = vb.GpuIndex(ds1)
    G2, _ = K.growing(vocab1, K.ABSENT, n_random=60, seed=7)
    ds2, got2, _ = compact_and_check(gix1, got1, np.arange(got1.n_docs) % 5 == 2, G2, "second compaction")
    vocab2 = [bytes(k) for k in got2.arrays()["term_key"].reshape(-1, 16)]
    assert vocab2 == K.KEYS and got2.n_docs <= 300 + 200
    # the final index against the oracle's brute force
    cix = vb.GpuIndex(ds2)
    assert cix.lookup_terms(K.KEYS).tolist() == list(range(len(K.KEYS)))
    terms, off = term_queries(got2.n_terms)
    oix = orc.OracleIndex.from_arrays(got2.meta(), got2.arrays())
    hits, nh = vb.search_batch(cix, terms, off, 10)
    ref, nref, _ = oix.search_batch(terms, off, 10, mode="brute", threads=4)
    assert np.array_equal(nh, nref) and nh[:got2.n_terms].min() >= 1
    for q in range(len(nh)):
        assert_bit_exact(ref[q, :nref[q]], hits[q, :nh[q]], what=f"after two compactions q{q}")


# ---- the resolver: key_order / lookup_lane in lookup_kernel, the cast-style dedup in front of it

def key_queries():
    rng = np.random.default_rng(8)
    pick = lambda pool, n: [pool[int(i)] for i in rng.choice(len(pool), n, replace=False)]
    return [list(K.SEALED), list(K.ABSENT), K.KEYS[::-1][:64], K.SEALED[:20] + K.ABSENT[:20] + K.SEALED[:20][::-1],
            [], [K.SEALED[0]], [K.ABSENT[0]], [K.KEYS[-1], K.KEYS[0]], pick(K.KEYS, 30), pick(K.KEYS, 63),
            sorted(pick(K.KEYS, 40), reverse=True), [k for k in K.KEYS if k[:8] == K.P] * 2]


def submit_keys(r, queries):
    flat = [k for q in queries for k in q]
    r.submit_keys(K.as_array(flat), np.cumsum([0] + [len(q) for q in queries]).astype(np.uint32))
    return r.collect()


def test_resolver_keys_and_lexemes(sealed):
    _, seg, gix = sealed
    r = vb.Resolver(gix, 1, 32, 1024, 1 << 14, seed=SEED)
    qs = key_queries()
    assert max(len(q) for q in qs) == 64                                   # the wave path
    want_ids, want_off = expected(gix, qs, interned=True)
    ids, off = submit_keys(r, qs)
    assert np.array_equal(off, want_off) and np.array_equal(ids, want_ids)
    assert off[1] == len(K.SEALED) and off[2] == off[1]                    # every sealed key found, no absent one
    q65 = K.KEYS[:65]
    qs2 = qs + [q65]                                                       # one 65-key query in the batch: the general path
    want_ids2, want_off2 = expected(gix, qs2, interned=True)
    ids2, off2 = submit_keys(r, qs2)
    assert np.array_equal(off2, want_off2) and np.array_equal(ids2, want_ids2)
    assert ids2[:len(ids)].tobytes() == ids.tobytes() and off2[-1] - off2[-2] == len([k for k in q65 if k in set(K.SEALED)])
    # the lexeme entry: the same lookups behind intern_lane
    lq = [list(K.LEX_SEALED), list(K.LEX_ABSENT), K.LEXEMES[::-1][:64], K.LEX_ABSENT[:9] + K.LEX_SEALED[:9] + K.LEX_ABSENT[:9]]
    for batch in (lq, lq + [K.LEXEMES[:65]]):
        want_ids, want_off = expected(gix, batch)
        r.submit(batch)
        ids, off = r.collect()
        assert np.array_equal(off, want_off) and np.array_equal(ids, want_ids)
        assert off[1] == len(K.LEX_SEALED) and off[2] == off[1]


# ---- bind and evaluate: lookup_lane in bind_lookup_kernel, then the `<&>` scores

def test_bind_and_evaluate(sealed):
    _, seg, gix = sealed
    r = vb.Resolver(gix, 1, 64, 4096, 1 << 16, seed=cm.SEED)
    lo, hi = K.LEX_ABSENT[0], K.LEX_ABSENT[-1]
    inner_s = [l for l in K.LEX_SEALED if K.pad(lo) < K.pad(l) < K.pad(hi)]
    edge = [
        [(lo, 2)] + [(l, 1) for l in inner_s[:5]],                        # an absent lexeme first
        [(l, 2) for l in inner_s[:5]] + [(hi, 1)],                        # ... last
        [(l, 1 + i % 3) for i, l in enumerate(K.LEXEMES)],                # ... between: every lexeme, sealed and absent alternate
        [(l, 1) for l in K.LEX_ABSENT],                                   # only absent ones
        [(l, 3) for l in K.LEX_SEALED][::-1],                             # only sealed ones, given descending
        [],
    ]
    docs = edge + K.lexeme_docs(n_random=40, seed=12)
    h = vb.Documents.cast(docs, None, seed=cm.SEED)
    dl = h.download()
    cm.assert_same(dl, cm.cast(docs), "the cast")
    dt = h.bind(r)
    assert_bound(dt, dl, gix, "key order documents")
    start, term, tf = dt.download()
    n = np.diff(start.astype(np.int64))
    assert n[:6].tolist() == [5, 5, len(K.LEX_SEALED), 0, len(K.LEX_SEALED), 0]
    assert term[start[2]:start[3]].tolist() == gix.lookup_terms([K.pad(l) for l in K.LEX_SEALED]).tolist()
    # evaluate: one query per sealed lexeme, some of several lexemes with absent ones among them, against vb.evaluate on the host
    queries = [[l] for l in K.LEX_SEALED] + [K.LEXEMES[i::7] for i in range(7)] + [list(K.LEX_ABSENT), []]
    r.submit(queries)
    term_ids, q_off = r.collect()
    want_ids, want_off = expected(gix, queries, seed=cm.SEED)
    assert np.array_equal(term_ids, want_ids) and np.array_equal(q_off, want_off)
    got = dt.evaluate(term_ids, q_off)
    key = np.asarray(dl["g_key"]).reshape(-1, 16)
    s = dl["g_start"].astype(np.int64)
    host_docs = [([bytes(k) for k in key[s[d]:s[d + 1]]], dl["g_tf"][s[d]:s[d + 1]]) for d in range(len(docs))]
    want = np.zeros(got.shape, dtype=np.float64)
    for q in range(len(queries)):
        query = vb.Query([K.SEALED[t] for t in term_ids[q_off[q]:q_off[q + 1]]])
        for d, (dk, dtf) in enumerate(host_docs):
            want[q, d] = vb.evaluate(seg, dk, dtf, query)
    assert np.array_equal(bits(got), bits(want)), f"{(bits(got) != bits(want)).sum()} of {want.size} scores differ"
    assert (want != 0).mean() > 0.02 and (want[:, 3] == 0).all()         # (the document of absent lexemes scores nothing)


# ---- pages: the device writer and the device reader (the keys travel as bytes; the reader checks their order)

def test_pages_round_trip(sealed):
    args, seg, _ = sealed
    ds = vb.DeviceSegment.build(1.2, 0.75, *args)
    cm.same_segment(ds.download(), seg, "the device build")
    pl = ds.to_relation(W.SEED)
    W.assert_same_pages(pl, W.oracle_relation(seg), "the written relation")
    back = vb.DeviceSegment.from_pages(pl)
    got = back.download()
    cm.same_segment(got, ds.download(), "read back against the source")
    cm.same_segment(got, vb.segment_from_pages(pl), "read back against the host page reader")
    assert got.arrays()["term_key"].tobytes() == b"".join(K.SEALED)
    assert vb.GpuIndex(back).lookup_terms(K.KEYS).tolist() == vb.GpuIndex(seg).lookup_terms(K.KEYS).tolist()


# ---- the vectors tape: key_half_be in vec_check_kernel

TAPE_PAIRS = {
    "byte 15": (K.P + b"\0" * 7 + b"\x01", K.P + b"\0" * 7 + b"\x02"),   # the two keys differ in the last byte only
    "byte 8 across the sign bit": (K.P + b"\x7f" + b"\0" * 7, K.P + b"\x80" + b"\0" * 7),
}


def tape_with(a, b):
    """a tape of three documents; the middle one holds `a` then `b` between a smaller and a larger key"""
    small = V.elements([V.key_of(5), V.key_of(9)], [2, 3])
    mid = V.elements([K.pad(b"abc"), a, b, K.pad(b"zzz")], [1, 2, 3, 4])
    return V.hand_relation([[V.t2(3), V.t0(small, (1, 2, 3)), V.t2(9), V.t0(mid, (4, 5, 6))], [V.t2(3), V.t0(small, (7, 8, 9))]])


@pytest.mark.parametrize("name", sorted(TAPE_PAIRS))
def test_vectors_tape_order_in_the_low_half(name):
    lo, hi = TAPE_PAIRS[name]
    assert lo < hi and lo[:8] == hi[:8] and len(lo) == 16
    gix = vb.GpuIndex(vb.segment_from_pages(V.hand_relation([[], [], []])))
    good = tape_with(lo, hi)
    want = vb.growing_from_pages(good)
    gs, csr = vb.GrowingSegment.from_pages(gix, good, return_csr=True)
    V.assert_same_csr(csr, want, f"{name}: the ascending twin")
    assert gs.n_docs == 3 and csr["g_key"].reshape(-1, 16)[3].tobytes() == lo
    bad = tape_with(hi, lo)
    assert V.first_unordered_document(vb.growing_from_pages(bad)) == 1
    code = assert_refused_like_the_composition(gix, bad, f"{name}: descending")   # the host route's code and message
    assert code == -1 and "document 1: keys must be strictly ascending" in vb.lib().vbm25_last_error().decode()
    same = tape_with(lo, lo)                                                     # equal keys are not ascending either
    assert assert_refused_like_the_composition(gix, same, f"{name}: equal") == -1
