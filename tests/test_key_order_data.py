"""What tests/test_gpu_key_order.py needs of tests/key_order_data.py, stated here so that a later edit of the data cannot hollow the
GPU tests out: enough neighbours that only the low half tells apart, enough that only the high half tells apart, both sides of the
sign bit -- and the host side (Python's bytes order, Segment.build, vb.intern, growing_search) agreeing with numpy's lexsort on the
(low, high) halves.  The counts are conditions, not measurements: if one fails, mend the key list, not the bound.  No GPU use.
(GpuIndex.lookup_terms needs an index in HBM: its half of the host-side agreement is the first test of the GPU file.)"""
import numpy as np

import key_order_data as K
import vectorchord_bm25_amd as vb


def padded(lexemes):
    return [K.pad(l) for l in lexemes]


def test_the_list_is_distinct_ascending_and_split_by_alternating_position():
    assert len(set(K.KEYS)) == len(K.KEYS) and all(len(k) == 16 for k in K.KEYS)
    assert K.KEYS == sorted(K.KEYS)                       # lexsort of the halves is memcmp (Python's bytes order)
    assert K.SEALED == K.KEYS[0::2] and K.ABSENT == K.KEYS[1::2] and len(K.KEYS) % 2 == 1
    for k in K.ABSENT:                                    # every absent key lies between two sealed ones
        assert K.SEALED[0] < k < K.SEALED[-1]
    assert not set(K.SEALED) & set(K.ABSENT)
    assert K.pad(b"\0" * 15 + b"\x01") == K.KEYS[0] and K.KEYS[-1] == b"\xff" * 16
    decimals = [k for k in K.KEYS if k.rstrip(b"\0").isdigit()]
    assert len(decimals) == K.N_DECIMAL                   # the old shape is in the mix


def test_sealed_and_absent_keys_need_the_low_half_and_unsigned_compares():
    assert K.adjacent_pairs_sharing(K.SEALED, 0) >= 12
    assert K.adjacent_pairs_sharing(K.SEALED, 1) >= 4
    assert K.absent_sharing_first_half(K.ABSENT, K.SEALED) >= 12
    assert K.across_the_sign_bit(K.SEALED) >= 6
    # the second halves that neighbours share are not all zero, and first halves differ across the sign bit of byte 0 too
    assert any(a[8:] == b[8:] != bytes(8) for a, b in zip(K.KEYS, K.KEYS[1:]))
    assert {k[0] >= 0x80 for k in K.SEALED} == {False, True} == {k[0] >= 0x80 for k in K.ABSENT}


def test_the_lexemes_keep_the_conditions():
    assert all(len(l) <= 15 and b"\0" not in l and l for l in K.LEXEMES)
    assert sorted(K.LEX_SEALED + K.LEX_ABSENT) == sorted(K.LEXEMES) and len(set(K.LEXEMES)) == len(K.LEXEMES)
    assert set(padded(K.LEX_SEALED)) <= set(K.SEALED) and set(padded(K.LEX_ABSENT)) <= set(K.ABSENT)
    sealed, absent = padded(K.LEX_SEALED), padded(K.LEX_ABSENT)
    assert sealed == sorted(sealed)
    assert K.adjacent_pairs_sharing(sealed, 0) >= 6
    assert K.adjacent_pairs_sharing(sealed, 1) >= 6
    assert K.absent_sharing_first_half(absent, sealed) >= 6
    assert K.across_the_sign_bit(sealed) >= 3


def test_intern_of_every_lexeme_is_the_padded_bytes():
    for l in K.LEXEMES:
        assert vb.intern(l) == K.pad(l) == vb.intern(l, bytes(range(32)))
    assert vb.Query.from_tokens(K.LEXEMES).keys == sorted(padded(K.LEXEMES)) == K.lexsorted(padded(K.LEXEMES))


def test_segment_build_accepts_the_vocabulary_in_lexsort_order():
    args = K.sealed_args()
    seg = vb.Segment.build(1.2, 0.75, *args)
    assert seg.n_terms == len(K.SEALED) and seg.n_docs == 200
    assert seg.arrays()["term_key"].tobytes() == b"".join(K.SEALED)
    df = np.diff(args[3].astype(np.int64))
    assert df.min() >= 1 and df.max() == 150 and {1, 2, 127, 128, 129, 150} <= set(df.tolist())
    assert seg.n_blocks > seg.n_terms                     # some terms span two blocks
    assert 1 <= args[5].min() and args[5].max() == 5
    # two neighbours that differ in the low half only, swapped: refused
    at = next(i for i in range(len(K.SEALED) - 1) if K.SEALED[i][:8] == K.SEALED[i + 1][:8])
    swapped = list(K.SEALED)
    swapped[at], swapped[at + 1] = swapped[at + 1], swapped[at]
    bad = list(args)
    bad[2] = K.as_array(swapped)
    try:
        vb.Segment.build(1.2, 0.75, *bad)
    except vb.Vbm25Error as e:
        assert e.code == -1 and "strictly ascending" in str(e)
    else:
        raise AssertionError("keys that descend in the low half were accepted")


def test_the_growing_csr_misleads_a_lookup_that_stops_at_the_first_half():
    G, g_term = K.growing()
    docs = K.documents_of(G)
    assert all(d == sorted(d) and len(set(d)) == len(d) for d in docs)     # ascending, distinct
    assert 0 < G["g_deleted"].sum() < len(docs) and len(docs) <= 300
    held = {k for d in docs for k in d}
    assert set(K.ABSENT) <= held and len(held & set(K.SEALED)) > len(K.SEALED) // 2
    assert len(K.misled_terms(G)) >= 10
    # g_term: the rank among the sealed keys, MISS for the others
    rank = {k: i for i, k in enumerate(K.SEALED)}
    assert g_term.tolist() == [rank.get(k, K.MISS) for d in docs for k in d]


def test_the_host_search_tells_the_low_halves_apart():
    """vbm25_growing_search (the host side of the GPU tests' host composition) over the growing CSR: a query of one sealed key finds
    exactly the live documents that hold that key"""
    seg = vb.Segment.build(1.2, 0.75, *K.sealed_args())
    G, g_term = K.growing()
    docs = K.documents_of(G)
    for t, key in enumerate(K.SEALED):
        hits = vb.growing_search(seg, vb.Query([key]), 1000, **G)
        got = sorted(int(0xFFFFFFFF - d) for d in hits["doc_id"])
        want = [g for g, d in enumerate(docs) if key in d and not G["g_deleted"][g]]
        assert got == want, (t, key)


def test_the_cast_documents_hold_every_lexeme():
    docs = K.lexeme_docs()
    assert len(docs) <= 300 and [] in docs
    assert {l for d in docs for l, _ in d} == set(K.LEXEMES)
    assert any(len({l for l, _ in d}) < len(d) for d in docs)             # repeats inside a document
