"""One adversarial set of 16-byte token keys, shared by tests/test_key_order_data.py and tests/test_gpu_key_order.py.  The reference
orders keys with memcmp; the device code compares two big-endian 64-bit halves.  That is only memcmp if the low half is looked at
when the high halves are equal and if both halves compare unsigned -- so the keys here come in families that make exactly that
decide: equal first halves with tails on both sides of 0x80, equal second halves, byte 7 against byte 8, the byte order inside a
half, the two extremes, and some of corpus.token_keys' decimals (low half zero) so that the old shape is in the mix.
tests/test_key_order_data.py states what the GPU tests need of this list.  No GPU use."""
import numpy as np

from corpus import token_keys

MISS = 0xFFFFFFFF
P = b"abcdefgh"
HEADS = (P, b"\x80" * 8, b"\xff" * 8)                      # first halves: plain, the sign bit alone, all ones
TAILS = (b"", b"\x01", b"1", b"2", b"\x7f", b"\x80", b"\xff", b"\0" * 7 + b"\x01", b"\xff" * 8)
N_DECIMAL = 40


def pad(raw):
    assert len(raw) <= 16
    return bytes(raw).ljust(16, b"\0")


def _families():
    keys = [head + tail for head in HEADS for tail in TAILS]                         # equal first halves
    keys += [b"1bcdefghXYZ", b"2bcdefghXYZ", b"\x7fbcdefghXYZ", b"\x80bcdefghXYZ",    # equal second halves: byte 0 ...
             b"abcdefg\x7fXYZ", b"abcdefg\x80XYZ"]                                    # ... and byte 7 decide
    keys += [b"\x01" * 7 + b"\x02", b"\x01" * 8 + b"\x03"]                            # byte 7 against byte 8
    keys += [b"\x02\x01", b"\x01\x02", P + b"\x02\x01", P + b"\x01\x02"]              # the byte order inside a half
    keys += [b"internation", b"international", b"internationale", b"internationals",  # real lexemes of one 8-byte prefix, each a
             b"internationally"]                                                      # prefix of the next or its neighbour
    keys += [b"\0" * 15 + b"\x01", b"\xff" * 16]                                      # the two extremes (the second is also HEADS[2]'s)
    keys += [bytes(k) for k in token_keys(N_DECIMAL)[0]]                              # the old shape: decimals, low half zero
    return [pad(k) for k in keys]


def halves(keys):
    """(high, low) of 16-byte keys as big-endian uint64 arrays: memcmp order is the order of the pairs"""
    k = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, 16) if len(keys) else np.zeros((0, 16), np.uint8)
    return k[:, :8].copy().view(">u8").ravel().astype(np.uint64), k[:, 8:].copy().view(">u8").ravel().astype(np.uint64)


def lexsorted(keys):
    """the keys in numpy's lexsort order of (low, high) halves"""
    hi, lo = halves(keys)
    return [keys[i] for i in np.lexsort((lo, hi))]


def lexeme_of(key):
    """the short lexeme whose key this is (vector.rs:21-24: fewer than 16 bytes, no NUL, zero padded), or None"""
    raw = key.rstrip(b"\0")
    return raw if raw and len(raw) <= 15 and b"\0" not in raw else None


KEYS = lexsorted(sorted(set(_families())))                  # distinct, ascending; an odd number, so ABSENT lies inside SEALED
SEALED, ABSENT = KEYS[0::2], KEYS[1::2]
LEXEMES = [lexeme_of(k) for k in KEYS if lexeme_of(k)]
LEX_SEALED = [lexeme_of(k) for k in SEALED if lexeme_of(k)]  # the same split: a lexeme is sealed where its key is
LEX_ABSENT = [lexeme_of(k) for k in ABSENT if lexeme_of(k)]


# ---- what makes a key set sensitive (counted by tests/test_key_order_data.py and by the GPU tests on the vocabularies they build)

def first_half(key):
    return key[:8]


def adjacent_pairs_sharing(keys, half):
    """pairs of neighbours of the ascending list `keys` whose first (half = 0) or second (half = 1) 8 bytes are equal"""
    return sum(a[8 * half:8 * half + 8] == b[8 * half:8 * half + 8] for a, b in zip(keys, keys[1:]))


def absent_sharing_first_half(absent, sealed):
    heads = {first_half(k) for k in sealed}
    return sum(first_half(k) in heads for k in absent)


def across_the_sign_bit(keys):
    """keys that share the first half with a key whose byte 8 lies on the other side of 0x80"""
    return sum(any(first_half(o) == first_half(k) and (o[8] < 0x80) != (k[8] < 0x80) for o in keys) for k in keys)


# ---- builders

def as_array(keys):
    return np.frombuffer(b"".join(keys), dtype=np.uint8).copy() if keys else np.zeros(0, np.uint8)


def sealed_args(keys=None, n_docs=200, seed=1):
    """(doc_len, doc_payload, term_key, term_start, post_doc, post_tf) for Segment.build / DeviceSegment.build over the ascending
    `keys`: every term in 1 to 150 of the n_docs documents (1, 2, 127 .. 129 and 150 among them: terms of one and of two blocks),
    tfs 1 .. 5, lengths the tf sums plus a rest"""
    keys = SEALED if keys is None else keys
    rng = np.random.default_rng(seed)
    fixed = [1, 2, 127, 128, 129, 150]
    post_doc, post_tf, term_start = [], [], [0]
    for t in range(len(keys)):
        df = fixed[t // 3 % len(fixed)] if t % 3 == 0 else int(rng.integers(1, 60))
        post_doc.append(np.sort(rng.choice(n_docs, df, replace=False)))
        post_tf.append(rng.integers(1, 6, df))
        term_start.append(term_start[-1] + df)
    post_doc, post_tf = np.concatenate(post_doc).astype(np.uint32), np.concatenate(post_tf).astype(np.uint32)
    doc_len = (np.bincount(post_doc, weights=post_tf, minlength=n_docs) + rng.integers(0, 30, n_docs)).astype(np.uint32)
    payload = rng.integers(0, 65535, (n_docs, 3)).astype(np.uint16)
    return doc_len, payload, as_array(keys), np.array(term_start, np.uint64), post_doc, post_tf


def growing(sealed=None, extra=None, n_random=100, seed=2, deleted=0.15):
    """(G, g_term) in the form growing_data.make_growing returns, over the sealed keys and the keys `extra` the sealed segment lacks.
    Document j < len(extra) is live and holds extra[j] together with sealed keys of OTHER first halves: a lookup that stops at the
    first half finds extra[j]'s sealed neighbours in it.  n_random more documents draw 1 .. 12 keys of the whole universe; some of
    those are deleted.  Elements ascend in key order, tf 1 .. 5."""
    sealed = SEALED if sealed is None else sealed
    extra = ABSENT if extra is None else extra
    rng = np.random.default_rng(seed)
    universe = lexsorted(sorted(set(sealed) | set(extra)))
    rank = {k: i for i, k in enumerate(sealed)}
    docs, dele = [], []
    for k in extra:
        others = [s for s in sealed if first_half(s) != first_half(k)]
        pick = [others[i] for i in rng.choice(len(others), min(len(others), int(rng.integers(2, 9))), replace=False)] if others else []
        docs.append(lexsorted(sorted(set(pick) | {k})))
        dele.append(0)
    for _ in range(n_random):
        n = int(rng.integers(1, 13))
        docs.append(lexsorted([universe[i] for i in rng.choice(len(universe), min(n, len(universe)), replace=False)]))
        dele.append(int(rng.random() < deleted))
    flat = [k for d in docs for k in d]
    G = dict(g_start=np.r_[0, np.cumsum([len(d) for d in docs])].astype(np.uint64), g_key=as_array(flat),
             g_tf=rng.integers(1, 6, len(flat)).astype(np.uint32), g_fieldnorm=rng.integers(0, 200, len(docs)).astype(np.uint8),
             g_payload=rng.integers(0, 65535, (len(docs), 3)).astype(np.uint16), g_deleted=np.array(dele, np.uint8))
    return G, np.array([rank.get(k, MISS) for k in flat], dtype=np.uint32)


def documents_of(G):
    """the growing CSR's documents as lists of keys"""
    key = G["g_key"].reshape(-1, 16)
    s = G["g_start"].astype(np.int64)
    return [[key[e].tobytes() for e in range(s[g], s[g + 1])] for g in range(len(s) - 1)]


def misled_terms(G, sealed=None, absent=None):
    """sealed terms t with a live document that holds an absent key of t's first half but not t itself: the documents a lookup
    blind to the low half would score for t"""
    sealed = SEALED if sealed is None else sealed
    absent = set(ABSENT if absent is None else absent)
    live = [set(d) for d, gone in zip(documents_of(G), G["g_deleted"]) if not gone]
    return [t for t in sealed if any(t not in d and any(k in absent and first_half(k) == first_half(t) for k in d) for d in live)]


def lexeme_docs(lexemes=None, n_random=150, seed=3):
    """documents of (lexeme, count) for the cast routes: every lexeme of `lexemes` in at least one document (document j holds
    lexeme j), 1 .. 10 more draws each with repeats (the dedup's business), counts 1 .. 3; then n_random documents of draws only, a
    document without lexemes among them"""
    lexemes = LEXEMES if lexemes is None else lexemes
    rng = np.random.default_rng(seed)
    docs = []
    for j in range(len(lexemes) + n_random):
        n = int(rng.integers(1, 11))
        d = [(lexemes[int(i)], int(c)) for i, c in zip(rng.integers(0, len(lexemes), n), rng.integers(1, 4, n))]
        if j < len(lexemes):
            d.insert(int(rng.integers(0, len(d) + 1)), (lexemes[j], 1 + j % 3))
        docs.append(d)
    docs[len(lexemes) + 1] = []
    return docs
