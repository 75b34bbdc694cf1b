"""The host model of the document cast (cast_tsvector_to_document, src/datatype/tsvector.rs:84-127) and of its two consumers, for
tests/test_gpu_cast*.py and tests/test_gpu_table_cast.py: per document vb.intern on each lexeme, a Python sort on the key bytes and a
saturating merge; the length is the saturating sum, the fieldnorm np.searchsorted on vbm25_fieldnorm_table."""
import ctypes as C

import numpy as np

import vectorchord_bm25_amd as vb

U32_MAX = 0xFFFFFFFF
SEED = bytes(range(7, 39))


def fieldnorm_table():
    t = np.zeros(256, dtype=np.uint32)
    vb._lib.check(vb.lib().vbm25_fieldnorm_table(t.ctypes.data_as(C.c_void_p)))
    return t


_TABLE = None
_KEYS = {}


def _intern(lexeme, seed):
    k = _KEYS.get((lexeme, seed))
    if k is None:
        k = _KEYS[(lexeme, seed)] = vb.intern(lexeme, seed)
    return k


def cast(docs, payload=None, seed=SEED):
    """docs: lists of (lexeme, count) -> the dict Documents.download() returns"""
    global _TABLE
    if _TABLE is None:
        _TABLE = fieldnorm_table()
    start, keys, tfs, lengths = [0], [], [], []
    for doc in docs:
        merged = {}
        for lexeme, count in doc:
            k = _intern(bytes(lexeme), seed)
            merged[k] = min(merged.get(k, 0) + count, U32_MAX)
        length = 0
        for k in sorted(merged):
            keys.append(k)
            tfs.append(merged[k])
            length = min(length + merged[k], U32_MAX)
        start.append(len(keys))
        lengths.append(length)
    length = np.array(lengths, dtype=np.uint32)
    n = len(docs)
    return dict(g_start=np.array(start, dtype=np.uint64),
                g_key=np.frombuffer(b"".join(keys), dtype=np.uint8).copy() if keys else np.zeros(0, np.uint8),
                g_tf=np.array(tfs, dtype=np.uint32),
                g_fieldnorm=(np.searchsorted(_TABLE, length, side="right") - 1).astype(np.uint8),
                g_payload=None if payload is None else np.ascontiguousarray(payload, dtype=np.uint16).reshape(n, 3),
                g_deleted=np.zeros(n, dtype=np.uint8), length=length)


def assert_same(got, want, what=""):
    for name in ("g_start", "g_key", "g_tf", "g_fieldnorm", "g_deleted", "length"):
        assert np.array_equal(np.asarray(got[name]).reshape(-1), np.asarray(want[name]).reshape(-1)), f"{what}: {name} differs"
    if want["g_payload"] is None:
        assert got["g_payload"] is None, f"{what}: a payload where none was given"
    else:
        assert np.array_equal(np.asarray(got["g_payload"]).reshape(-1, 3), want["g_payload"]), f"{what}: g_payload differs"


def payloads(n, seed=5):
    return np.random.default_rng(seed).integers(0, 65535, (n, 3)).astype(np.uint16)


def build_segment(model, k1, b):
    """What ambuild + io.rs + flush.rs make of the model's documents, on the host: the vocabulary is sorted(set(keys)), every element a
    mapping, Segment.build encodes."""
    key = model["g_key"].reshape(-1, 16)
    start = model["g_start"].astype(np.int64)
    key_bytes = [k.tobytes() for k in key]
    vocab = sorted(set(key_bytes))
    rank = {k: i for i, k in enumerate(vocab)}
    term = np.array([rank[k] for k in key_bytes], dtype=np.int64)
    doc = np.repeat(np.arange(len(start) - 1), np.diff(start))
    order = np.lexsort((doc, term))
    term_start = np.zeros(len(vocab) + 1, dtype=np.uint64)
    np.add.at(term_start, term + 1, 1)
    term_start = np.cumsum(term_start).astype(np.uint64)
    term_key = np.frombuffer(b"".join(vocab), dtype=np.uint8) if vocab else np.zeros(0, np.uint8)
    return vb.Segment.build(k1, b, model["length"], model["g_payload"], term_key, term_start, doc[order].astype(np.uint32),
                            model["g_tf"][order])


def concat(a, b):
    """the growing CSR of a's documents followed by b's"""
    return dict(g_start=np.concatenate([a["g_start"], b["g_start"][1:] + a["g_start"][-1]]).astype(np.uint64),
                g_key=np.concatenate([np.asarray(a["g_key"]).reshape(-1), np.asarray(b["g_key"]).reshape(-1)]),
                g_tf=np.concatenate([a["g_tf"], b["g_tf"]]), g_fieldnorm=np.concatenate([a["g_fieldnorm"], b["g_fieldnorm"]]),
                g_payload=np.concatenate([np.asarray(a["g_payload"]).reshape(-1, 3), np.asarray(b["g_payload"]).reshape(-1, 3)]),
                g_deleted=np.concatenate([a["g_deleted"], b["g_deleted"]]))


def grid_stride_docs():
    """70 000 documents of 2 short lexemes: more than the 65 536 lanes of the intern grid, more waves than the wave kernel's grid and
    more workgroups than the workgroup kernel's"""
    n = 70_000
    return [[(b"w%d" % (i % 977), 1 + i % 3), (b"x%d" % (i % 31), 2)] for i in range(n)]


def grid_stride_docs_wide():
    """70 000 documents of 8 distinct short lexemes = 560 000 lexemes and 560 000 elements: more than the 2048 x 256 = 524 288 threads
    of one pass of the per-element kernels (the general class's over the lexemes, the build's over the elements), so their
    grid-stride loops take a second turn"""
    n = 70_000
    return [[(b"w%d" % ((i * 11 + j * 151) % 1201), 1 + (i + j) % 3) for j in range(8)] for i in range(n)]


_SHARED = {}


def shared(name, make):
    """a model computed once for the tests of one run that need it (the large batches); left unchanged by them"""
    if name not in _SHARED:
        _SHARED[name] = make()
    return _SHARED[name]


def grid_stride_model(wide):
    """(docs, payloads, the model's cast) of the grid-stride batches"""
    def make():
        docs = grid_stride_docs_wide() if wide else grid_stride_docs()
        pay = payloads(len(docs))
        return docs, pay, cast(docs, pay)
    return shared(("grid", wide), make)


def words(n, tag=b"w"):
    """n lexemes, every other one of the hashed kind (16 bytes or more)"""
    return [tag + (b"%d" % i if i % 2 else b"-a-lexeme-of-the-long-kind-%d" % i) for i in range(n)]


def corpus(lexemes, n_docs, seed, mean=8):
    """documents of (lexeme, count): Zipf-ish picks (repeats inside a document happen and are the dedup's business), counts 1 .. 3"""
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(len(lexemes)) + 1.0)
    p /= p.sum()
    out = []
    for _ in range(n_docs):
        n = int(rng.poisson(mean))
        out.append([(lexemes[j], int(c)) for j, c in zip(rng.choice(len(lexemes), n, p=p), rng.integers(1, 4, n))])
    return out


def same_records(a, b, what):
    """(hits, n_hits) of two searches: the records byte for byte"""
    assert np.array_equal(a[1], b[1]), f"{what}: counts differ"
    for q in range(len(a[1])):
        assert a[0][q, :a[1][q]].tobytes() == b[0][q, :b[1][q]].tobytes(), f"{what} q{q}: records differ"


def same_segment(got, want, what):
    """two host segments: meta() and every array of arrays()"""
    assert got.meta() == want.meta(), f"{what}: {got.meta()} != {want.meta()}"
    ga, wa = got.arrays(), want.arrays()
    assert sorted(ga) == sorted(wa)
    for name in wa:
        assert np.asarray(ga[name]).tobytes() == np.asarray(wa[name]).tobytes(), f"{what}: {name} differs"
