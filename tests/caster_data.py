"""Batches for the caster's tests (tests/test_gpu_caster.py): documents of given sizes, the packing edges, the lexemes of the in-lane
intern at every pool alignment, and the raw submit through ctypes."""
import ctypes as C

import numpy as np

import vectorchord_bm25_amd as vb


def lex(i, hashed=None):
    """lexeme number i: short (the key is the bytes) or long (hashed)"""
    if hashed is None:
        hashed = i % 3 == 0
    return (b"a-long-lexeme-number-%09d" % i) if hashed else (b"t%d" % i)


def docs_of(sizes, pool=40, seed=1):
    """one document per size, its lexemes drawn from `pool` distinct ones: they repeat inside a document and across neighbours"""
    rng = np.random.default_rng(seed)
    return [[(lex(int(i)), int(c)) for i, c in zip(rng.integers(0, pool, n), rng.integers(1, 6, n))] for n in sizes]


# runs of consecutive short documents around the 64 lexemes and the 64 documents of one packed wave
PACKING = {
    "sum 63": [20, 20, 23, 5],
    "sum 64": [20, 20, 24, 5],
    "sum 65": [20, 20, 25, 5],
    "64 ones then one": [1] * 65,
    "64 empty": [0] * 64,
    "65 empty": [0] * 65,
    "empty first and last in a wave": [0, 30, 34, 0, 0, 7, 0],
    "64 between ones": [1, 64, 1],
    "a group-class document splits a run": [5, 5, 65, 5, 5],
    "no documents": [],
    "one empty document": [0],
    "mixed": [3, 0, 0, 61, 1, 2, 64, 0, 17, 17, 17, 13, 1, 63, 2],
}
WAVE_MAX_8 = [3, 8, 9, 2, 8, 1, 1, 0, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, 70, 4, 4]  # (the class edge moves inside a wave)


def intern_docs():
    """lexemes of 15, 16, 17, 1024, 1025 and 8193 bytes, plain and with a NUL inside, each at every pool alignment 0 .. 3 (a filler
    lexeme in front shifts it), in documents of two or three lexemes: an all-wave-class batch"""
    docs, at = [], 0
    for n in (15, 16, 17, 1024, 1025, 8193, 3):
        for nul in (False, True):
            for align in range(4):
                body = bytearray((7 + 13 * j + n) % 255 + 1 for j in range(n))
                if nul:
                    body[n // 2] = 0
                fill = b"f" * ((align - at) % 4)
                doc = [(fill, 1), (bytes(body), 2)] if fill else [(b"", 3), (bytes(body), 2)]
                at += len(fill) + n
                assert (at - n) % 4 == align
                docs.append(doc + [(bytes(body), 5)] * (align == 3))  # (a repeat: the second copy sits at another alignment)
                at += n * (align == 3)
    return docs


def raw_submit(caster, data, lex_off, lex_count, doc_lex, n_docs, payload=None):
    """vbm25_caster_submit with the arrays as given (None: NULL) -> (code, message)"""
    L = vb.lib()
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = L.vbm25_caster_submit(caster.h, p(data), p(lex_off), p(lex_count), p(doc_lex), n_docs, p(payload))
    return rc, L.vbm25_last_error().decode() if rc else ""


def raw_collect(caster):
    L = vb.lib()
    out = C.c_void_p(1)
    rc = L.vbm25_caster_collect(caster.h, C.byref(out))
    return rc, out.value, L.vbm25_last_error().decode() if rc else ""


# what vbm25_debug_caster_launched reports of the last collected batch
INTERN, WAVE, PACK, PACK_FUSED = 1, 2, 4, 8


def launched(caster):
    """the kernels the last collected batch's lexemes and wave class went through, as a mask of the four above"""
    L = vb.lib()
    L.vbm25_debug_caster_launched.argtypes = [C.c_void_p, C.c_void_p]
    mask = C.c_uint32()
    assert L.vbm25_debug_caster_launched(caster.h, C.byref(mask)) == 0
    return mask.value
