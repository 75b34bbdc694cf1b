"""vbm25_filter_remap without a GPU: the numpy model (tests/filter_remap_model.py) -- the concatenation of the kept bits -- against
the permutation through maintain_model.maintain's relabel array (a second, independent derivation), the kernel's word-level scheme
restated in Python against the concatenation over the shapes the device tests use, and the argument checks that come before any
device call."""
import ctypes as C

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus
from filter_remap_model import (compress64, deletion_patterns, pack_bits, remap_bits, remap_by_relabel, remap_word_scheme, remap_words,
                                unpack_bits)
from growing_data import make_growing
from maintain_model import maintain


@pytest.mark.parametrize("dele", [0.0, 0.01, 0.5, "range"])
@pytest.mark.parametrize("grow", [0, 3000])
def test_concatenation_equals_the_permutation_through_relabel(dele, grow):
    """the lognormal corpus of tests/test_gpu_maintain.py, growing documents from make_growing"""
    c = make_corpus(20_000, 600, seed=1, length="lognormal", mean_len=40)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    n = seg.n_docs
    rng = np.random.default_rng(5)
    deleted = deletion_patterns(n, rng)["range"] if dele == "range" else rng.random(n) < dele
    G = make_growing(seg.arrays()["term_key"], grow, seed=8, deleted=0.1)[0] if grow else None
    args, relabel = maintain(seg.arrays(), seg.meta(), deleted, G)
    n_new = len(args[2])
    F = 3
    bits_s = rng.random((F, n)) < 0.5
    bits_g = rng.random((F, grow)) < 0.5 if grow else None
    want = remap_by_relabel(bits_s, bits_g, relabel, n_new)
    got = remap_words(bits_s, deleted, bits_g, G["g_deleted"] if grow else None)
    assert got.shape == (F, (n_new + 63) // 64) and np.array_equal(got, want)
    assert np.array_equal(unpack_bits(got, n_new), remap_bits(bits_s, deleted, bits_g, G["g_deleted"] if grow else None))


def test_compress64():
    rng = np.random.default_rng(0)
    for m in [0, 1, 1 << 63, (1 << 64) - 1, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555, 0xFFFFFFFF00000000] + \
            [int(x) for x in rng.integers(0, 1 << 63, 50, dtype=np.uint64) * 2 + rng.integers(0, 2, 50, dtype=np.uint64)]:
        x = int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))
        want = sum(((x >> b) & 1) << i for i, b in enumerate(b for b in range(64) if (m >> b) & 1))
        assert compress64(x, m) == want, hex(m)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 1000, 4097])
def test_word_scheme_equals_the_concatenation(n):
    """the kernel's scheme, word by word, over every deletion pattern x growing count x growing delete rate"""
    rng = np.random.default_rng(n)
    F = 2
    for name, deleted in deletion_patterns(n, rng).items():
        for g in (0, 1, 63, 64, 65, 300):
            for grate in (0.0, 0.1, 1.0):
                bits_s = rng.random((F, n)) < 0.5
                bits_g = rng.random((F, g)) < 0.5
                gdel = (rng.random(g) < grate).astype(np.uint8)
                want = remap_words(bits_s, deleted, bits_g if g else None, gdel if g else None)
                got = remap_word_scheme(pack_bits(bits_s), n, deleted, pack_bits(bits_g), g, gdel)
                assert got.shape == want.shape and np.array_equal(got, want), (n, name, g, grate)


def test_argument_errors_without_a_device():
    """NULL handles: VBM25_ERR_INVALID before any device call, *out NULL afterwards"""
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_filter_remap(None, None, 0, None, None, C.byref(out)) == -1
    assert out.value is None
    assert L.vbm25_filter_remap(None, None, 0, None, None, None) == -1
    assert b"out" in L.vbm25_last_error()
    words = np.zeros(1, np.uint64)
    assert L.vbm25_filter_read(None, 0, 0, words.ctypes.data) == -1
    out = C.c_void_p(1)
    devs = (C.c_int * 1)(0)
    assert L.vbm25_multi_create_from_device(None, devs, 1, C.byref(out)) == -1
    assert out.value is None
    assert b"segment" in L.vbm25_last_error()
