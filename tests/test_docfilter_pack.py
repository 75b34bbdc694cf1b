"""DocFilter's host side without a GPU: the bit packing of the bitmaps (uint64 words, ceil(n_docs / 64) per bitmap, bit d % 64 of
word d / 64 counted from the least significant bit) and the filtered-search symbols of include/vbm25.h in the ctypes table."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI


def _unpack_reference(words, n_docs):
    """bit d of bitmap i, read one document at a time"""
    return np.array([[(int(w[d // 64]) >> (d % 64)) & 1 for d in range(n_docs)] for w in words], dtype=bool)


@pytest.mark.parametrize("n_docs", [1, 63, 64, 65, 128, 1000, 4097])
def test_bool_array_packs_lsb_first(n_docs):
    rng = np.random.default_rng(n_docs)
    keep = rng.random((3, n_docs)) < 0.3
    words = vb.DocFilter.pack(keep, n_docs)
    assert words.dtype == np.uint64 and words.shape == (3, (n_docs + 63) // 64)
    assert np.array_equal(_unpack_reference(words, n_docs), keep)
    # nothing at or beyond n_docs
    if n_docs % 64:
        assert not (int(words[:, -1].max()) >> (n_docs % 64))


def test_single_bits_and_doc_id_lists():
    words = vb.DocFilter.pack([[0], [63], [64], [0, 1, 130]], 131)
    assert words.shape == (4, 3)
    assert words[0].tolist() == [1, 0, 0]
    assert words[1].tolist() == [1 << 63, 0, 0]
    assert words[2].tolist() == [0, 1, 0]
    assert words[3].tolist() == [3, 0, 1 << 2]
    # a 1-d bool array is one bitmap; a list of id arrays equals the bool form
    keep = np.zeros(131, dtype=bool)
    keep[[5, 77, 129]] = True
    assert np.array_equal(vb.DocFilter.pack(keep, 131), vb.DocFilter.pack([np.array([129, 5, 77])], 131))
    assert np.array_equal(vb.DocFilter.pack([[]], 131), np.zeros((1, 3), np.uint64))


def test_bad_shapes_and_ids_are_rejected():
    with pytest.raises(ValueError):
        vb.DocFilter.pack(np.ones((2, 10), dtype=bool), 11)
    with pytest.raises(ValueError):
        vb.DocFilter.pack([[10]], 10)
    with pytest.raises(ValueError):
        vb.DocFilter.pack([[-1]], 10)


def test_filter_symbols_are_bound():
    for name in ("vbm25_filter_create", "vbm25_filter_update", "vbm25_filter_device_words", "vbm25_filter_destroy",
                 "vbm25_search_batch_filtered", "vbm25_batch_set_filter"):
        assert name in ABI
        assert hasattr(vb.lib(), name)
    assert vb.NO_FILTER == 0xFFFFFFFF
