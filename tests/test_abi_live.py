"""The entry points of the live table on the ring and the multi-GPU batch (vbm25_stream_set_growing / _set_filter / _submit_filtered,
vbm25_filter_extend_growing, vbm25_multi_batch_set_growing / _set_filter) are declared, exported and bound, and answer NULL handles
with VBM25_ERR_INVALID before any device is touched (no GPU use)."""
import ctypes

import numpy as np

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI

from test_abi import declared_functions

INVALID = -1
NEW = ["vbm25_stream_set_growing", "vbm25_stream_set_filter", "vbm25_stream_submit_filtered", "vbm25_filter_extend_growing",
       "vbm25_multi_batch_set_growing", "vbm25_multi_batch_set_filter"]


def test_declared_exported_and_bound():
    declared = declared_functions()
    raw = ctypes.CDLL(vb.library_path())
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/vbm25.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in ABI, f"{name} has no ctypes binding"
        assert getattr(vb.lib(), name).argtypes == ABI[name][1]


def test_null_handles_are_invalid_arguments():
    L = vb.lib()
    sel = np.zeros(4, np.uint32)
    off = np.arange(5, dtype=np.uint32)
    words = np.zeros(4, np.uint64)
    ptrs = (ctypes.c_void_p * 2)(None, None)
    assert L.vbm25_stream_set_growing(None, None) == INVALID
    assert b"NULL" in L.vbm25_last_error()
    assert L.vbm25_stream_set_filter(None, None) == INVALID
    assert L.vbm25_stream_submit_filtered(None, sel.ctypes.data, sel.ctypes.data, off.ctypes.data, 4) == INVALID
    assert L.vbm25_filter_extend_growing(None, None, words.ctypes.data) == INVALID
    assert L.vbm25_filter_extend_growing(None, None, None) == INVALID
    assert L.vbm25_multi_batch_set_growing(None, ptrs) == INVALID
    assert L.vbm25_multi_batch_set_growing(None, None) == INVALID
    assert L.vbm25_multi_batch_set_filter(None, ptrs, sel.ctypes.data) == INVALID
    assert L.vbm25_multi_batch_set_filter(None, None, None) == INVALID
    assert L.vbm25_stream_in_flight(None) == 0


def test_python_mirrors_exist():
    for cls, names in ((vb.Stream, ("set_growing", "set_filter", "submit")), (vb.DocFilter, ("extend_growing",)),
                       (vb.MultiBatch, ("set_growing", "set_filter")), (vb.MultiIndex, ("index",))):
        for n in names:
            assert callable(getattr(cls, n)), f"{cls.__name__}.{n}"
