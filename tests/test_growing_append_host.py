"""vbm25_device_growing_append / _delete / _docs without a device: argument errors come back as a status and a message before any
GPU call, and the Python mirror has the methods."""
import ctypes as C

import numpy as np

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd.api import GrowingDesc

INVALID = -1


def _message():
    lib = vb.lib()
    lib.vbm25_last_error.restype = C.c_char_p
    return lib.vbm25_last_error().decode()


def test_null_arguments_are_refused_without_touching_a_device():
    lib = vb.lib()
    d = GrowingDesc()
    assert lib.vbm25_device_growing_append(None, C.byref(d)) == INVALID
    assert "NULL" in _message()
    fake = C.c_void_p(0)  # (a NULL segment with a NULL delta)
    assert lib.vbm25_device_growing_append(fake, None) == INVALID
    assert "NULL" in _message()
    g = np.array([0, 1], np.uint32)
    assert lib.vbm25_device_growing_delete(None, g.ctypes.data_as(C.c_void_p), 2) == INVALID
    assert "NULL" in _message()
    assert lib.vbm25_device_growing_delete(None, None, 0) == INVALID


def test_docs_of_null_is_zero():
    assert vb.lib().vbm25_device_growing_docs(None) == 0


def test_python_mirror_has_the_methods():
    assert callable(vb.GrowingSegment.append) and callable(vb.GrowingSegment.delete)
