"""TID sets without a device: the per-document functions of the match (csrc/tid_lane.h) under AddressSanitizer + UBSan on the CPU,
the symbols, the tuning switches and the argument errors of the ABI.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, DEVICE, UNSUPPORTED = -1, -3, -4

SYMBOLS = ("vbm25_tid_set_create", "vbm25_tid_set_info", "vbm25_tid_set_read", "vbm25_tid_set_device_bytes", "vbm25_tid_set_free",
           "vbm25_tid_set_match_index", "vbm25_tid_set_match_growing", "vbm25_filter_set_tids", "vbm25_device_growing_delete_tids",
           "vbm25_device_vacuum_bulkdelete")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_tid.cpp built as tests/test_rerank_host.py builds its harness: a stand-alone program, nothing of it is
    loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_tid")
    src = os.path.join(ROOT, "tests/native/fuzz_tid.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src, "-o", exe])
    return exe


def test_search_and_word_assembly_under_asan(harness):
    """tid_contains through the directory equals std::binary_search on 200 seeded sets (sizes 0, 1, 2, directory - 1, directory,
    directory + 1, strides that do not divide the size, every tid_dir from 0 up; members, members +- 1 in each field, keys 0 and
    2^48 - 1, keys that differ in one field only), and a model wave's words (tail bits, invert, OR and new-count) equal a plain loop"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "200 cases" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout


def test_symbols_are_declared_exported_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    mirror = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    L = C.CDLL(vb.library_path())
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(L, name) and name in ABI, name
        assert name + "(" in mirror, f"{name} is not used by include/vbm25.hpp"
    assert "typedef struct vbm25_tid_set vbm25_tid_set;" in header
    assert hasattr(vb, "TidSet")
    for attr in ("match", "match_growing", "read", "device_bytes", "close", "__enter__", "__exit__"):
        assert hasattr(vb.TidSet, attr), attr
    assert hasattr(vb.DocFilter, "set_tids") and hasattr(vb.GrowingSegment, "delete_tids") and hasattr(vb.DeviceVacuum, "bulkdelete")
    assert "class TidSet" in mirror and "set_tids" in mirror and "erase(const TidSet &" in mirror and "bulkdelete" in mirror
    # the packing of the keys: most significant field first
    assert vb.TidSet.keys([[1, 2, 3], [0xffff, 0xffff, 0xffff]]).tolist() == [(1 << 32) | (2 << 16) | 3, (1 << 48) - 1]


def test_refusals_come_with_a_message():
    L = vb.lib()
    tids = np.zeros(3, dtype=np.uint16)
    out = C.c_void_p(1)
    # n > 2^32 - 1: refused before tids is read (one TID is all this buffer holds) or anything is allocated
    assert L.vbm25_tid_set_create(0, tids.ctypes.data, 1 << 32, C.byref(out)) == UNSUPPORTED and not out.value
    assert b"at most 2^32 - 1" in L.vbm25_last_error()
    out = C.c_void_p(1)
    assert L.vbm25_tid_set_create(0, None, 1 << 40, C.byref(out)) == UNSUPPORTED and not out.value
    assert L.vbm25_tid_set_create(0, tids.ctypes.data, 1, None) == INVALID
    assert b"out is NULL" in L.vbm25_last_error()
    out = C.c_void_p(1)
    assert L.vbm25_tid_set_create(0, None, 1, C.byref(out)) == INVALID and not out.value
    assert b"tids is NULL" in L.vbm25_last_error()
    assert L.vbm25_tid_set_info(None, None, None) == INVALID and b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_tid_set_read(None, None) == INVALID and b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_tid_set_device_bytes(None) == 0
    L.vbm25_tid_set_free(None)
    assert L.vbm25_tid_set_match_index(None, None, None, None) == INVALID and b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_tid_set_match_growing(None, None, None, None) == INVALID and b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_filter_set_tids(None, 0, None, 0, None) == INVALID and b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_device_growing_delete_tids(None, None, None) == INVALID and b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_device_vacuum_bulkdelete(None, None, None, None, None) == INVALID and b"NULL argument" in L.vbm25_last_error()


def test_no_device_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = vb.lib()
    tids = np.zeros(3, dtype=np.uint16)
    for n, ptr in ((1, tids.ctypes.data), (0, None)):   # the empty set lives on the device too
        out = C.c_void_p(1)
        assert L.vbm25_tid_set_create(0, ptr, n, C.byref(out)) == DEVICE and not out.value
        assert b"no HIP device" in L.vbm25_last_error()
    with pytest.raises(vb.Vbm25Error) as e:
        vb.TidSet(np.zeros((4, 3), np.uint16))
    assert e.value.code == DEVICE


def test_tid_grid_and_tid_dir_are_tuning_switches():
    try:
        for value in (-5, 0, 1, 3, 2048, 1 << 30):  # (clamped to 1 .. 2048)
            vb.set_tuning("tid_grid", value)
        for value in (-1, 0, 2, 12, 13, 1000):  # (clamped to 0 .. 12: 4096 entries, 32 KB of LDS)
            vb.set_tuning("tid_dir", value)
        with pytest.raises(RuntimeError, match="unknown tuning switch"):
            vb.set_tuning("tid_stride", 1)
    finally:
        vb.reset_tuning()
