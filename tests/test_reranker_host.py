"""The reranker ring without a device: its ctid search (tid_find of csrc/tid_lane.h) under AddressSanitizer + UBSan on the CPU, its
symbols, and the argument errors of vbm25_reranker_create that come before any device is touched.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4

SYMBOLS = ("vbm25_reranker_create", "vbm25_reranker_free", "vbm25_reranker_device_bytes", "vbm25_reranker_info",
           "vbm25_reranker_submit_lexemes", "vbm25_reranker_submit_ids", "vbm25_reranker_collect", "vbm25_reranker_in_flight")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_tid_find.cpp built as tests/test_tid_host.py builds its harness: a stand-alone program, nothing of it is
    loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_tid_find")
    src = os.path.join(ROOT, "tests/native/fuzz_tid_find.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src, "-o", exe])
    return exe


def test_tid_find_under_asan(harness):
    """tid_find through the directory equals std::lower_bound + equality -- the first position of a key that repeats -- on sorted keys
    with duplicates, 0 .. 5000 of them, every directory size 0 .. 4, 2048 and 4096, keys below, between, equal to and above the set's"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "cases" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout


def test_symbols_are_declared_exported_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    mirror = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    L = C.CDLL(vb.library_path())
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(L, name) and name in ABI, name
        assert name + "(" in mirror, f"{name} is not used by include/vbm25.hpp"
    assert "typedef struct vbm25_reranker vbm25_reranker;" in header
    assert hasattr(vb, "Reranker") and hasattr(vb.DocTerms, "reranker") and "class Reranker" in mirror
    for attr in ("submit", "submit_ids", "collect", "in_flight", "device_bytes", "allocations", "close", "__enter__", "__exit__"):
        assert hasattr(vb.Reranker, attr), attr


def test_create_refuses_its_arguments_before_any_device():
    L = vb.lib()
    fake = C.c_void_p(8)  # (never dereferenced: NULL and depth are looked at first)
    out = C.c_void_p(1)
    assert L.vbm25_reranker_create(None, fake, None, 2, 4, 16, 64, 100, 10, C.byref(out)) == INVALID and not out.value
    assert L.vbm25_last_error() == b"NULL argument"
    out = C.c_void_p(1)
    assert L.vbm25_reranker_create(fake, None, None, 2, 4, 16, 64, 100, 10, C.byref(out)) == INVALID and not out.value
    assert L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_reranker_create(fake, fake, None, 2, 4, 16, 64, 100, 10, None) == INVALID and L.vbm25_last_error() == b"out is NULL"
    for depth in (0, 17, 1 << 20):
        out = C.c_void_p(1)
        assert L.vbm25_reranker_create(fake, fake, None, depth, 4, 16, 64, 100, 10, C.byref(out)) == INVALID and not out.value
        assert L.vbm25_last_error() == b"depth %d is outside 1 .. 16" % depth
    for caps in ((0, 16, 64, 100, 10), (4, 0, 64, 100, 10), (4, 16, 64, 0, 10), (4, 16, 64, 100, 0)):
        assert L.vbm25_reranker_create(fake, fake, None, 2, *caps, C.byref(out)) == INVALID
        assert L.vbm25_last_error() == b"max_queries, max_lexemes, max_candidates or max_k is 0"
    assert L.vbm25_reranker_create(fake, fake, None, 2, 4, 16, 64, 100, 1025, C.byref(out)) == UNSUPPORTED
    assert L.vbm25_last_error() == b"k is 1025: a scorer returns at most 1024 candidates a query"
    # the other entry points with a NULL handle
    assert L.vbm25_reranker_submit_lexemes(None, None, None, None, 0, None, None, None, 10) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_reranker_submit_ids(None, None, None, 0, None, None, None, 10) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_reranker_collect(None, None, None, None, None) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_reranker_info(None, None, None, None, None) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_reranker_device_bytes(None) == 0 and L.vbm25_reranker_in_flight(None) == 0
    L.vbm25_reranker_free(None)
