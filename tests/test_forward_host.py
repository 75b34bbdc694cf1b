"""The forward index without a device: the per-lane functions of its sorts (csrc/forward_lane.h) under AddressSanitizer + UBSan on the
CPU, driven as a wave and as a workgroup drive them, against std::sort; the symbols, the tuning switches with their bounds and the
argument errors of the ABI that come before any device is touched.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, DEVICE = -1, -3

SYMBOLS = ("vbm25_index_bind", "vbm25_reranker_create_from_index")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_forward.cpp built as tests/test_tid_host.py builds its harness: a stand-alone program, nothing of it is
    loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_forward")
    src = os.path.join(ROOT, "tests/native/fuzz_forward.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src, "-o", exe])
    return exe


def test_the_sort_schedule_under_asan(harness):
    """runs of every length 0 .. 130 and of the class edges, five arrival orders each: the model wave (<= 64) and the model workgroup
    (<= 2048, its array exactly the network's size) against std::sort; run_class around both bounds, padded_len, slot_of, the walk"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "690 cases" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout


def test_symbols_are_declared_exported_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    mirror = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    L = C.CDLL(vb.library_path())
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(L, name) and name in ABI, name
        assert name + "(" in mirror, f"{name} is not used by include/vbm25.hpp"
    assert hasattr(vb.GpuIndex, "bind") and "from_index" in vb.DocTerms.reranker.__code__.co_varnames
    assert "DocTerms bind() const" in mirror and "FromIndex" in mirror
    # the hooks of the tests and of tools/forward_cost.py are exported and stay out of the header
    for name in ("vbm25_debug_forward", "vbm25_debug_doc_terms_fieldnorm"):
        assert hasattr(L, name) and name not in header and name not in ABI


def test_refusals_come_with_a_message():
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_index_bind(None, C.byref(out)) == INVALID and not out.value
    assert L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_index_bind(None, None) == INVALID and L.vbm25_last_error() == b"out is NULL"
    out = C.c_void_p(1)
    assert L.vbm25_reranker_create_from_index(None, None, 2, 4, 16, 64, 100, 10, C.byref(out)) == INVALID and not out.value
    assert L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_reranker_create_from_index(None, None, 2, 4, 16, 64, 100, 10, None) == INVALID and L.vbm25_last_error() == b"out is NULL"
    f = L.vbm25_debug_forward
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 4
    assert f(None, None, None, None) == INVALID and L.vbm25_last_error() == b"NULL argument"


def test_no_device_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = vb.lib()
    fake = C.create_string_buffer(4096)  # (never looked at: without a device there is no index)
    out = C.c_void_p(1)
    assert L.vbm25_index_bind(C.addressof(fake), C.byref(out)) == DEVICE and not out.value
    assert b"no HIP device" in L.vbm25_last_error() and b"no host fallback" in L.vbm25_last_error()


@pytest.mark.parametrize("name,bound", [("fwd_grid", 2048), ("fwd_wave_max", 64), ("fwd_group_max", 2048)])
def test_the_tuning_switches_and_their_bounds(name, bound):
    try:
        for value in (0, 1, bound - 1, bound):
            vb.set_tuning(name, value)
        for value in (-1, bound + 1, 1 << 40):
            with pytest.raises(vb.Vbm25Error, match=rf"{name} {value} is outside 0 \.\. {bound}") as e:
                vb.set_tuning(name, value)
            assert e.value.code == INVALID
        with pytest.raises(RuntimeError, match="unknown tuning switch"):
            vb.set_tuning("fwd_long_max", 1)
    finally:
        vb.reset_tuning()
