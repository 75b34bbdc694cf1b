"""The caster without a device: the packing functions of csrc/cast_lane.h (the host's plan, the lane's document, the segmented
rank-and-merge) under AddressSanitizer + UBSan on the CPU, the new symbols, their no-device codes and the bounds of the two new
tuning switches.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vbm25_caster_create", "vbm25_caster_free", "vbm25_caster_device_bytes", "vbm25_caster_info", "vbm25_caster_submit",
           "vbm25_caster_collect", "vbm25_caster_in_flight", "vbm25_documents_extend")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_cast_pack.cpp built as tests/test_cast_host.py builds its harness: a stand-alone program, nothing of it is
    loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_cast_pack")
    src = os.path.join(ROOT, "tests/native/fuzz_cast_pack.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src, "-o", exe])
    return exe


def test_packing_functions_under_asan(harness):
    """the plan against a restatement and its properties (at most 64 lexemes and 64 documents an entry, every wave-class document
    exactly once and in order, no document of another class); the segmented merge lane by lane against merge_document per document on
    the GPU tests' runs, keys in adjacent documents, saturation beside a count of 1, keys that differ in byte 15 only, and a few
    thousand random packed waves"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "fuzz done" in out.stdout and "FAIL" not in out.stdout


def test_symbols_are_declared_exported_and_wrapped():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    L = C.CDLL(vb.library_path())
    from vectorchord_bm25_amd._lib import ABI
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(L, name) and name in ABI, name
    assert hasattr(vb, "Caster") and hasattr(vb.Documents, "extend") and hasattr(vb.Documents, "empty")
    for method in ("submit", "collect", "in_flight", "device_bytes", "allocations"):
        assert hasattr(vb.Caster, method), method
    hpp = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    assert "class Caster" in hpp and "extend(" in hpp


def test_null_handles_give_a_status_never_a_crash():
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_caster_submit(None, None, None, None, None, 0, None) == -1
    assert L.vbm25_caster_collect(None, C.byref(out)) == -1 and not out.value
    assert L.vbm25_caster_collect(None, None) == -1
    assert L.vbm25_caster_info(None, None, None, None) == -1
    assert L.vbm25_caster_in_flight(None) == 0 and L.vbm25_caster_device_bytes(None) == 0
    L.vbm25_caster_free(None)
    assert L.vbm25_documents_extend(None, None) == -1 and L.vbm25_last_error() == b"NULL argument"
    # arguments refused before a device is looked for
    for depth in (0, 17):
        assert L.vbm25_caster_create(0, None, depth, 1, 1, 1, 0, C.byref(out)) == -1 and b"outside 1 .. 16" in L.vbm25_last_error()
        assert not out.value
    assert L.vbm25_caster_create(0, None, 1, 0, 1, 1, 0, C.byref(out)) == -1
    assert L.vbm25_caster_create(0, None, 1, 1, 1, 1, 2, C.byref(out)) == -1 and b"max_long_lexemes" in L.vbm25_last_error()
    assert L.vbm25_caster_create(0, None, 1, 1, 1, 1, 0, None) == -1


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_caster_create(0, None, 2, 16, 64, 1024, 0, C.byref(out)) == -3 and not out.value  # VBM25_ERR_DEVICE
    with pytest.raises(vb.Vbm25Error) as e:
        vb.Caster(0, 2, 16, 64, 1024)
    assert e.value.code == -3
    with pytest.raises(vb.Vbm25Error) as e:
        vb.Documents.empty()
    assert e.value.code == -3


def test_tuning_switches_bounds():
    try:
        for value in (0, 1, 2):
            vb.set_tuning("cast_pack", value)
        for value in (3, -1):
            with pytest.raises(vb.Vbm25Error, match="outside 0 .. 2"):
                vb.set_tuning("cast_pack", value)
        vb.set_tuning("cast_grid", 0)
        vb.set_tuning("cast_grid", 3)
        with pytest.raises(vb.Vbm25Error, match="outside 0"):
            vb.set_tuning("cast_grid", -1)
    finally:
        vb.reset_tuning()
