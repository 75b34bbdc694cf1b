"""The rerank step without a device: the per-entry functions of its top-k selection (csrc/rerank_lane.h) under AddressSanitizer + UBSan
on the CPU, its symbols, its tuning switches and the argument errors of its ABI.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("vbm25_scorer_create", "vbm25_scorer_free", "vbm25_scorer_device_bytes", "vbm25_scorer_evaluate", "vbm25_scorer_topk")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_rerank.cpp built as tests/test_evaluate_documents_host.py builds its harness: a stand-alone program, nothing
    of it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_rerank")
    src = os.path.join(ROOT, "tests/native/fuzz_rerank.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src,
                           "-o", exe])
    return exe


def test_selection_functions_under_asan(harness):
    """a model workgroup -- four waves in shuffled order, 64 offers a wave, buffers of 2k allocated exactly, k from 1 to 1024, heavy
    ties, parts merged -- equals std::stable_sort cut at k on 200 seeded cases; the key order is the doubles' order and a strict weak
    order with equal scores and pos = 0 and 2^32 - 1"""
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
    assert "typedef struct vbm25_scorer vbm25_scorer;" in header
    assert "typedef struct vbm25_rank { double score; uint32_t pos; uint32_t doc; } vbm25_rank;" in header
    assert vb.RANK_DTYPE.itemsize == 16 and vb.RANK_DTYPE.names == ("score", "pos", "doc")
    assert [vb.RANK_DTYPE.fields[n][1] for n in vb.RANK_DTYPE.names] == [0, 8, 12]
    assert hasattr(vb, "Scorer") and hasattr(vb.DocTerms, "scorer")
    for attr in ("evaluate", "topk", "device_bytes", "close", "__enter__", "__exit__"):
        assert hasattr(vb.Scorer, attr), attr
    assert "class Scorer" in mirror and "DocTerms::scorer" in mirror


def test_null_arguments_are_refused_with_a_message():
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_scorer_create(None, C.byref(out)) == -1 and not out.value
    assert b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_scorer_create(None, None) == -1
    assert b"out is NULL" in L.vbm25_last_error()
    assert L.vbm25_scorer_device_bytes(None) == 0
    L.vbm25_scorer_free(None)
    assert L.vbm25_scorer_evaluate(None, None, None, 0, None, None, None) == -1
    assert b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_scorer_topk(None, None, None, 3, None, None, 10, None, None) == -1
    assert b"NULL argument" in L.vbm25_last_error()


def test_rerank_part_and_rerank_buf_are_tuning_switches():
    try:
        for value in (1, 64, 100, 1000, 1 << 30):  # (clamped to 64 .. 2^20, in 64s)
            vb.set_tuning("rerank_part", value)
        for value in (0, 2, 3, 8, 1000):  # (clamped to 2 .. 8)
            vb.set_tuning("rerank_buf", value)
        with pytest.raises(RuntimeError, match="unknown tuning switch"):
            vb.set_tuning("rerank_k", 1)
    finally:
        vb.reset_tuning()
