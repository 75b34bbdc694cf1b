"""The evaluate operator on bound documents without a device: its per-lane functions (csrc/evaluate_lane.h) under AddressSanitizer +
UBSan on the CPU, its symbols, and the argument errors of its ABI.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("vbm25_documents_bind", "vbm25_doc_terms_info", "vbm25_doc_terms_download", "vbm25_doc_terms_device_bytes",
           "vbm25_doc_terms_free", "vbm25_evaluate_documents")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_evaluate.cpp built as tests/test_resolve_host.py builds its harness: a stand-alone program, nothing of it
    is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_evaluate")
    src = os.path.join(ROOT, "tests/native/fuzz_evaluate.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src,
                           "-o", exe])
    return exe


def test_lane_functions_under_asan(harness):
    """bisect_run equal to std::lower_bound, with its found flag, on exactly allocated runs of every power of two up to 4096, each
    +- 1, and 5000 ids -- probes below, on, between and above the ids, on the whole run and on sub-ranges (empty ones too; an empty
    run is a NULL array) -- and pair_score bit for bit a merge walk's sum for queries of 0 .. 300 ids, ids the index lacks among
    them, against documents of 0 .. 600 known elements that sit between two neighbours"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "fuzz done" in out.stdout and "FAIL" not in out.stdout


def test_symbols_are_declared_exported_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    mirror = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    L = C.CDLL(vb.library_path())
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(L, name) and name in ABI, name
        assert name + "(" in mirror, f"{name} is not used by include/vbm25.hpp"
    assert "typedef struct vbm25_doc_terms vbm25_doc_terms;" in header
    assert hasattr(vb, "DocTerms") and hasattr(vb.Documents, "bind")
    for attr in ("evaluate", "download", "device_bytes"):
        assert hasattr(vb.DocTerms, attr), attr
    assert "class DocTerms" in mirror and "Documents::bind" in mirror


def test_null_arguments_are_refused_with_a_message():
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_documents_bind(None, None, C.byref(out)) == -1 and not out.value
    assert b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_documents_bind(None, None, None) == -1
    assert b"out is NULL" in L.vbm25_last_error()
    assert L.vbm25_doc_terms_info(None, None, None, None) == -1
    assert b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_doc_terms_download(None, None, None, None) == -1
    assert b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_doc_terms_device_bytes(None) == 0
    L.vbm25_doc_terms_free(None)
    assert L.vbm25_evaluate_documents(None, None, None, 0, None, None, None) == -1
    assert b"NULL argument" in L.vbm25_last_error()
    assert L.vbm25_evaluate_documents(None, None, None, 3, None, None, None) == -1
    assert b"NULL argument" in L.vbm25_last_error()


def test_eval_grid_is_a_tuning_switch():
    try:
        vb.set_tuning("eval_grid", 1)
        vb.set_tuning("eval_grid", 3)
        vb.set_tuning("eval_grid", 1 << 20)  # (clamped to the built-in grid)
        with pytest.raises(RuntimeError, match="unknown tuning switch"):
            vb.set_tuning("eval_route", 1)  # (one route was built: no switch to force another)
    finally:
        vb.reset_tuning()
