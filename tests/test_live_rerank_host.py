"""The rerank stack on a live table without a device: the rank functions of vbm25_reranker_sync's merge and the LDS sort's network
(csrc/tid_lane.h) under AddressSanitizer + UBSan on the CPU, the new symbols, and the NULL-argument refusals that come before any
device is touched.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

SYMBOLS = ("vbm25_doc_terms_append_documents", "vbm25_doc_terms_append", "vbm25_doc_terms_base_docs", "vbm25_reranker_sync",
           "vbm25_reranker_directory_docs")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_live_merge.cpp built as tests/test_reranker_host.py builds its harness: a stand-alone program, nothing of it
    is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_live_merge")
    src = os.path.join(ROOT, "tests/native/fuzz_live_merge.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src, "-o", exe])
    return exe


def test_merge_by_rank_under_asan(harness):
    """every old entry to i + #{delta keys < key}, every new one to j + #{old keys <= key} through the old directory: std::merge on
    (key, doc) with every position written once -- old sets of 0 .. 5000 keys with duplicates, deltas of 0 .. 300 keys below, between,
    equal to and above them, directories of 0 .. 4, 2048 and 4096 entries; the delta sorted by the LDS network; the new directory
    against dir_shape + dir_source"""
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
    for attr in ("append_documents", "append", "base_docs"):
        assert hasattr(vb.DocTerms, attr), attr
    for attr in ("sync", "directory_docs"):
        assert hasattr(vb.Reranker, attr), attr
    for text in ("void append(const Documents &delta, const Resolver &resolver)", "void append(const GrowingDocs &delta, const Resolver &resolver)",
                 "void sync()"):
        assert text in mirror, text
    makefile = open(os.path.join(ROOT, "vectorchord-bm25_amd", "csrc", "Makefile")).read()
    assert " live.o " in makefile and os.path.exists(os.path.join(ROOT, "vectorchord-bm25_amd", "csrc", "live.hip"))


def test_null_arguments_are_refused_before_any_device():
    L = vb.lib()
    fake = C.c_void_p(8)  # (never dereferenced: NULL is looked at first)
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert L.vbm25_doc_terms_append_documents(*args) == INVALID and L.vbm25_last_error() == b"NULL argument"
        assert L.vbm25_doc_terms_append(*args) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_reranker_sync(None) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_doc_terms_base_docs(None) == 0 and L.vbm25_reranker_directory_docs(None) == 0


def test_live_sort_max_is_a_tuning_switch_with_bounds():
    try:
        for value in (0, 1, 64, 4096):
            vb.set_tuning("live_sort_max", value)
        for value in (-1, 4097):
            with pytest.raises(vb.Vbm25Error, match=rf"live_sort_max {value} is outside 0 .. 4096") as e:
                vb.set_tuning("live_sort_max", value)
            assert e.value.code == INVALID
    finally:
        vb.reset_tuning()
