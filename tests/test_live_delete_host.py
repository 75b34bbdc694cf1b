"""Deletes on a bound handle without a device: the walk to a ctid's lowest live document and a model wave's word across the base / tail
split (csrc/tid_lane.h) under AddressSanitizer + UBSan on the CPU, the new symbols, and the NULL-argument refusals that come before
any device is touched.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

SYMBOLS = ("vbm25_doc_terms_delete", "vbm25_doc_terms_delete_tids", "vbm25_doc_terms_dead_docs", "vbm25_doc_terms_read_dead")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_live_dead.cpp built as tests/test_live_rerank_host.py builds its harness: a stand-alone program, nothing of
    it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_live_dead")
    src = os.path.join(ROOT, "tests/native/fuzz_live_dead.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src, "-o", exe])
    return exe


def test_the_walk_and_the_word_under_asan(harness):
    """tid_find + tid_first_live against a linear scan for the lowest live document -- runs of 1 .. 5 equal keys, every dead pattern
    of a run, directories of 1 .. 4, 2048 and 4096 entries -- and a model wave's words across the base / tail split against a loop
    over the bits, at base_docs 0, 1, 59, 64, 70, 300 with tails of 0, 1, 58, 59, 200"""
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
    for attr in ("delete", "delete_tids", "dead_docs", "read_dead"):
        assert hasattr(vb.DocTerms, attr), attr
    for text in ("uint32_t erase(const uint32_t *docs, uint64_t n)", "uint32_t erase(const TidSet &tids, const Documents *payloads = nullptr)",
                 "uint32_t dead_docs() const", "std::vector<uint64_t> read_dead() const"):
        assert text in mirror, text
    lane = open(os.path.join(ROOT, "vectorchord-bm25_amd", "csrc", "tid_lane.h")).read()
    assert "tid_first_live(" in lane and "split_payload(" in lane


def test_null_arguments_are_refused_before_any_device():
    L = vb.lib()
    fake = C.c_void_p(8)  # (never dereferenced: NULL is looked at first)
    n_new = C.c_uint32(7)
    assert L.vbm25_doc_terms_delete(None, fake, 1, C.byref(n_new)) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_doc_terms_delete(None, None, 0, None) == INVALID and L.vbm25_last_error() == b"NULL argument"
    for args in ((None, fake, None, C.byref(n_new)), (fake, None, None, C.byref(n_new)), (None, None, fake, None)):
        assert L.vbm25_doc_terms_delete_tids(*args) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_doc_terms_read_dead(None, fake) == INVALID and L.vbm25_last_error() == b"NULL argument"
    assert L.vbm25_doc_terms_dead_docs(None) == 0
    assert n_new.value == 7  # (a refused call writes nothing)
