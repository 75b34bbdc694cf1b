"""The query resolver without a device: its per-lexeme and per-key functions (csrc/resolve_lane.h) under AddressSanitizer + UBSan on
the CPU, and the argument errors of its ABI.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_resolve.cpp built as tests/test_pages_device_host.py builds its harness: a stand-alone program, nothing of
    it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_resolve")
    src = [os.path.join(ROOT, p) for p in ("tests/native/fuzz_resolve.cpp", "vectorchord-bm25_amd/csrc/blake3.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", *src, "-o", exe])
    return exe


def test_lane_functions_under_asan(harness):
    """intern_lane byte for byte vbm25_intern's (published vectors, every length 0 .. 130, the chunk and tree edges up to 8193 bytes,
    every start alignment in exactly allocated pools through both loaders, NULs, hash byte 15 == 0, random lexemes) and lookup_lane
    equal to std::lower_bound (0, 1, 2 and 1000 keys; byte 7 / 8 / 15, signed and byte order traps, probes outside the vocabulary)"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "fuzz done" in out.stdout and "FAIL" not in out.stdout


def test_resolver_symbols_are_declared_exported_and_wrapped():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    L = C.CDLL(vb.library_path())
    for name in ("vbm25_resolver_create", "vbm25_resolver_destroy", "vbm25_resolver_device_bytes", "vbm25_resolver_submit_lexemes",
                 "vbm25_resolver_submit_keys", "vbm25_resolver_collect", "vbm25_resolver_in_flight", "vbm25_intern_batch_device",
                 "vbm25_search_batch_lexemes"):
        assert name + "(" in header and hasattr(L, name), name
    assert hasattr(vb, "Resolver") and hasattr(vb, "intern_batch") and hasattr(vb, "search_batch_lexemes")


def test_create_with_a_null_index_is_refused_with_a_message():
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_resolver_create(None, None, 2, 16, 64, 1024, C.byref(out)) == -1 and not out.value
    assert b"index is NULL" in L.vbm25_last_error()
    assert L.vbm25_resolver_create(None, None, 2, 16, 64, 1024, None) == -1
    # the other entry points with nothing to work on: a status, never a crash
    assert L.vbm25_resolver_submit_lexemes(None, None, None, None, 0) == -1
    assert L.vbm25_resolver_submit_keys(None, None, None, 0) == -1
    assert L.vbm25_resolver_collect(None, None, None, None) == -1
    assert L.vbm25_resolver_in_flight(None) == 0 and L.vbm25_resolver_device_bytes(None) == 0
    L.vbm25_resolver_destroy(None)
    assert L.vbm25_search_batch_lexemes(None, None, None, None, None, 0, 10, None, None) == -1


def test_intern_batch_argument_errors_come_before_the_device():
    lex_off = np.array([0, 3, 20], dtype=np.uint64)
    data = np.frombuffer(b"abc" + b"x" * 17, dtype=np.uint8)
    keys = np.zeros(32, dtype=np.uint8)
    L = vb.lib()
    assert L.vbm25_intern_batch_device(0, None, data.ctypes.data, None, 2, keys.ctypes.data) == -1
    assert L.vbm25_intern_batch_device(0, None, data.ctypes.data, lex_off.ctypes.data, 2, None) == -1
    # a lexeme of 16 bytes or more without a seed: vbm25_intern's words
    assert L.vbm25_intern_batch_device(0, None, data.ctypes.data, lex_off.ctypes.data, 2, keys.ctypes.data) == -1
    with pytest.raises(vb.Vbm25Error) as e:
        vb.intern(b"x" * 17)
    assert L.vbm25_last_error().decode() in str(e.value) and "needs the index's seed" in str(e.value)
    # ... and a NUL inside a short one
    with pytest.raises(vb.Vbm25Error, match="needs the index's seed"):
        vb.intern_batch([b"ab", b"c\0d"], None)
    # offsets that go backwards
    bad = np.array([0, 5, 3], dtype=np.uint64)
    assert L.vbm25_intern_batch_device(0, bytes(32), data.ctypes.data, bad.ctypes.data, 2, keys.ctypes.data) == -1
    assert b"not monotone" in L.vbm25_last_error()


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(vb.Vbm25Error) as e:
        vb.intern_batch([b"abc", b"x" * 40], bytes(range(32)))
    assert e.value.code == -3  # VBM25_ERR_DEVICE: vbm25_intern is another entry point, not a fallback
    with pytest.raises(vb.Vbm25Error) as e:
        vb.intern_batch([b"abc"], None)
    assert e.value.code == -3
