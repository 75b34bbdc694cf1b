"""The document cast without a device: its per-document functions (csrc/cast_lane.h) under AddressSanitizer + UBSan on the CPU, the
argument refusals of vbm25_documents_cast message for message, and the no-device code of the three new entry points.  No GPU use."""
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
    """tests/native/fuzz_cast.cpp built as tests/test_resolve_host.py builds its harness: a stand-alone program, nothing of it is
    loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_cast")
    src = os.path.join(ROOT, "tests/native/fuzz_cast.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src, "-o", exe])
    return exe


def test_lane_functions_under_asan(harness):
    """merge_document against std::sort + a loop (the issue's key-order and saturation cases and 4000 random documents with long runs
    of equal keys), key_less / key_equal against memcmp, fieldnorm_of against a linear search, doc_class at its edges"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "fuzz done" in out.stdout and "FAIL" not in out.stdout


def test_symbols_are_declared_exported_and_wrapped():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    L = C.CDLL(vb.library_path())
    for name in ("vbm25_documents_cast", "vbm25_documents_info", "vbm25_documents_download", "vbm25_documents_device_bytes",
                 "vbm25_documents_free", "vbm25_device_segment_build_documents", "vbm25_device_growing_append_documents"):
        assert name + "(" in header and hasattr(L, name), name
    assert hasattr(vb, "Documents") and hasattr(vb, "pack_documents")
    assert hasattr(vb.DeviceSegment, "from_documents") and hasattr(vb.GrowingSegment, "append_documents")


def _cast(seed, data, lex_off, lex_count, doc_lex, n_docs, payload=None, out="byref"):
    L = vb.lib()
    h = C.c_void_p(1)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = L.vbm25_documents_cast(0, seed, p(data), p(lex_off), p(lex_count), p(doc_lex), n_docs, p(payload), C.byref(h) if out == "byref" else None)
    return rc, h.value, L.vbm25_last_error().decode()


def test_cast_refusals_come_before_the_device_message_for_message():
    data = np.frombuffer(b"abc" + b"x" * 17 + b"d\0e", dtype=np.uint8)
    lex_off = np.array([0, 3, 20, 23], dtype=np.uint64)
    count = np.array([1, 2, 3], dtype=np.uint32)
    doc_lex = np.array([0, 2, 2, 3], dtype=np.uint32)
    seed = bytes(32)
    assert _cast(seed, data, lex_off, count, doc_lex, 3, out=None)[0] == -1
    for args in ((data, None, count, doc_lex), (data, lex_off, None, doc_lex), (data, lex_off, count, None), (None, lex_off, count, doc_lex)):
        rc, h, msg = _cast(seed, *args, 3)
        assert (rc, h, msg) == (-1, None, "NULL argument"), args
    rc, h, msg = _cast(seed, data, lex_off, count, np.array([1, 2, 2, 3], dtype=np.uint32), 3)
    assert (rc, h, msg) == (-1, None, "doc_lex[0] is 1, not 0")
    rc, h, msg = _cast(seed, data, lex_off, count, np.array([0, 2, 1, 3], dtype=np.uint32), 3)
    assert (rc, h, msg) == (-1, None, "doc_lex is not monotone at document 1")
    rc, h, msg = _cast(seed, data, np.array([0, 3, 2, 23], dtype=np.uint64), count, doc_lex, 3)
    assert (rc, h, msg) == (-1, None, "lex_off is not monotone at lexeme 1")
    # a lexeme without positions: the first one is named (the reference panics there)
    rc, h, msg = _cast(seed, data, lex_off, np.array([1, 0, 0], dtype=np.uint32), doc_lex, 3)
    assert (rc, h, msg) == (-1, None, "lexeme 1 (document 0) has count 0")
    rc, h, msg = _cast(seed, data, lex_off, np.array([1, 1, 0], dtype=np.uint32), doc_lex, 3)
    assert (rc, h, msg) == (-1, None, "lexeme 2 (document 2) has count 0")
    # a lexeme that needs the hash without a seed: the resolver's and vbm25_intern's words
    rc, h, msg = _cast(None, data, lex_off, count, doc_lex, 3)
    assert (rc, h) == (-1, None) and msg == "a lexeme of 16 bytes or more needs the index's seed (Meta tuple)"
    with pytest.raises(vb.Vbm25Error) as e:
        vb.intern(b"x" * 17)
    assert msg in str(e.value)
    rc, h, msg = _cast(None, data[20:], np.array([0, 3], dtype=np.uint64), count[:1], np.array([0, 1], dtype=np.uint32), 1)  # the NUL inside
    assert (rc, h) == (-1, None) and "needs the index's seed" in msg
    # 2^31 lexemes: refused from doc_lex alone, before a lexeme array is read
    rc, h, msg = _cast(seed, data, lex_off, count, np.array([0, 1 << 31], dtype=np.uint32), 1)
    assert (rc, h) == (-4, None) and "fewer than 2^31" in msg  # VBM25_ERR_UNSUPPORTED


def test_tuning_switches_bounds():
    try:
        vb.set_tuning("cast_wave_max", 0)
        vb.set_tuning("cast_wave_max", 64)
        vb.set_tuning("cast_group_max", 0)
        vb.set_tuning("cast_group_max", 2048)
        for name, value in (("cast_wave_max", 65), ("cast_group_max", 2049), ("cast_wave_max", -1)):
            with pytest.raises(vb.Vbm25Error, match="outside 0"):
                vb.set_tuning(name, value)
    finally:
        vb.reset_tuning()


def test_pack_documents():
    data, lex_off, lex_count, doc_lex = vb.pack_documents([[(b"ab", 2), (b"", 1)], [], [(b"cde", 7)]])
    assert data.tobytes() == b"abcde" and lex_off.tolist() == [0, 2, 2, 5] and lex_count.tolist() == [2, 1, 7] and doc_lex.tolist() == [0, 2, 2, 3]
    assert (lex_off.dtype, lex_count.dtype, doc_lex.dtype) == (np.uint64, np.uint32, np.uint32)


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(vb.Vbm25Error) as e:
        vb.Documents.cast([[(b"abc", 1)], []])
    assert e.value.code == -3  # VBM25_ERR_DEVICE: there is no host cast behind the entry point
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_device_segment_build_documents(None, 1.2, 0.75, C.byref(out)) == -3 and not out.value
    assert L.vbm25_device_growing_append_documents(None, None) == -3
    # handles nobody has: a status, never a crash
    assert L.vbm25_documents_info(None, None, None, None) == -1 and L.vbm25_documents_device_bytes(None) == 0
    assert L.vbm25_documents_download(None, C.byref(out), None) == -1
    L.vbm25_documents_free(None)
