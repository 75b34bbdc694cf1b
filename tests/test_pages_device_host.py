"""The device reader without a device: its per-tuple functions (csrc/pages_parse.h) under AddressSanitizer on the CPU, and the ABI of
vbm25_device_segment_from_pages.  No GPU use."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import pages_device_data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_functions_under_asan(tmp_path):
    """tests/native/fuzz_pages_device.cpp: the host pass and the kernels' (page, slot) grid as plain loops over csrc/pages_parse.h,
    output arrays sized exactly as the device allocates them, built with AddressSanitizer + UBSan (the build line of
    test_page_reader_under_asan).  First the 40 damaged relations tests/test_gpu_pages_device.py reads on the GPU, then 4000 more: every
    one accepted or refused as vbm25_segment_from_pages does, equal arrays when accepted, no out-of-bounds access."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    base = D.damage_relation()
    cases = D.random_damage(len(base), 40, seed=0)
    outcomes = [D.host_outcome(D.apply_edits(base, e))[0] for e in cases]
    assert any(outcomes) and not all(outcomes)   # seed 0 gives both classes
    case_file = str(tmp_path / "cases.bin")
    with open(case_file, "wb") as f:
        f.write(struct.pack("<I", len(base)))
        for p in base:
            f.write(p.tobytes())
        f.write(struct.pack("<I", len(cases)))
        for edits in cases:
            f.write(struct.pack("<I", len(edits)))
            for e in edits:
                f.write(struct.pack("<III", *e))
    exe = str(tmp_path / "fuzz_pages_device")
    src = [os.path.join(ROOT, p) for p in ("tests/native/fuzz_pages_device.cpp", "vectorchord-bm25_amd/csrc/pages.cpp",
                                           "vectorchord-bm25_amd/csrc/segment.cpp", "vectorchord-bm25_amd/csrc/blake3.cpp", "oracle/oracle.cpp",
                                           "oracle/pages.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-pthread", *src, "-o", exe])
    out = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert f"case file done: {sum(outcomes)} flattened, {len(outcomes) - sum(outcomes)} rejected" in out.stdout
    assert "fuzz done" in out.stdout


def test_named_damage_belongs_in_the_list():
    """every named case of the GPU test is refused by the host reader with VBM25_ERR_CORRUPT (checked here where no GPU is needed)"""
    c, seg, oix, pages = D.relation(n_docs=800, vocab=100)
    pl = [p.copy() for p in D.page_list(pages)]
    for name, edit in D.named_damage(pl):
        cp = [p.copy() for p in pl]
        edit(cp)
        ok, code = D.host_outcome(cp)
        assert not ok and code == -2, name
    ok, seg0 = D.host_outcome(D.empty_relation())
    assert ok and seg0.n_docs == 0


def test_symbol_is_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    assert "int vbm25_device_segment_from_pages(vbm25_read_page_fn read_page, void *ctx, int device," in header
    assert hasattr(C.CDLL(vb.library_path()), "vbm25_device_segment_from_pages")
    assert hasattr(vb.DeviceSegment, "from_pages")


def test_null_arguments_are_invalid():
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_device_segment_from_pages(None, None, 0, C.byref(out)) == -1 and not out.value
    cb = vb.api.READ_PAGE_FN(lambda ctx, i: None)
    assert L.vbm25_device_segment_from_pages(C.cast(cb, C.c_void_p), None, 0, None) == -1


def test_no_host_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c, seg, oix, pages = D.relation(n_docs=800, vocab=100)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.DeviceSegment.from_pages(D.page_list(pages))
    assert e.value.code == -3  # VBM25_ERR_DEVICE: the host reader is another entry point, not a fallback
