"""The tiles of scan_sparse_big_kernel without a device: its per-lane functions (csrc/sparse_big_lane.h) under AddressSanitizer +
UBSan on the CPU.  No GPU use."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_functions_under_asan(tmp_path):
    """200 seeded items of random sorted runs walked tile by tile as the workgroup walks them -- chunk assignment with head and tail
    masks, slot from prefix and word, tile halving -- against a std::map accumulation.  A stand-alone program: nothing of it is
    loaded here."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_sparse_big")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests/native/fuzz_sparse_big.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "200 cases" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout
