"""The dense k > 1024 route without a device: the per-lane functions of its threshold search (csrc/bigk_dense_lane.h) under
AddressSanitizer + UBSan on the CPU.  No GPU use."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_threshold_search_under_asan(tmp_path):
    """histogram -> walk -> next interval over (key, doc) sets equals std::nth_element: the clip bin, tie masses down to the last of
    the nine levels, fewer than and exactly k entries, above + bin at the capacity and one past it; a stand-alone program, nothing
    of it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_bigk_dense")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests/native/fuzz_bigk_dense.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "127 cases, most levels 9" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout
