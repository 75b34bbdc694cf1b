"""The growing segment's k > 1024 route without a device: the per-entry functions of its merge and of the host's cuts
(csrc/growing_bigk_lane.h) under AddressSanitizer + UBSan on the CPU.  No GPU use."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_positions_and_cuts_under_asan(tmp_path):
    """the positions growing_bigk_merge_kernel gives sealed records and growing survivors equal std::merge (sealed first on equal
    scores) over sorted lists with ties, tiles at their edges; capacity, chunk and item cuts equal brute force; a stand-alone
    program, nothing of it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_growing_bigk")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests/native/fuzz_growing_bigk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "420 cases, 0 failures" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout
