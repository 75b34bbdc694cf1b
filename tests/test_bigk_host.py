"""The sparse k > 1024 path without a device: the per-entry functions of its select and tile rank (csrc/bigk_lane.h) under
AddressSanitizer + UBSan on the CPU.  No GPU use."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_and_tile_rank_under_asan(tmp_path):
    """a model workgroup's select (digit walk, boundary count, compaction) and the tile sort with merge-by-rank equal
    std::nth_element + std::sort on the strict order: all-equal keys (the doc digits decide), counts at the tile edges, k at, below
    and above the number of candidates; a stand-alone program, nothing of it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_bigk")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests/native/fuzz_bigk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "1920 cases" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout

