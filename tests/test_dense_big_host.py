"""The survivor list of scan_dense_kernel<1024> without a device: its per-lane functions (csrc/dense_list_lane.h) under
AddressSanitizer + UBSan on the CPU.  No GPU use."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_functions_under_asan(tmp_path):
    """eight model waves append to a buffer of exactly CAP entries and cut it with the kernel's schedule (local stages wave after wave):
    equal to std::partial_sort on "score descending, doc ascending" on 160 seeded cases, k from 257 to 1024, runs of ties, rising
    scores that overflow the buffer (given up, nothing written past it).  A stand-alone program: nothing of it is loaded here."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_dense_big")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests/native/fuzz_dense_big.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "160 cases" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout

