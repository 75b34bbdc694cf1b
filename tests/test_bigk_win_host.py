"""bigk_scan_win_kernel without a device: the per-lane functions of its tiles and of its single-field decode (csrc/bigk_win_lane.h)
under AddressSanitizer + UBSan on the CPU.  No GPU use."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("g", [1, 2, 4])
def test_tiles_and_field_decode_under_asan(tmp_path, g):
    """a model workgroup's tiles (the multi-window plan, the window of a posting, chunk masks, slots) equal a std::map accumulation,
    and field_at a bit-by-bit extraction over both packings and every width, at every compile-time tile span; a stand-alone program,
    nothing of it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_bigk_win")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           f"-DVBM25_BIGK_WIN_G={g}", os.path.join(ROOT, "tests/native/fuzz_bigk_win.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "200 cases" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout
