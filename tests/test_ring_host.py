"""The ring cursor without a device: csrc/ring.h, the first-in-first-out arithmetic that vbm25_stream, the resolver, the caster and
the reranker share, under AddressSanitizer + UBSan on the CPU against a std::deque of the slots in flight; and that the four units
keep no ring arithmetic of their own.  No GPU use."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
RING_UNITS = ("stream.hip", "resolve.hip", "cast.hip", "reranker.hip")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/ring_cursor.cpp built as tests/test_forward_host.py builds its harness: a stand-alone program, nothing of it is
    loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "ring_cursor")
    src = os.path.join(ROOT, "tests/native/ring_cursor.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", src, "-o", exe])
    return exe


def test_the_cursor_against_a_deque_under_asan(harness):
    """depths 1 .. 16, 4000 random pushes and pops each: tail() is the slot pushed, pop() the deque's front, full(), empty(), count and
    head agree with the deque after every step, and every depth's cursor has gone round at least 50 times at the end"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "64000 cases" in out.stdout and "fuzz done" in out.stdout and "FAIL" not in out.stdout


def test_the_header_is_plain_cxx():
    text = open(os.path.join(CSRC, "ring.h")).read()
    includes = re.findall(r"^#include\s+(\S+)", text, flags=re.M)
    assert includes == ["<cstdint>"] and "__device__" not in text and "__host__" not in text


@pytest.mark.parametrize("unit", RING_UNITS)
def test_a_ring_unit_has_no_arithmetic_of_its_own(unit):
    text = open(os.path.join(CSRC, unit)).read()
    assert '#include "ring.h"' in text and "RingCursor" in text
    assert not re.search(r"%\s*(\w+->)?depth\b", text) and not re.search(r"%\s*(uint32_t\()?\w+->slots\.size\(\)", text)
