"""vbm25::TidSet, DocFilter::set_tids and DeviceGrowing::erase(const TidSet &) of include/vbm25.hpp compile against the C ABI and give
the words the Python mirror gives: examples/bulkdelete_example.cpp prints the match words of a small table and a filter made from
them."""
import os
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
N_SEALED, N_GROW = 150, 70


def build_example(tmp_path):
    exe = str(tmp_path / "bulkdelete_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "bulkdelete_example.cpp"), "-L", CSRC, "-lvbm25",
                           f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_the_example_uses_the_tid_set_and_compiles(tmp_path):
    src = open(os.path.join(ROOT, "examples", "bulkdelete_example.cpp")).read()
    assert "vbm25::TidSet" in src and ".set_tids(" in src and ".erase(set)" in src and ".match(" in src
    assert os.path.exists(build_example(tmp_path))


def ctid(r):
    return (0, r // 7, r % 7 + 1)


def document(r):
    return [(b"t%d" % ((r * 3 + j) % 11), 1 + j) for j in range(1 + r % 4)]


def hex_words(words):
    return [f"{int(w):016x}" for w in words]


@pytest.mark.gpu
def test_cpp_words_match_python(tmp_path):
    out = subprocess.check_output([build_example(tmp_path)], text=True, timeout=120)
    lines = {}
    for line in out.splitlines():
        for name in ("filter 0 sealed", "filter 0 growing", "filter 1 sealed", "filter 1 growing", "sealed", "growing"):
            if line.startswith(name + " ") or line == name:
                lines[name] = line[len(name):].split()
                break
    rows = range(N_SEALED + N_GROW)
    pay = np.array([ctid(r) for r in rows], np.uint16)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(vb.Documents.cast([document(r) for r in range(N_SEALED)], pay[:N_SEALED]), 1.2, 0.75))
    G = vb.Documents.cast([document(r) for r in range(N_SEALED, N_SEALED + N_GROW)], pay[N_SEALED:]).download()
    grow = vb.GrowingSegment(gix, G["g_start"], G["g_key"], G["g_tf"], G["g_fieldnorm"], G["g_payload"])
    dead = [r for r in range(N_SEALED + N_GROW + 20) if r % 5 == 0 or r >= N_SEALED + N_GROW]
    with vb.TidSet(np.array([ctid(r) for r in dead[::-1]] * 2, np.uint16)) as ts:
        assert f"set {len(dead)} distinct of {2 * len(dead)}, device 0, bytes ok" in out
        first, last = ts.read()[0], ts.read()[-1]
        assert f"first {first[0]} {first[1]} {first[2]} last {last[0]} {last[1]} {last[2]}" in out
        ws, ns = ts.match(gix)
        wg, ng = ts.match_growing(grow)
        # the Python mirror's words are numpy's
        keep = np.array([r % 5 == 0 for r in rows])
        assert np.array_equal(ws, vb.DocFilter.pack(keep[:N_SEALED], N_SEALED)[0]) and ns == int(keep[:N_SEALED].sum())
        assert np.array_equal(wg, vb.DocFilter.pack(keep[N_SEALED:], N_GROW)[0]) and ng == int(keep[N_SEALED:].sum())
        assert lines["sealed"] == hex_words(ws) and lines["growing"] == hex_words(wg)
        assert f"matched {ns} sealed {ng} growing" in out and f"deleted by TID: {ng} matched" in out
        f = vb.DocFilter(gix, np.zeros((2, N_SEALED), bool))
        f.set_growing(grow)
        f.set_tids(0, ts, False, grow)
        f.set_tids(1, ts, True, grow)
        for i in (0, 1):
            assert lines[f"filter {i} sealed"] == hex_words(f.read(i))
            assert lines[f"filter {i} growing"] == hex_words(f.read(i, growing=True))
        assert lines["filter 1 sealed"] == hex_words(vb.DocFilter.pack(~keep[:N_SEALED], N_SEALED)[0])
    assert "refused: " in out and "bitmap 2 of a filter of 2" in out
