"""vbm25::DocTerms of include/vbm25.hpp (Documents::bind, evaluate) compiles against the C ABI and scores one batch bit for bit as the
Python mirror does: examples/evaluate_example.cpp prints its scores as hexadecimal floats."""
import os
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
SEED = bytes(range(7, 39))


def build_example(tmp_path):
    exe = str(tmp_path / "evaluate_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "evaluate_example.cpp"), "-L", CSRC, "-lvbm25",
                           f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_the_example_compiles_against_the_header(tmp_path):
    assert os.path.exists(build_example(tmp_path))


def lexeme(j):
    return b"t%d" % j if j % 3 else b"a-lexeme-of-the-long-kind-%d" % j


@pytest.mark.gpu
def test_cpp_mirror_scores_match_python(tmp_path):
    out = subprocess.check_output([build_example(tmp_path)], text=True, timeout=120)
    docs = [[(lexeme(j), 1 + (d * 7 + j) % 4) for j in range(12) if (d + j) % (2 + j % 3) == 0] for d in range(40)]
    pay = np.array([[0, d, 1] for d in range(41)], dtype=np.uint16)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(vb.Documents.cast(docs, pay[:40], seed=SEED), 1.2, 0.75))
    r = vb.Resolver(gix, 1, 8, 64, 4096, seed=SEED)
    rows = vb.Documents.cast(docs + [[(b"t1", 2), (b"not-in-the-index", 9)]], pay, seed=SEED)
    dt = rows.bind(r)
    assert f"bound {dt.n_docs} documents, {dt.n_known} of {rows.n_elements} elements known" in out
    r.submit([[b"t1", b"t2", b"unknown"], [lexeme(0), b"t4"], []])
    term_ids, q_off = r.collect()
    listed = dt.evaluate(term_ids, q_off, [0, 3, 5, 6], [40, 0, 7, 39, 39, 2])
    cross = dt.evaluate(term_ids, q_off).reshape(-1)
    assert (listed[:5] > 0).any() and listed[5] == 0 and (cross > 0).sum() > 20
    for tag, want in (("listed", listed), ("cross", cross)):
        got = [float.fromhex(l.split()[2]) for l in out.splitlines() if l.startswith(tag + " ")]
        assert len(got) == len(want)
        assert np.array_equal(np.array(got).view(np.uint64), want.view(np.uint64)), tag
    assert "candidate out of range: error -1" in out
