"""vbm25::Caster and Documents::extend of include/vbm25.hpp compile against the C ABI and give, chunk by chunk through a ring of two
slots, the arrays the Python mirror's one-shot cast gives: examples/caster_example.cpp prints the extended handle document by
document."""
import os
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
SEED = bytes(range(7, 39))


def build_example(tmp_path):
    exe = str(tmp_path / "caster_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "caster_example.cpp"), "-L", CSRC, "-lvbm25",
                           f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_the_example_uses_the_caster_and_compiles(tmp_path):
    src = open(os.path.join(ROOT, "examples", "caster_example.cpp")).read()
    assert "vbm25::Caster" in src and ".collect()" in src and ".extend(" in src and "Documents::empty" in src
    assert os.path.exists(build_example(tmp_path))


def lexeme(j):
    return b"t%d" % j if j % 3 else b"a-lexeme-of-the-long-kind-%d" % j


def document(d):
    doc = [(lexeme((d * 5 + j * 2) % 9), 1 + (d + j) % 3) for j in range(d % 7)]
    if d % 2 and d % 7:
        doc.append((lexeme((d * 5) % 9), 4))
    return doc


@pytest.mark.gpu
def test_cpp_caster_chunks_match_python(tmp_path):
    out = subprocess.check_output([build_example(tmp_path)], text=True, timeout=120)
    docs = [document(d) for d in range(100)]
    pay = np.array([[0, d, 1] for d in range(100)], dtype=np.uint16)
    want = vb.Documents.cast(docs, pay, seed=SEED).download()
    assert "caster allocations unchanged, device bytes unchanged" in out
    assert f"extended 100 documents {len(want['g_tf'])} elements: equal" in out
    assert "refused: dst and src are the same handle" in out
    chunks = [l.split() for l in out.splitlines() if l.startswith("chunk ")]
    assert [int(c[2]) for c in chunks] == [0, 1, 64, 35] and [int(c[6]) for c in chunks] == [1, 1, 1, 0]
    rows = [l.split() for l in out.splitlines() if l.startswith("doc ")]
    assert len(rows) == 100
    start, key = want["g_start"].astype(np.int64), np.asarray(want["g_key"]).reshape(-1, 16)
    for d, row in enumerate(rows):
        assert (int(row[1]), int(row[2]), int(row[3])) == (d, want["g_fieldnorm"][d], want["length"][d])
        got = [(bytes.fromhex(e.split(":")[0]), int(e.split(":")[1])) for e in row[4:]]
        assert got == [(key[e].tobytes(), int(want["g_tf"][e])) for e in range(start[d], start[d + 1])], d
