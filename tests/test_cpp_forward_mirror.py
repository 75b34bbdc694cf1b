"""Index::bind and the from_index constructor of vbm25::Reranker of include/vbm25.hpp compile against the C ABI and give, on an index
whose documents are gone, the forward index and the reranked rows of the Python mirror (GpuIndex.bind, DocTerms.reranker(...,
from_index=True)): examples/forward_example.cpp prints both, the scores as hexadecimal floats."""
import os
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
SEED = bytes(range(7, 39))


def build_example(tmp_path):
    exe = str(tmp_path / "forward_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "forward_example.cpp"), "-L", CSRC, "-lvbm25",
                           f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_the_example_uses_the_bind_and_compiles(tmp_path):
    src = open(os.path.join(ROOT, "examples", "forward_example.cpp")).read()
    assert "->bind()" in src and "vbm25::from_index" in src and ".submit_tids(" in src and ".collect(" in src
    mirror = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    assert "vbm25_index_bind(" in mirror and "vbm25_reranker_create_from_index(" in mirror
    assert os.path.exists(build_example(tmp_path))


def lexeme(j):
    return b"t%d" % j if j % 3 else b"a-lexeme-of-the-long-kind-%d" % j


@pytest.mark.gpu
def test_cpp_forward_index_and_rows_match_python(tmp_path):
    out = subprocess.check_output([build_example(tmp_path)], text=True, timeout=120)
    docs = [[(lexeme(j), 1 + (d * 7 + j) % 4) for j in range(12) if (d + j) % (2 + j % 3) == 0] for d in range(40)]
    pay = np.array([[0, d, 1] for d in range(40)], dtype=np.uint16)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(vb.Documents.cast(docs, pay, seed=SEED), 1.2, 0.75))
    r = vb.Resolver(gix, 1, 8, 64, 4096, seed=SEED)
    dt = gix.bind()
    start, term, tf = dt.download()
    assert f"forward 40 documents {dt.n_known} postings" in out and "documents-bound handle: error -1" in out
    lines = [l for l in out.splitlines() if l.startswith("doc ")]
    assert len(lines) == 40
    for d, line in enumerate(lines):
        want = " ".join(f"{t}:{f}" for t, f in zip(term[int(start[d]):int(start[d + 1])], tf[int(start[d]):int(start[d + 1])]))
        assert line == f"doc {d}:" + (" " + want if want else ""), d
    queries = [[b"t1", b"t2", b"unknown"], [lexeme(0), b"t4"], []]
    tids = np.array([[0, 7, 1], [0, 0, 1], [9, 9, 9], [0, 39, 1], [0, 39, 1], [0, 2, 1], [0, 2, 1]], dtype=np.uint16)
    with dt.reranker(r, 2, 8, 64, 4096, 1024, 16, from_index=True) as ring:
        ring.submit(queries, 3, [0, 4, 6, 7], cand_tid=tids)
        ring.submit(queries, 3)
        by_tid, cross = ring.collect(), ring.collect()
    assert by_tid[1].tolist() == [3, 2, 1] and sorted(by_tid[0]["pos"][0].tolist()) == [0, 1, 3] and cross[1].tolist() == [3, 3, 3]
    for tag, (ranks, n_ranks) in (("ring tids", by_tid), ("ring cross", cross)):
        got = [l.split()[2:] for l in out.splitlines() if l.startswith(tag + " ")]
        assert len(got) == 9
        for q, i, n, pos, doc, score in got:
            q, i = int(q), int(i)
            assert int(n) == n_ranks[q] and int(pos) == ranks["pos"][q, i] and int(doc) == ranks["doc"][q, i], (tag, q, i)
            assert np.float64(float.fromhex(score)).view(np.uint64) == ranks["score"][q, i].view(np.uint64), (tag, q, i)
    assert (cross[0]["score"][:2] > 0).any()
