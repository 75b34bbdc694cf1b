"""vbm25::Reranker of include/vbm25.hpp compiles against the C ABI and reranks three batches in flight -- document indices, ctids, the
cross product -- row for row as the Python mirror's Reranker and as Scorer.topk do: examples/rerank_ring_example.cpp prints its top-3
rows with the scores as hexadecimal floats."""
import os
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
SEED = bytes(range(7, 39))


def build_example(tmp_path):
    exe = str(tmp_path / "rerank_ring_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "rerank_ring_example.cpp"), "-L", CSRC, "-lvbm25",
                           f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_the_example_uses_the_reranker_and_compiles(tmp_path):
    src = open(os.path.join(ROOT, "examples", "rerank_ring_example.cpp")).read()
    assert "vbm25::Reranker" in src and ".submit_tids(" in src and ".collect(" in src
    assert os.path.exists(build_example(tmp_path))


def lexeme(j):
    return b"t%d" % j if j % 3 else b"a-lexeme-of-the-long-kind-%d" % j


@pytest.mark.gpu
def test_cpp_reranker_rows_match_python(tmp_path):
    out = subprocess.check_output([build_example(tmp_path)], text=True, timeout=120)
    docs = [[(lexeme(j), 1 + (d * 7 + j) % 4) for j in range(12) if (d + j) % (2 + j % 3) == 0] for d in range(40)]
    pay = np.array([[0, d, 1] for d in range(40)] + [[0, 7, 1]], dtype=np.uint16)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(vb.Documents.cast(docs, pay[:40], seed=SEED), 1.2, 0.75))
    r = vb.Resolver(gix, 1, 8, 64, 4096, seed=SEED)
    rows = vb.Documents.cast(docs + [[(b"t1", 2), (b"not-in-the-index", 9)]], pay, seed=SEED)
    dt = rows.bind(r)
    queries = [[b"t1", b"t2", b"unknown"], [lexeme(0), b"t4"], []]
    r.submit(queries)
    term_ids, q_off = r.collect()
    tids = np.array([[0, 7, 1], [0, 0, 1], [9, 9, 9], [0, 39, 1], [0, 39, 1], [0, 2, 1], [0, 2, 1]], dtype=np.uint16)
    assert "in flight 3" in out and "allocations unchanged" in out and "empty ring: error -1" in out
    with dt.scorer() as s, dt.reranker(r, 3, 8, 64, 4096, 1024, 16, documents=rows) as ring:
        ring.submit(queries, 3, [0, 3, 5, 6], [40, 0, 7, 39, 39, 2])
        ring.submit(queries, 3, [0, 4, 6, 7], cand_tid=tids)
        ring.submit(queries, 3)
        listed, by_tid, cross = ring.collect(), ring.collect(), ring.collect()
        for got, args in ((listed, ([0, 3, 5, 6], [40, 0, 7, 39, 39, 2])), (cross, ())):
            want = s.topk(term_ids, q_off, 3, *args)
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
        # the ctids: (0, 7, 1) is documents 7 and 40 -> 7; (9, 9, 9) is no document and keeps its position
        want = s.topk(term_ids, q_off, 3, [0, 3, 5, 6], [7, 0, 39, 39, 2, 2])
        assert by_tid[1].tolist() == want[1].tolist() == [3, 2, 1]
        assert np.array_equal(by_tid[0]["doc"], want[0]["doc"]) and by_tid[0]["score"].tobytes() == want[0]["score"].tobytes()
        assert 2 not in by_tid[0]["pos"][0].tolist() and sorted(by_tid[0]["pos"][0].tolist()) == [0, 1, 3]
    for tag, (ranks, n_ranks) in (("ring listed", listed), ("ring tids", by_tid), ("ring cross", cross)):
        got = [l.split()[2:] for l in out.splitlines() if l.startswith(tag + " ")]
        assert len(got) == 9
        for q, i, n, pos, doc, score in got:
            q, i = int(q), int(i)
            assert int(n) == n_ranks[q] and int(pos) == ranks["pos"][q, i] and int(doc) == ranks["doc"][q, i], (tag, q, i)
            assert np.float64(float.fromhex(score)).view(np.uint64) == ranks["score"][q, i].view(np.uint64), (tag, q, i)
    assert (listed[0]["score"][:2] > 0).any() and cross[1].tolist() == [3, 3, 3]
