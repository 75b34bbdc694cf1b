"""DocTerms::append, Reranker::sync and their neighbours of include/vbm25.hpp compile against the C ABI and give, over three rounds of
appends to an index-bound handle, the reranked rows of the Python mirror (DocTerms.append_documents, Reranker.sync):
examples/live_rerank_example.cpp prints them, the scores as hexadecimal floats."""
import os
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
SEED = bytes(range(7, 39))
CUTS = (40, 41, 50, 70)


def build_example(tmp_path):
    exe = str(tmp_path / "live_rerank_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "live_rerank_example.cpp"), "-L", CSRC, "-lvbm25",
                           f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_the_example_uses_the_new_calls_and_compiles(tmp_path):
    src = open(os.path.join(ROOT, "examples", "live_rerank_example.cpp")).read()
    for call in (".bind()", "vbm25::from_index", "bound.append(delta, resolver)", "growing->append(delta)", "ring.sync()", ".submit_tids(",
                 ".directory_docs()", ".base_docs()"):
        assert call in src, call
    mirror = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    for name in ("vbm25_doc_terms_append_documents(", "vbm25_doc_terms_append(", "vbm25_doc_terms_base_docs(", "vbm25_reranker_sync(",
                 "vbm25_reranker_directory_docs("):
        assert name in mirror, name
    assert os.path.exists(build_example(tmp_path))


def lexeme(j):
    return b"t%d" % j if j % 3 else b"a-lexeme-of-the-long-kind-%d" % j


def rows(first, end):
    docs = [[(lexeme(j), 1 + (d * 7 + j) % 4) for j in range(12) if (d + j) % (2 + j % 3) == 0] for d in range(first, end)]
    return vb.Documents.cast(docs, np.array([[0, d, 1] for d in range(first, end)], dtype=np.uint16), seed=SEED)


@pytest.mark.gpu
def test_cpp_rows_of_the_new_documents_match_python(tmp_path):
    out = subprocess.check_output([build_example(tmp_path)], text=True, timeout=120)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(rows(0, 40), 1.2, 0.75))
    res = vb.Resolver(gix, 1, 8, 64, 4096, seed=SEED)
    dt = gix.bind()
    queries = [[b"t1", b"t2", b"unknown"], [lexeme(0), b"t4"]]
    found_new = False
    with dt.reranker(res, 2, 8, 64, 4096, 1024, 16, from_index=True) as ring:
        gs = None
        for rnd in range(3):
            first, end = CUTS[rnd], CUTS[rnd + 1]
            delta = rows(first, end)
            if gs is None:
                gs = vb.GrowingSegment.from_dict(gix, delta.download())
            else:
                gs.append_documents(delta)
            dt.append_documents(delta, res)
            ring.sync()
            assert f"round {rnd}: {end} documents, 40 sealed, {end - 40} growing, directory {end}" in out
            assert (dt.n_docs, dt.base_docs, gs.n_docs, ring.directory_docs) == (end, 40, end - 40, end)
            tids = np.array([[0, d, 1] for d in range(first, end)] + [[9, 9, 9], [0, 7, 1]], dtype=np.uint16)
            n = len(tids)
            ring.submit(queries, 4, [0, n, 2 * n], cand_tid=np.concatenate([tids, tids]))
            ranks, n_ranks = ring.collect()
            got = [l.split()[2:] for l in out.splitlines() if l.startswith(f"row {rnd} ")]
            assert len(got) == 8 and (n_ranks == min(4, n - 1)).all()
            for q, i, nr, pos, doc, score in got:
                q, i = int(q), int(i)
                assert int(nr) == n_ranks[q] and int(pos) == ranks["pos"][q, i] and int(doc) == ranks["doc"][q, i], (rnd, q, i)
                assert np.float64(float.fromhex(score)).view(np.uint64) == ranks["score"][q, i].view(np.uint64), (rnd, q, i)
            found_new |= bool((ranks["doc"][:, :n_ranks.min()] >= first).any())
            assert n - 2 not in ranks["pos"][0, :n_ranks[0]].tolist()  # (the ctid nobody carries)
    assert found_new
