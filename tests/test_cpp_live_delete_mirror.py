"""DocTerms::erase, dead_docs and read_dead of include/vbm25.hpp compile against the C ABI and give, over a delete, a reused ctid and a
sync on an index-bound handle, the reranked rows of the Python mirror (DocTerms.delete_tids, delete, dead_docs, read_dead):
examples/live_delete_example.cpp prints them, the scores as hexadecimal floats."""
import os
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorchord-bm25_amd", "csrc")
SEED = bytes(range(7, 39))
VICTIM = 7


def build_example(tmp_path):
    exe = str(tmp_path / "live_delete_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "live_delete_example.cpp"), "-L", CSRC, "-lvbm25",
                           f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_the_example_uses_the_new_calls_and_compiles(tmp_path):
    src = open(os.path.join(ROOT, "examples", "live_delete_example.cpp")).read()
    for call in (".bind()", "vbm25::from_index", "bound.erase(gone)", "bound.erase(again, 2)", "bound.append(delta, resolver)", "ring.sync()",
                 ".submit_tids(", ".dead_docs()", ".read_dead()"):
        assert call in src, call
    mirror = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    for name in ("vbm25_doc_terms_delete(", "vbm25_doc_terms_delete_tids(", "vbm25_doc_terms_dead_docs(", "vbm25_doc_terms_read_dead("):
        assert name in mirror, name
    assert os.path.exists(build_example(tmp_path))


def lexeme(j):
    return b"t%d" % j if j % 3 else b"a-lexeme-of-the-long-kind-%d" % j


def rows(first, end, at):
    docs = [[(lexeme(j), 1 + (d * 7 + j) % 4) for j in range(12) if (d + j) % (2 + j % 3) == 0] for d in range(first, end)]
    return vb.Documents.cast(docs, np.array([[0, at + d - first, 1] for d in range(first, end)], dtype=np.uint16), seed=SEED)


@pytest.mark.gpu
def test_cpp_rows_of_each_step_match_python(tmp_path):
    out = subprocess.check_output([build_example(tmp_path)], text=True, timeout=120)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(rows(0, 40, 0), 1.2, 0.75))
    res = vb.Resolver(gix, 1, 8, 64, 4096, seed=SEED)
    dt = gix.bind()
    queries = [[b"t1", b"t2", b"unknown"], [lexeme(0), b"t4"]]
    tids = np.array([[0, d, 1] for d in range(5, 10)] + [[9, 9, 9]], dtype=np.uint16)
    n = len(tids)
    named = {}
    with dt.reranker(res, 2, 8, 64, 4096, 1024, 16, from_index=True) as ring:

        def rerank(step):
            ring.submit(queries, 8, [0, n, 2 * n], cand_tid=np.concatenate([tids, tids]))
            ranks, n_ranks = ring.collect()
            assert f"{step}: {dt.n_docs} documents, {dt.dead_docs} dead, directory {ring.directory_docs}" in out
            got = [l.split()[2:] for l in out.splitlines() if l.startswith(f"row {step} ")]
            assert len(got) == 16
            for q, i, nr, pos, doc, score in got:
                q, i = int(q), int(i)
                assert int(nr) == n_ranks[q] and int(pos) == ranks["pos"][q, i] and int(doc) == ranks["doc"][q, i], (step, q, i)
                assert np.float64(float.fromhex(score)).view(np.uint64) == ranks["score"][q, i].view(np.uint64), (step, q, i)
            named[step] = dict(zip(ranks["pos"][0, :n_ranks[0]].tolist(), ranks["doc"][0, :n_ranks[0]].tolist()))

        rerank("bound")
        with vb.TidSet(np.array([[0, VICTIM, 1]], np.uint16)) as gone:
            assert dt.delete_tids(gone) == 1
        assert f"deleted 1, word 0 of the bitmap {int(dt.read_dead()[0]):x}\n" in out and int(dt.read_dead()[0]) == 1 << VICTIM
        rerank("deleted")
        dt.append_documents(rows(40, 41, VICTIM), res)
        rerank("appended")
        ring.sync()
        rerank("synced")
        assert dt.delete([VICTIM, VICTIM]) == 0 and "deleted again 0, dead 1\n" in out
    # pos 2 is the ctid of row 7: the sealed row, nobody, nobody until the sync, the new row; pos 5 names nobody throughout
    assert named["bound"] == {0: 5, 1: 6, 2: 7, 3: 8, 4: 9}
    assert named["deleted"] == named["appended"] == {0: 5, 1: 6, 3: 8, 4: 9}
    assert named["synced"] == {0: 5, 1: 6, 2: 40, 3: 8, 4: 9}
