"""vbm25::Scorer of include/vbm25.hpp (DocTerms::scorer, evaluate, topk) compiles against the C ABI and reranks one batch entry for
entry as the Python mirror does: examples/evaluate_example.cpp prints its top-3 rows with the scores as hexadecimal floats."""
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


def test_the_example_uses_the_scorer_and_compiles(tmp_path):
    src = open(os.path.join(ROOT, "examples", "evaluate_example.cpp")).read()
    assert "vbm25::Scorer" in src and ".topk(" in src and "bound.scorer()" in src
    assert os.path.exists(build_example(tmp_path))


def lexeme(j):
    return b"t%d" % j if j % 3 else b"a-lexeme-of-the-long-kind-%d" % j


@pytest.mark.gpu
def test_cpp_scorer_ranks_match_python(tmp_path):
    out = subprocess.check_output([build_example(tmp_path)], text=True, timeout=120)
    docs = [[(lexeme(j), 1 + (d * 7 + j) % 4) for j in range(12) if (d + j) % (2 + j % 3) == 0] for d in range(40)]
    pay = np.array([[0, d, 1] for d in range(41)], dtype=np.uint16)
    gix = vb.GpuIndex(vb.DeviceSegment.from_documents(vb.Documents.cast(docs, pay[:40], seed=SEED), 1.2, 0.75))
    r = vb.Resolver(gix, 1, 8, 64, 4096, seed=SEED)
    rows = vb.Documents.cast(docs + [[(b"t1", 2), (b"not-in-the-index", 9)]], pay, seed=SEED)
    dt = rows.bind(r)
    r.submit([[b"t1", b"t2", b"unknown"], [lexeme(0), b"t4"], []])
    term_ids, q_off = r.collect()
    assert "scorer evaluate equal" in out
    with dt.scorer() as s:
        for tag, args in (("top listed", ([0, 3, 5, 6], [40, 0, 7, 39, 39, 2])), ("top cross", ())):
            ranks, n_ranks = s.topk(term_ids, q_off, 3, *args)
            # the Python result is the definition's: a stable descending sort of DocTerms.evaluate cut at 3
            scores = dt.evaluate(term_ids, q_off, *args)
            for q in range(3):
                row = scores[q] if not args else scores[args[0][q]:args[0][q + 1]]
                order = np.argsort(-row, kind="stable")[:3]
                assert n_ranks[q] == len(order) and ranks["pos"][q, :len(order)].tolist() == order.tolist()
            got = [l.split()[2:] for l in out.splitlines() if l.startswith(tag + " ")]
            assert len(got) == 9
            for q, i, n, pos, doc, score in got:
                q, i = int(q), int(i)
                assert int(n) == n_ranks[q] and int(pos) == ranks["pos"][q, i] and int(doc) == ranks["doc"][q, i]
                assert np.float64(float.fromhex(score)).view(np.uint64) == ranks["score"][q, i].view(np.uint64), (tag, q, i)
        held = [int(l.split()[2]) for l in out.splitlines() if l.startswith("scorer holds ")]
        assert len(held) == 1 and held[0] >= s.device_bytes() > 0  # (the example's scorer has also served an evaluate)
    assert (ranks["score"][:2] > 0).any() and n_ranks.tolist() == [3, 3, 3]
