"""bench.py --dump-outputs above its size limit: a fixed seeded sample of the queries, their indices beside it (host only)."""
import os

import numpy as np

import bench
import vectorchord_bm25_amd as vb


def test_dump_above_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200_000)
    nq, k = 5000, 10
    hits = np.zeros((nq, k), dtype=vb.HIT_DTYPE)
    hits["score"] = np.random.default_rng(1).random((nq, k))
    hits["doc_id"] = np.arange(nq * k, dtype=np.uint32).reshape(nq, k)
    hits["payload"] = 65535
    n_hits = np.arange(nq, dtype=np.uint32) % (k + 1)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), hits, n_hits)
    names = ["doc_id.npy", "n_hits.npy", "payload.npy", "query_index.npy", "score.npy"]
    for d in dirs:
        assert sorted(os.listdir(d)) == names
        assert sum(os.path.getsize(d / f) for f in names) <= bench.DUMP_MAX_BYTES
    for f in names:
        assert (dirs[0] / f).read_bytes() == (dirs[1] / f).read_bytes()
    got = {f[:-4]: np.load(dirs[0] / f) for f in names}
    rows = got["query_index"].astype(np.int64)
    assert 0 < len(rows) < nq and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["score"], hits["score"][rows]) and np.array_equal(got["doc_id"], hits["doc_id"][rows])
    assert np.array_equal(got["payload"], hits["payload"][rows]) and np.array_equal(got["n_hits"], n_hits[rows])
