"""vbm25_batch_run, detached: a one-launch run of scan_win_kernel of a batch without a filter goes to a stream the batch object owns
(tuning switch run_overlap, default 1), so that runs of different batch objects overlap.  Runs in rotation without a fetch in
between, on the default stream and on a side stream, against the oracle and against the same sequence with run_overlap = 0; the
re-run after a given-up item under overlap; every way out of the detached form (device addresses asked for, a filter attached, a new
query set, a batch destroyed beside a sibling's run); kernel_ms as exclusive shares; and the batches that are never detached.
-m gpu only.

Corpora and query sets are those of test_gpu_win_lds_merge.py: 190 000 documents are three windows, three items per query.  nq = 4 is one
full workgroup of four queries, 5 one and a rest query through memory, 9 two and one."""
import time

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from growing_data import make_growing
from parity import assert_bit_exact
from test_gpu_win_lds_merge import N_DOCS, V_GROUPS, Built, _corpus, _v_queries

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
NONE32 = 0xFFFFFFFF
NQS = (4, 5, 9)
KS = (1, 10, 64)
N_OBJ = 4


@pytest.fixture(scope="module")
def V():
    return Built(_corpus(V_GROUPS, seed=1))


@pytest.fixture(scope="module")
def G():
    # (the corpus of test_one_launch_merge_and_its_fallback at three windows: more second arrivals in a window than the list holds)
    return Built(make_corpus(N_DOCS, 3000, seed=2, length="lognormal", mean_len=60))


class _DevArray:
    """__cuda_array_interface__ view of a device buffer of the library (for torch)"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _device_views(b, nq, k):
    import torch

    hp, cp = b.device_results()
    return (torch.as_tensor(_DevArray(hp, nq * k * 3, "<i8"), device="cuda"), torch.as_tensor(_DevArray(cp, nq, "<i4"), device="cuda"))


def _objects(B, nq, k, seed0):
    """N_OBJ batch objects with different query sets, each on the one-launch window form"""
    out = []
    for i in range(N_OBJ):
        terms, off = _v_queries(nq, seed=seed0 + 7 * i)
        b = vb.Batch(B.gix, nq, len(terms), k)
        b.set_queries(terms, off)
        assert b.debug_route() == 3, f"route {b.debug_route()}"
        out.append((b, terms, off))
    return out


def _assert_one_launch(b, nq):
    assert b.debug_win_launches() == 1, "the run did not take the one-launch form"
    assert b.debug_win_handover() == (2 if nq >= 4 else 1), f"hand-over {b.debug_win_handover()}"


def _assert_oracle(B, terms, off, k, hits, nh, what):
    rb, rnb = B.ref(terms, off, k)
    assert np.array_equal(nh, rnb), f"{what}: counts {nh} want {rnb}"
    for q in range(len(off) - 1):
        assert_bit_exact(rb[q, :rnb[q]], hits[q, :nh[q]], what=f"{what} q{q}")


def _rotation(B, nq, k, stream, rounds=3):
    objs = _objects(B, nq, k, seed0=100 + nq)
    for _ in range(rounds):
        for b, _, _ in objs:
            b.run(stream)
    for b, _, _ in objs:
        _assert_one_launch(b, nq)
    return objs, [b.fetch() for b, _, _ in objs]


@pytest.mark.parametrize("side", [False, True], ids=["default_stream", "side_stream"])
@pytest.mark.parametrize("k", KS)
def test_rotation_without_fetch(tuning, V, k, side):
    """four objects, three rounds, one stream, no fetch in between: the oracle's records, and the bytes of run_overlap = 0"""
    import torch

    stream = torch.cuda.Stream().cuda_stream if side else None
    for nq in NQS:
        tuning(win_force=1, fused=0, run_overlap=1)
        objs, got = _rotation(V, nq, k, stream)
        for i, ((b, terms, off), (hits, nh)) in enumerate(zip(objs, got)):
            _assert_oracle(V, terms, off, k, hits, nh, f"nq {nq} k {k} object {i}")
        tuning(run_overlap=0)
        _, plain = _rotation(V, nq, k, stream)
        for i, ((hits, nh), (h0, n0)) in enumerate(zip(got, plain)):
            assert hits.tobytes() == h0.tobytes() and np.array_equal(nh, n0), f"nq {nq} k {k} object {i}: differs from run_overlap = 0"
        torch.cuda.synchronize()


def test_fifty_rounds_are_the_first(tuning, V):
    """the results under overlap are the same every time: four objects x 50 rounds at nq = 9, fetched after each round of four"""
    tuning(win_force=1, fused=0)
    objs = _objects(V, 9, 10, seed0=300)
    first = None
    for r in range(50):
        for b, _, _ in objs:
            b.run()
        got = [b.fetch() for b, _, _ in objs]
        if first is None:
            first = got
            for i, ((b, terms, off), (hits, nh)) in enumerate(zip(objs, got)):
                _assert_one_launch(b, 9)
                _assert_oracle(V, terms, off, 10, hits, nh, f"object {i}")
        for i, ((hits, nh), (h0, n0)) in enumerate(zip(got, first)):
            assert hits.tobytes() == h0.tobytes() and np.array_equal(nh, n0), f"round {r} object {i}"


@pytest.mark.parametrize("nq", [5, 8])
def test_given_up_items_in_two_overlapping_objects(tuning, G, nq):
    """thick lists: both one-launch runs mark queries; each fetch repeats its batch's scan behind the overlapped run"""
    tuning(win_force=1, fused=0, win_fuse=1)
    objs = []
    for seed in (9, 10):
        terms, off = make_queries(G.c, nq, 4, seed=seed)
        b = vb.Batch(G.gix, nq, len(terms), 10)
        b.set_queries(terms, off)
        assert b.debug_route() == 3
        objs.append((b, terms, off))
    for b, _, _ in objs:
        b.run()
    for b, _, _ in objs:
        assert b.debug_win_launches() == 1
    gave_up = 0
    for i, (b, terms, off) in enumerate(objs):
        hits, nh = b.fetch()
        assert not (nh == NONE32).any(), "a count of NONE32 reached the caller"
        gave_up += b.debug_counts()[1]
        _assert_oracle(G, terms, off, 10, hits, nh, f"object {i}")
    assert gave_up > 0, "this shape is expected to give items up"


def test_device_addresses_after_detached_runs(tuning, V):
    """detached runs, then vbm25_batch_device_results: the next run's records, read on the stream by torch without a fetch"""
    import torch

    tuning(win_force=1, fused=0)
    nq, k = 9, 10
    (b, terms, off), (sib, _, _) = _objects(V, nq, k, seed0=400)[:2]
    for _ in range(2):
        b.run()
        sib.run()
    _assert_one_launch(b, nq)
    recs, cnts = _device_views(b, nq, k)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.run(s.cuda_stream)
        assert b.debug_win_launches() == 3, "a device consumer's run is expected to leave complete records"
        got, got_n = recs.clone(), cnts.clone()
    s.synchronize()
    hits, nh = b.fetch()
    _assert_oracle(V, terms, off, k, hits, nh, "fetched")
    assert got.cpu().numpy().tobytes() == hits.tobytes(), "the records read in stream order differ from the fetched ones"
    assert np.array_equal(got_n.cpu().numpy().astype(np.uint32), nh)
    sib.fetch()


def test_filter_after_detached_runs(tuning, V):
    tuning(win_force=1, fused=0)
    nq, k = 5, 10
    (b, terms, off), (sib, _, _) = _objects(V, nq, k, seed0=500)[:2]
    b.run()
    sib.run()
    b.run()
    ids = np.arange(N_DOCS)
    keeps = np.stack([ids % 2 == 0, ids % 7 == 3])
    sel = np.array([[0, NONE, 1][q % 3] for q in range(nq)], dtype=np.uint32)
    f = vb.DocFilter(V.gix, keeps)
    b.set_filter(f, sel)
    b.run()
    hits, nh = b.fetch()
    for q in range(nq):
        full = V.oix.search_brute(terms[off[q]:off[q + 1]], 65535)
        assert len(full) < 65535
        want = full[:k] if sel[q] == NONE else full[keeps[sel[q]][full["doc_id"]]][:k]
        assert nh[q] == len(want)
        assert_bit_exact(want, hits[q, :nh[q]], what=f"filtered q{q}")
    sib.fetch()


def test_new_queries_right_after_a_detached_run(tuning, V):
    tuning(win_force=1, fused=0)
    nq, k = 9, 10
    (b, _, _), (sib, st, so) = _objects(V, nq, k, seed0=600)[:2]
    terms, off = _v_queries(nq, seed=677)
    sib.run()
    b.run()
    b.set_queries(terms, off)
    b.run()
    _assert_one_launch(b, nq)
    hits, nh = b.fetch()
    _assert_oracle(V, terms, off, k, hits, nh, "the new queries")
    _assert_oracle(V, st, so, k, *sib.fetch(), "the sibling")


def test_destroyed_beside_a_siblings_run(tuning, V):
    tuning(win_force=1, fused=0)
    nq, k = 9, 10
    (b, _, _), (sib, st, so) = _objects(V, nq, k, seed0=700)[:2]
    sib.run()
    b.run()
    del b  # (vbm25_batch_destroy, no fetch before it)
    _assert_oracle(V, st, so, k, *sib.fetch(), "the sibling")


def test_kernel_ms_is_an_exclusive_share(tuning, V):
    """four objects x 3 rounds, timed: exclusive shares cannot add up to more than the time that went by"""
    import torch

    for overlap in (1, 0):
        tuning(win_force=1, fused=0, run_overlap=overlap)
        objs = _objects(V, 9, 10, seed0=800)
        for b, _, _ in objs:
            b.run()
        torch.cuda.synchronize()
        for b, _, _ in objs:
            b.set_timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            for b, _, _ in objs:
                b.run()
        torch.cuda.synchronize()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        parts = [b.kernel_ms() for b, _, _ in objs]
        print(f"run_overlap {overlap}: wall {wall_ms:.4f} ms, kernel_ms {parts}")
        for ms, n in parts:
            assert n == 3
            assert ms > 0
        if overlap:
            assert sum(ms * n for ms, n in parts) <= wall_ms
        for b, _, _ in objs:
            _assert_one_launch(b, 9)
            b.set_timing(False)


def _behind_a_busy_stream(s, b):
    """b.run on stream s behind 50 ms of other work, then the device addresses: a run that stays in stream order makes nobody wait
    for it (the stream is still busy when the addresses come back), and torch reads its complete records in stream order"""
    import torch

    with torch.cuda.stream(s):
        torch.cuda._sleep(100_000_000)
        b.run(s.cuda_stream)
        recs, cnts = _device_views(b, b.nq, b.k)
        busy = not s.query()
        got, got_n = recs.clone(), cnts.clone()
    s.synchronize()
    return busy, got.cpu().numpy().tobytes(), got_n.cpu().numpy().astype(np.uint32)


def test_batches_that_are_not_detached(tuning, V):
    """a filter, a growing segment, device addresses asked for: complete records in stream order, no fetch"""
    import torch

    tuning(win_force=1, fused=0)
    nq, k = 9, 10
    terms, off = _v_queries(nq, seed=900)
    s = torch.cuda.Stream()
    ids = np.arange(N_DOCS)
    keeps = np.stack([ids % 2 == 0, ids % 7 == 3])
    sel = np.array([[0, NONE, 1][q % 3] for q in range(nq)], dtype=np.uint32)
    f = vb.DocFilter(V.gix, keeps)
    G, _ = make_growing(V.seg.arrays()["term_key"], 3000, seed=5, pool=terms)
    gs = vb.GrowingSegment(V.gix, **G)
    for what in ("filter", "growing", "device"):
        b = vb.Batch(V.gix, nq, len(terms), k)
        if what == "filter":
            b.set_filter(f, sel)
        if what == "growing":
            b.set_growing(gs)
        b.set_queries(terms, off)
        assert b.debug_route() == 3
        if what == "device":
            b.device_results()
        busy, got, got_n = _behind_a_busy_stream(s, b)
        assert busy, f"{what}: the run was waited for -- it did not stay in the caller's stream order"
        hits, nh = b.fetch()
        assert got == hits.tobytes() and np.array_equal(got_n, nh), f"{what}: the records read in stream order are not the fetched ones"
        if what == "growing":
            h1, n1 = vb.search_batch_growing(V.gix, gs, terms, off, k)
            assert hits.tobytes() == h1.tobytes() and np.array_equal(nh, n1)
        if what == "device":
            _assert_oracle(V, terms, off, k, hits, nh, what)
        if what == "filter":
            for q in range(nq):
                full = V.oix.search_brute(terms[off[q]:off[q + 1]], 65535)
                want = full[:k] if sel[q] == NONE else full[keeps[sel[q]][full["doc_id"]]][:k]
                assert nh[q] == len(want)
                assert_bit_exact(want, hits[q, :nh[q]], what=f"filter q{q}")
