"""One batch object over its whole life, as INTEGRATION.md, bench.py and the stream / multi-device rings use it: query set after query
set, refused sets in between, filters and growing segments attached and detached, device_results, repeated runs.  Every record is
compared bit for bit with the oracle's brute force for the batch's state of the moment (tests/lifecycle_data.py), and every shape
asserts the route it takes.

include/vbm25.h: a failed vbm25_batch_set_queries / vbm25_multi_batch_set_queries leaves the object holding no queries -- run does
nothing, fetch writes nothing, the next set works on every route.  -m gpu only."""
import ctypes as C

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_queries
from growing_data import make_growing
from lifecycle_data import (NONE, Expect, bench_queries, built, check, failing_sets, from_rows, id16_blocks, rows_of,
                            term_df)

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5

_CACHE = {}


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _index(name, seg, **index_tune):
    """a GpuIndex of `seg` made under the index-creation switches `index_tune` (cached per name)"""
    def make():
        for n, v in index_tune.items():
            vb.set_tuning(n, v)
        try:
            return vb.GpuIndex(seg)
        finally:
            vb.reset_tuning()
    return _cached(name, make)


def _corpus_a_dict():
    return _cached("A dict", lambda: make_corpus(200_000, 3000, seed=2, length="lognormal", mean_len=60))


def _corpus(name):
    """(segment, Expect, set A, set B): two different valid query sets of each corpus"""
    def make():
        if name == "A":  # 200 k documents, 4-term queries (thick lists: win_force gives items up)
            c = _corpus_a_dict()
            seg = built(c)
            a, b = make_queries(c, 48, 4, seed=9), make_queries(c, 30, 4, seed=10)
        elif name == "A20":  # more than 16 terms: scan_many_kernel
            c = make_corpus(60_000, 3000, seed=4, length="lognormal", mean_len=60)
            seg = built(c)
            a, b = make_queries(c, 16, 20, seed=14), make_queries(c, 11, 20, seed=15)
        elif name == "C3":  # C3's shape at reduced size: scan_win_kernel
            seg = vb.Segment.synth(700_000, 33_000, mean_len=100, len_mode=1, seed=7)
            a, b = bench_queries(seg, 33_000, 160, 5, seed=3), bench_queries(seg, 33_000, 96, 5, seed=4)
        elif name == "Z":  # Zipf head terms: scan_dense_kernel
            seg = vb.Segment.synth(60_000, 20_000, mean_len=100, len_mode=1, zipf_s=1.0, seed=3)
            a, b = bench_queries(seg, 20_000, 48, 3, seed=5, zipf_s=1.0), bench_queries(seg, 20_000, 40, 3, seed=6, zipf_s=1.0)
        else:
            raise KeyError(name)
        return seg, Expect(seg), a, b
    return _cached("corpus " + name, make)


def _head(s, n):
    t, o = s
    return t[:o[n]], o[:n + 1]


def _raw_fetch_writes_nothing(b, rows, k, what):
    """vbm25_batch_fetch into `rows` rows pre-filled with a sentinel: VBM25_OK, nothing written"""
    hits = np.zeros((rows, k), dtype=vb.HIT_DTYPE)
    hits.view(np.uint8)[...] = SENTINEL
    cnt = np.full(rows, SENTINEL * 0x01010101, dtype=np.uint32)
    vb.api.check(vb.lib().vbm25_batch_fetch(b.h, hits.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
    assert np.all(hits.view(np.uint8) == SENTINEL) and np.all(cnt == SENTINEL * 0x01010101), f"{what}: fetch wrote records"


# (case, corpus, k, route, batch tuning, index tuning, attachment)
ROUTES = [
    ("fused", "A", 10, 1, {}, {}, None),
    ("plan", "A", 10, 0, dict(fused=0, arith=0, win=0), {}, None),
    ("arith", "A", 10, 2, dict(fused=0, win=0), {}, None),
    ("win_one_launch", "C3", 10, 3, dict(fused=0), {}, None),
    ("win_giveup", "A", 10, 3, dict(win_force=1, fused=0), {}, None),
    ("win_id16_decode", "C3", 10, 3, dict(fused=0), dict(id16_plane=0, rel16_plane=0), None),
    ("dense", "Z", 10, 0, {}, {}, None),
    ("terms_over_16", "A20", 10, 0, {}, {}, None),
    ("bigk_k2000", "A20", 2000, 4, {}, {}, None),
    ("win_filter", "C3", 10, 3, dict(fused=0), {}, "filter"),
    ("win_growing", "C3", 10, 3, dict(fused=0), {}, "growing"),
]


@pytest.mark.parametrize("case,corpus,k,route,tune,index_tune,attach", ROUTES, ids=[r[0] for r in ROUTES])
def test_failed_set_queries_leave_an_empty_reusable_batch(tuning, case, corpus, k, route, tune, index_tune, attach):
    seg, ex, set_a, set_b = _corpus(corpus)
    if route == 1:  # (the one-launch route: a handful of queries)
        set_a, set_b = _head(set_a, 4), _head(set_b, 3)
    elif route == 4:
        set_a, set_b = _head(set_a, 3), _head(set_b, 3)
    gix = _index(f"{corpus} {sorted(index_tune.items())}", seg, **index_tune)
    tuning(**tune)
    max_q = max(len(set_a[1]), len(set_b[1])) - 1
    max_t = max(len(set_a[0]), len(set_b[0]))
    b = vb.Batch(gix, max_q, max_t, k)
    ids = np.arange(seg.n_docs)
    keeps = np.stack([ids % 10 == 7, ids % 3 == 1])
    sel = np.array([[0, NONE, 1][q % 3] for q in range(max_q)], dtype=np.uint32)
    G = None
    if attach == "filter":
        b.set_filter(vb.DocFilter(gix, keeps), sel)
    elif attach == "growing":
        G, _ = make_growing(seg.arrays()["term_key"], 3000, seed=4, pool=set_a[0][set_a[0] < seg.n_terms])
        b.set_growing(vb.GrowingSegment(gix, **G))

    def want(t, o):
        if attach == "filter":
            return ex.filtered(t, o, k, keeps, sel)
        if attach == "growing":
            return ex.growing(t, o, k, G)
        return ex.plain(t, o, k)

    def run_and_check(t, o, what):
        b.set_queries(t, o)
        assert b.debug_route() == route, f"{what}: route {b.debug_route()} instead of {route}"
        if corpus == "Z":
            assert b.debug_routes()[1] > 0, f"{what}: no query classed dense"
        b.run()
        hits, nh = b.fetch()
        check(want(t, o), hits, nh, f"{case} {what}")
        if case == "win_one_launch":
            assert b.debug_win_launches() == 1
        elif attach == "growing":
            assert b.debug_win_launches() == 3  # (a growing segment takes the complete-records form)

    run_and_check(*set_a, "set A")
    if case == "win_giveup":
        assert b.debug_counts()[1] > 0 and b.debug_win_launches() == 3, "this shape is expected to give items up"
    for name, t, o, code in failing_sets(*set_a, max_q, max_t, seg.n_terms):
        with pytest.raises(vb.Vbm25Error) as e:
            b.set_queries(t, o)
        assert e.value.code == code, f"{name}: error {e.value.code}, want {code}"
        assert b.nq == 0, f"{name}: the Python mirror kept {b.nq} queries"
        b.run()
        _raw_fetch_writes_nothing(b, max_q, k, name)
        hits, nh = b.fetch()
        assert hits.shape == (0, k) and len(nh) == 0
    run_and_check(*set_b, "set B")


def test_scratch_plane_limit_falls_back_to_scan_range(tuning):
    """An index without post_id16 and a scratch-plane limit below what the larger set needs: under the limit the window route (through
    decode_id16_kernel), over it scan_range_kernel, under it again the window route -- on one batch object, through vbm25_search_batch
    and through a stream of depth 3.  Each set's records are those of the same segment's index with every plane."""
    seg, ex, _, _ = _corpus("C3")
    full = _index("C3 []", seg)
    nop = _index("C3 [('id16_plane', 0), ('rel16_plane', 0)]", seg, id16_plane=0, rel16_plane=0)
    df = term_df(seg)
    under1 = bench_queries(seg, 33_000, 16, 5, seed=21)
    over = bench_queries(seg, 33_000, 64, 5, seed=22)
    under2 = bench_queries(seg, 33_000, 16, 5, seed=23)
    need = [id16_blocks(df, *s) for s in (under1, over, under2)]
    limit = (max(need[0], need[2]) + need[1]) // 2
    assert need[0] <= limit < need[1] and need[2] <= limit
    tuning(fused=0, id16_max_blocks=limit)
    sets = [("under", under1, 3), ("over", over, 2), ("under again", under2, 3)]
    wants = {}
    for name, (t, o), _ in sets:
        wants[name] = vb.search_batch(full, t, o, 10)
        check(ex.plain(t, o, 10), *wants[name], f"{name} (every plane)")
    max_t = max(len(s[1][0]) for s in sets)
    b = vb.Batch(nop, 64, max_t, 10)
    for name, (t, o), route in sets:
        b.set_queries(t, o)  # (raises on a library that refuses the set: nothing is launched)
        assert b.debug_route() == route, f"{name}: route {b.debug_route()} instead of {route}"
        b.run()
        hits, nh = b.fetch()
        assert np.array_equal(nh, wants[name][1]) and hits.tobytes() == wants[name][0].tobytes(), f"{name}: records differ"
    for name, (t, o), _ in sets:
        hits, nh = vb.search_batch(nop, t, o, 10)
        assert np.array_equal(nh, wants[name][1]) and hits.tobytes() == wants[name][0].tobytes(), f"{name} (search_batch)"
    st = vb.Stream(nop, 3, 64, max_t, 10)
    for _, (t, o), _ in sets:
        st.submit(t, o)
    for name, _, _ in sets:
        hits, nh = st.collect()
        assert np.array_equal(nh, wants[name][1]) and hits.tobytes() == wants[name][0].tobytes(), f"{name} (stream)"


def test_failed_multi_batch_set_queries_leaves_every_shard_empty():
    """Three replicas on device 0, 101 queries set and fetched; then 40 queries whose last shard holds an unsorted query: the error,
    and a fetch into buffers of twice max_queries rows with guard words behind them writes nothing (a shard that kept its old 33
    queries would write them at the new set's offset 27).  Then a valid set: byte for byte the single handle's records."""
    seg, ex, _, _ = _corpus("A")
    c = _corpus_a_dict()
    t101, o101 = make_queries(c, 101, 4, seed=31)
    t40, o40 = make_queries(c, 40, 4, seed=32)
    t40 = t40.copy()
    a = int(o40[-2])
    t40[a], t40[a + 1] = t40[a + 1], t40[a]
    t60, o60 = make_queries(c, 60, 3, seed=33)
    single = _index("A []", seg)
    multi = vb.MultiIndex(seg, [0, 0, 0])
    max_q, max_t = 101, len(t101)
    mb = vb.MultiBatch(multi, max_q, max_t, 10)
    mb.set_queries(t101, o101)
    mb.run()
    check(ex.plain(t101, o101, 10), *mb.fetch(), "101 queries")
    with pytest.raises(vb.Vbm25Error) as e:
        mb.set_queries(t40, o40)
    assert e.value.code == -1
    assert mb.nq == 0
    mb.run()
    hits = np.zeros((2 * max_q + 4, 10), dtype=vb.HIT_DTYPE)
    hits.view(np.uint8)[...] = SENTINEL
    cnt = np.full(2 * max_q + 4, SENTINEL * 0x01010101, dtype=np.uint32)
    vb.api.check(vb.lib().vbm25_multi_batch_fetch(mb.h, hits.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
    assert np.all(cnt == SENTINEL * 0x01010101), f"counts written at rows {np.flatnonzero(cnt != SENTINEL * 0x01010101)}"
    assert np.all(hits.view(np.uint8) == SENTINEL), "records written"
    assert len(mb.fetch()[1]) == 0
    mb.set_queries(t60, o60)
    mb.run()
    h, n = mb.fetch()
    h1, n1 = vb.search_batch(single, t60, o60, 10)
    assert np.array_equal(n, n1) and h.tobytes() == h1.tobytes()


# ---- route and feature transitions on one batch object ----

def _zipf_corpus():
    """Zipf(1) at reduced size: the library's own routing reaches every route.  Shapes: window (5 terms of comparable df, 32 .. 232
    postings per 2^16-document window), range (one thicker term beside two of them), one launch (4 queries), many (a query of 20
    terms), dense (Zipf head terms)."""
    def make():
        seg = vb.Segment.synth(400_000, 20_000, mean_len=100, len_mode=1, zipf_s=1.0, seed=5)
        df = term_df(seg)
        wins = seg.n_docs / 65536.0
        band = np.flatnonzero((df >= 80 * wins) & (df < 120 * wins))
        thick = np.flatnonzero((df >= 600 * wins) & (df < 0.02 * seg.n_docs))
        head = np.argsort(-df)[:12]
        assert len(band) >= 200 and len(thick) >= 10 and df[head].min() >= 0.1 * seg.n_docs
        return seg, Expect(seg), dict(band=band, thick=thick, head=head)
    return _cached("zipf", make)


def _shape_queries(pools, shape, rng):
    def pick(pool, n):
        return np.sort(rng.choice(pool, n, replace=False)).astype(np.uint32)
    band = pools["band"]
    if shape == "win":
        rows = [pick(band, 5) for _ in range(int(rng.integers(140, 200)))]
    elif shape == "range":
        rows = [np.sort(np.r_[pick(pools["thick"], 1), pick(band, 2)]).astype(np.uint32) for _ in range(int(rng.integers(140, 200)))]
    elif shape == "one":
        rows = [pick(band, 5) for _ in range(4)]
    elif shape == "many":
        rows = [pick(band, 5) for _ in range(int(rng.integers(20, 60)))] + [pick(band, 20)]
    elif shape == "dense":
        rows = [pick(pools["head"], 3) for _ in range(int(rng.integers(10, 40)))]
    elif shape == "w4":  # corpus A under win_force: thick lists, items given up
        rows = [pick(band, 4) for _ in range(int(rng.integers(30, 64)))]
    elif shape == "t12":
        rows = [pick(band, 12) for _ in range(int(rng.integers(20, 40)))]
    elif shape == "t20":
        rows = [pick(band, 20) for _ in range(int(rng.integers(10, 20)))]
    else:
        raise KeyError(shape)
    return from_rows(rows)


def _sequence(seed, n_steps, shapes, no_filter_shapes, devres_at):
    """a seeded sequence of steps; filter and growing segment are never attached together, a filter never meets a shape whose
    full ranking the oracle would cut"""
    rng = np.random.default_rng(seed)
    steps, filt, grow, shape = [], False, 0, None
    for i in range(n_steps):
        if i == devres_at:
            steps.append(("devres",))
            continue
        opts = [("set", s) for s in shapes if not (filt and s in no_filter_shapes)] * 2
        if shape is not None:
            if not filt and not grow and shape not in no_filter_shapes:
                opts.append(("filter",))
            if filt:
                opts += [("unfilter",), ("update",)]
            if not filt:
                opts.append(("grow",))
            if grow:
                opts.append(("ungrow",))
        step = opts[int(rng.integers(len(opts)))]
        if step[0] == "set":
            shape = step[1]
        elif step[0] == "filter":
            filt = True
        elif step[0] == "unfilter":
            filt = False
        elif step[0] == "grow":
            grow += 1
        elif step[0] == "ungrow":
            grow = 0
        steps.append(step)
    return steps


def _drive(seg, ex, gix, pools, steps, seed, k=10):
    """runs `steps` on one batch object; after every step the batch is run and its records checked.  Returns what was reached:
    (route, launches, filtered, growing, device_results) per run"""
    rng = np.random.default_rng(seed + 1)
    ids = np.arange(seg.n_docs)
    b = vb.Batch(gix, 256, 256 * 20, k)
    keeps = np.stack([ids % 10 == 3, ids % 7 == 1])
    f = vb.DocFilter(gix, keeps)
    key = seg.arrays()["term_key"]
    segs = [make_growing(key, n, seed=seed + n, pool=pools["band"], pool_p=0.5)[0] for n in (3000, 3 * 8192 + 5)]
    gsegs = [vb.GrowingSegment(gix, **G) for G in segs]
    assert gsegs[1].device_bytes > gsegs[0].device_bytes
    hip = C.CDLL("libamdhip64.so")
    state = dict(t=None, o=None, sel=None, G=None, dev=None)
    reached = []
    for i, step in enumerate(steps):
        what = f"step {i} {step}"
        if step[0] == "set":
            t, o = _shape_queries(pools, step[1], rng)
            b.set_queries(t, o)
            state.update(t=t, o=o)
        elif step[0] == "filter":
            sel = rng.choice(np.array([0, 1, NONE], dtype=np.uint32), 256)
            b.set_filter(f, sel)
            state["sel"] = sel
        elif step[0] == "unfilter":
            b.set_filter(None)
            state["sel"] = None
        elif step[0] == "update":
            j = int(rng.integers(2))
            keeps[j] = rng.random(seg.n_docs) < 0.3
            f.update(j, keeps[j])
        elif step[0] == "grow":
            g = 1 if state["G"] is not None else int(rng.integers(2))  # (a second attach: the larger re-upload)
            b.set_growing(gsegs[g])
            state["G"] = segs[g]
        elif step[0] == "ungrow":
            b.set_growing(None)
            state["G"] = None
        elif step[0] == "devres":
            state["dev"] = b.device_results()
        t, o = state["t"], state["o"]
        route = b.debug_route()
        b.run()
        nq = len(o) - 1
        if state["dev"] is not None:  # the complete records on the device, read behind the run (null stream)
            hits = np.zeros((nq, k), dtype=vb.HIT_DTYPE)
            nh = np.zeros(nq, dtype=np.uint32)
            assert hip.hipMemcpy(C.c_void_p(hits.ctypes.data), C.c_void_p(state["dev"][0]), C.c_size_t(hits.nbytes), 2) == 0
            assert hip.hipMemcpy(C.c_void_p(nh.ctypes.data), C.c_void_p(state["dev"][1]), C.c_size_t(nh.nbytes), 2) == 0
        else:
            hits, nh = b.fetch()
        launches = b.debug_win_launches()
        if state["sel"] is not None:
            want = ex.filtered(t, o, k, keeps, state["sel"])
        elif state["G"] is not None:
            want = ex.growing(t, o, k, state["G"])
        else:
            want = ex.plain(t, o, k)
        check(want, hits, nh, what)
        reached.append((route, launches, state["sel"] is not None, state["G"] is not None, state["dev"] is not None,
                        b.debug_counts()[1] if route == 3 else 0))
    return reached


def test_route_and_feature_transitions_on_one_batch():
    """About 40 seeded steps on one batch object under the library's own routing: query sets of every route, filters attached,
    updated and detached, growing segments attached (also a larger re-upload) and detached, device_results."""
    seg, ex, pools = _zipf_corpus()
    gix = _index("zipf []", seg)
    steps = _sequence(11, 40, ["win", "range", "one", "many", "dense"], {"dense"}, devres_at=30)
    reached = _drive(seg, ex, gix, pools, steps, seed=11)
    routes = {r[0] for r in reached}
    assert routes >= {0, 1, 2, 3}, f"routes reached: {routes}"
    win = [r for r in reached if r[0] == 3]
    assert any(r[1] == 1 and not r[4] for r in win), "no one-launch window run"
    assert any(r[1] == 3 and not r[4] for r in win), "no three-launch window run before device_results"
    assert any(r[1] == 3 and r[4] for r in win), "no window run after device_results"
    assert any(r[2] for r in win) and any(r[3] for r in win), "no filtered / growing window run"


def test_transitions_across_the_give_up_rerun(tuning):
    """The same on corpus A under win_force=1, fused=0 (and no query dense: 12 terms take scan_range_kernel): the window route's
    one-launch run gives items up and fetch re-runs the set with three launches (win_nofuse), across set_queries, filter and growing
    segment changes."""
    seg, ex, _, _ = _corpus("A")
    gix = _index("A []", seg)
    tuning(win_force=1, fused=0, dense_x1000=10 ** 9)
    df = term_df(seg)
    pools = dict(band=np.flatnonzero(df > 0))
    steps = _sequence(13, 30, ["w4", "t12", "t20"], {"t20"}, devres_at=-1)
    reached = _drive(seg, ex, gix, pools, steps, seed=13)
    win = [r for r in reached if r[0] == 3]
    assert {r[0] for r in reached} >= {0, 2, 3}
    assert any(r[5] > 0 and r[1] == 3 for r in win), "no window run gave an item up"
    assert any(r[2] for r in win) and any(r[3] for r in win), "no filtered / growing window run"


def test_win_nofuse_resets_with_every_query_set(tuning):
    """After a give-up re-run, a new query set tries the one-launch form first."""
    seg, ex, _, _ = _corpus("A")
    gix = _index("A []", seg)
    tuning(win_force=1, fused=0)
    c = _corpus_a_dict()
    b = vb.Batch(gix, 64, 64 * 4, 10)
    for seed in (9, 40, 41):
        t, o = make_queries(c, 48, 4, seed=seed)
        b.set_queries(t, o)
        assert b.debug_route() == 3
        b.run()
        assert b.debug_win_launches() == 1, f"seed {seed}: the query set did not start on the one-launch form"
        check(ex.plain(t, o, 10), *b.fetch(), f"seed {seed}")
        if seed == 9:
            assert b.debug_counts()[1] > 0 and b.debug_win_launches() == 3, "this set is expected to give items up"


# ---- repeated one-launch merges ----

def _repeat(b, want, n, what, launches=None):
    for i in range(n):
        b.run()
        hits, nh = b.fetch()
        if launches is not None:
            assert b.debug_win_launches() == launches, f"{what} run {i}: {b.debug_win_launches()} launches"
        for q, w in enumerate(want):
            if nh[q] != len(w) or hits[q, :nh[q]].tobytes() != w.tobytes():
                check([w], hits[q:q + 1], nh[q:q + 1], f"{what} run {i} q{q}")


REPEATS = 40


@pytest.mark.parametrize("k", [10, 100])
def test_repeated_one_launch_merges_across_workgroups(tuning, k):
    """1.5 M documents, one item per window: every query has more items than a workgroup has waves, so its lists are handed from
    workgroup to workgroup through the counter of the in-kernel merge.  40 runs, each against the oracle."""
    def make():
        seg = vb.Segment.synth(1_500_000, 33_000, mean_len=100, len_mode=1, seed=11)
        return seg, Expect(seg), vb.GpuIndex(seg), bench_queries(seg, 33_000, 64, 5, seed=12)
    seg, ex, gix, (t, o) = _cached("big", make)
    tuning(fused=0, win_skew=0, win_items=100_000)
    b = vb.Batch(gix, 64, len(t), k)
    b.set_queries(t, o)
    assert b.debug_route() == 3
    want = ex.plain(t, o, k)
    b.run()
    check(want, *b.fetch(), "first run")
    items, failed = b.debug_counts()
    assert b.debug_win_launches() == 1 and failed == 0 and items // 64 >= 17, (b.debug_win_launches(), items, failed)
    _repeat(b, want, REPEATS, f"k={k}", launches=1)


def test_repeated_runs_c3_layout_one_launch_range_and_growing(tuning):
    """The C3 layout scaled down (1024 queries: a query's three runs in one workgroup), the one-launch scan_range_kernel route and a
    window batch with a growing segment: 40 runs each on one batch object."""
    seg, ex, _, _ = _corpus("C3")
    gix = _index("C3 []", seg)
    tuning(fused=0)
    t, o = bench_queries(seg, 33_000, 1024, 5, seed=3)
    b = vb.Batch(gix, 1024, len(t), 10)
    b.set_queries(t, o)
    assert b.debug_route() == 3
    _repeat(b, ex.plain(t, o, 10), REPEATS, "C3 layout", launches=1)
    assert b.debug_counts() == (1024 * 3, 0)

    t2, o2 = t[:o[200]], o[:201]
    G, _ = make_growing(seg.arrays()["term_key"], 5000, seed=8, pool=t2, pool_p=0.5)
    bg = vb.Batch(gix, 200, len(t2), 10)
    bg.set_growing(vb.GrowingSegment(gix, **G))
    bg.set_queries(t2, o2)
    assert bg.debug_route() == 3
    _repeat(bg, ex.growing(t2, o2, 10, G), REPEATS, "growing", launches=3)

    segA, exA, set_a, _ = _corpus("A")
    vb.reset_tuning()
    t3, o3 = _head(set_a, 4)
    b1 = vb.Batch(_index("A []", segA), 4, len(t3), 10)
    b1.set_queries(t3, o3)
    assert b1.debug_route() == 1
    _repeat(b1, exA.plain(t3, o3, 10), REPEATS, "one-launch range")
