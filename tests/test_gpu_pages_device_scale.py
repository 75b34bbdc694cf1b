"""The device reader (vbm25_device_segment_from_pages, csrc/pages_device.hip) where only the device path has code of its own: tapes
of more than one chunk of 1024 pages, more than one grid-stride pass of its kernels (2048 workgroups: 8192 pages, 524 288 tokens),
block bodies of every length, several errors in one relation, illegal parameters together with damage, a walk that fails with
uploads in flight, calls from several threads, the `device` argument, and every sealed route on the segment it makes.

The yardstick of every assertion is the host reader (vbm25_segment_from_pages) or the test's own construction, never the device
reader.  Every damaged relation read here is first refused (or accepted) by the host reader; tests/test_pages_device_host.py runs
the chunked ones through the same per-tuple functions under AddressSanitizer on the CPU.  The relations' lengths are asserted
there too.  -m gpu only."""
import ctypes as C
import threading

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import pages_device_data as D
from corpus import make_queries
from test_gpu_growing_filter import ROUTES
from test_gpu_pages_device import assert_device_equals_host, assert_same_segment, cached, rel3000

pytestmark = pytest.mark.gpu


def rel800():
    def make():
        c, seg, oix, pages = D.relation(n_docs=800, vocab=100)
        return [p.copy() for p in D.page_list(pages)]
    return cached("800", make)


def big540():
    return cached("540000", lambda: D.single_posting_relation(540_000))


def device_error(pl, **kw):
    with pytest.raises(vb.Vbm25Error) as e:
        vb.DeviceSegment.from_pages(pl, **kw)
    return e.value.code, str(e.value)


def assert_query_bytes(ds, want):
    """the host members of the device segment (term_df, term_first_block, bytes per token): the first, the last and a middle term"""
    for t in (0, ds.n_terms // 2, ds.n_terms - 1):
        terms = np.array([t], np.uint32)
        assert ds.query_bytes(terms, 10) == want.query_bytes(terms, 10), t
    terms = np.array([0, ds.n_terms // 2, ds.n_terms - 1], np.uint32)
    assert ds.query_bytes(terms, 10) == want.query_bytes(terms, 10)


# ---- 1. byte identity at scale

def test_three_tapes_of_more_than_one_chunk_and_a_second_pass_over_the_tokens():
    """540 000 terms of one posting: 3 / 2390 / 1856 / 2390 pages, so the tokens and blocks tapes lie in three chunks and the
    summaries in two; term_kernel and gather_kernel take a second grid-stride pass"""
    seg, pl = big540()
    ds, want = assert_device_equals_host(pl)
    assert_same_segment(want, seg)
    assert_query_bytes(ds, want)


def test_tapes_of_more_than_one_pass_of_the_page_kernels():
    """1 860 000 terms of one posting: 8231 token and block pages, more than 2048 workgroups x 4 waves take in one pass (187 MB of
    pages, nine chunks per tape)"""
    seg, pl = D.single_posting_relation(1_860_000)
    ds, want = assert_device_equals_host(pl)
    assert_same_segment(want, seg)
    assert_query_bytes(ds, want)


def test_every_body_length_and_a_documents_tape_of_two_chunks():
    """wide_relation(): bit-packed bodies of document width 1..20 and tf width 1..31, byte-packed tails of 1..127 postings with every
    byte width the size allows (lengths that are no multiple of 8: copy_lane's partial reads; up to 102 units of 8 bytes: its unit loop),
    1550 document pages.  The achieved widths are asserted on the host reader's segment; then the index of the device segment answers
    as the index of the host segment does: every width-term alone and with the term that meets them all, every tail alone."""
    seg, pl, expect = D.wide_relation()
    ds, want = assert_device_equals_host(pl)
    assert_same_segment(want, seg)
    D.check_wide_widths(want, expect)
    assert_query_bytes(ds, want)
    mixed = 40
    terms, off = [], [0]
    for t in range(mixed):
        terms += [t]
        off.append(len(terms))
        terms += [t, mixed]
        off.append(len(terms))
    for t in range(mixed + 1, ds.n_terms):
        terms += [t]
        off.append(len(terms))
    terms, off = np.array(terms, np.uint32), np.array(off, np.uint32)
    h0, n0 = vb.search_batch(vb.GpuIndex(want), terms, off, 10)
    h1, n1 = vb.search_batch(vb.GpuIndex(ds), terms, off, 10)
    assert int(n0.min()) > 0 and np.array_equal(n0, n1) and h0.tobytes() == h1.tobytes()


# ---- 2. damage beyond chunk 0 and beyond the first grid-stride pass

def test_damage_in_later_chunks_and_later_passes():
    """chunk_damage on the 540 000-term relation: the host reader's code; for line-pointer, block-pointer and block-header damage the
    host reader's text and page id too (both name the page that holds the tuple: error_page through a prefix of 2390 entries)"""
    seg, pl = big540()
    for name, kind, pages, edit, where in D.chunk_damage(pl):
        cp = D.damaged(pl, pages, edit)
        code, text = D.host_error(cp)
        assert code == -2, name
        got_code, got_text = device_error(cp)
        assert got_code == code and "data corruption" in got_text, (name, got_text)
        if kind == "message":
            assert got_text == text, name
    assert_device_equals_host(rel3000()[2])


def test_a_walk_that_fails_with_uploads_in_flight():
    """the callable form, a page in the third chunk of the blocks tape cannot be read: the chunks of the other tapes and two of this
    one are on their way up when the walk ends"""
    seg, pl = big540()
    (docs, toks, sums, blks), _ = D.tapes(pl)
    bad = blks[2 * D.CHUNK_PAGES + 100]
    address = [p.ctypes.data for p in pl]
    read = lambda i: None if i == bad or i >= len(address) else address[i]
    code, text = D.host_error(read)
    assert (code, text) == (-2, f"vbm25 error -2: data corruption: page cannot be read (page {bad})")
    assert device_error(read) == (code, text)
    assert_device_equals_host(rel3000()[2])


# ---- 3. several errors at once

def test_the_first_error_in_walk_order_is_the_one_reported():
    seg, pages, pl = rel3000()
    for name, pgs, edits, text, page in D.paired_damage(pl):
        cp = D.damaged(pl, pgs, *edits)
        want = D.host_error(cp)
        assert want == (-2, f"vbm25 error -2: data corruption: {text} (page {page})"), name
        assert device_error(cp) == want, name
    assert_device_equals_host(pl)


# ---- 4. the order of the verdict

@pytest.mark.parametrize("params", [dict(k1=3.0), dict(b=1.5)], ids=["k1", "b"])
def test_illegal_parameters_with_damage(params):
    """structure -> empty index -> k1 / b (VBM25_ERR_INVALID) -> arrays -> key order: the host reader's code case by case (its table
    is asserted in tests/test_pages_device_host.py: -1 for the undamaged relation and four cases, -2 for fifteen)"""
    pl = rel800()
    assert D.host_error(D.damaged(pl, [0], D.set_params(**params)))[0] == -1
    assert device_error(D.damaged(pl, [0], D.set_params(**params)))[0] == -1
    codes = []
    for name, edit in D.named_damage(pl):
        cp = [p.copy() for p in pl]
        edit(cp)
        D.set_params(**params)(cp)
        code, _ = D.host_error(cp)
        assert code == (-1 if name in D.ARRAY_LEVEL_DAMAGE else -2), name
        assert device_error(cp)[0] == code, name
        codes.append(code)
    assert (codes.count(-1), codes.count(-2)) == (4, 15)
    empty = D.empty_relation()
    D.set_params(**params)(empty)
    ds, want = assert_device_equals_host(empty)
    assert ds.n_docs == 0 and want.meta()[next(iter(params))] == next(iter(params.values()))
    assert_device_equals_host(pl)


# ---- 5. every sealed route

def rel12000():
    def make():
        c, seg, oix, pages = D.relation(n_docs=12000, vocab=600, seed=2)
        pl = D.page_list(pages)
        return c, vb.GpuIndex(vb.segment_from_pages(pl)), vb.GpuIndex(vb.DeviceSegment.from_pages(pl))
    return cached("12000", make)


@pytest.mark.parametrize("case,tune,k,nterms,nq,route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_sealed_route_on_the_device_segment(tuning, case, tune, k, nterms, nq, route):
    """The route table of tests/test_gpu_growing_filter.py with its tuning switches, on the index of DeviceSegment.from_pages: the
    expected route is taken and the records are byte for byte those of the index of segment_from_pages (which takes the same route).
    Every term of this relation is in about 6 % of the 12 000 documents, so a query of four terms is dense by the default threshold
    (100 postings per 1000 documents) and scan_dense_kernel would serve it whatever the switches -- also in the cases that expect
    route 0 for sparse queries (plan_range, many_k1024), which would then pass on the dense kernel's route 0.  So every case whose
    switches do not set the threshold themselves (dense_k10 sets 0) raises it out of reach (dense_x1000 = 10^9, as the other suites
    do), and the classes the host gave the queries are asserted: none dense, or in dense_k10 all of them."""
    c, host, dev = rel12000()
    tune = dict(tune)
    tune.setdefault("dense_x1000", 10 ** 9)
    tuning(**tune)
    terms, off = make_queries(c, nq, nterms, seed=nq + k + nterms)
    got = []
    for ix in (host, dev):
        b = vb.Batch(ix, nq, len(terms), k)
        b.set_queries(terms, off)
        assert b.debug_route() == route, f"{case}: route {b.debug_route()} instead of {route}"
        b.run()
        if k <= 1024:   # (the exhaustive route of k > 1024 does not class its queries)
            assert b.debug_routes()[1] == (nq if tune["dense_x1000"] == 0 else 0), f"{case}: {b.debug_routes()}"
        got.append(b.fetch())
    (h0, n0), (h1, n1) = got
    assert int(n0.min()) > 0 and np.array_equal(n0, n1) and h0.tobytes() == h1.tobytes()


# ---- 6. the device argument, threads, a stream at work

def test_a_device_out_of_range_is_invalid():
    import torch
    seg, pages, pl = rel3000()
    for device in (-1, torch.cuda.device_count()):
        code, text = device_error(pl, device=device)
        assert code == -1 and "out of range" in text, (device, text)
    assert_device_equals_host(pl)


def test_the_second_device():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    seg, pages, pl = rel3000()
    assert_same_segment(vb.DeviceSegment.from_pages(pl, device=1).download(), vb.segment_from_pages(pl))
    assert_device_equals_host(pl)


def pages_device_stats():
    f = vb.lib().vbm25_debug_pages_device_stats
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    out = np.zeros(4, np.float64)
    assert f(out.ctypes.data_as(C.c_void_p)) == 0
    return out


def expected_bytes_up(pl):
    """what the call sends up: the tapes' page images, and per tape a pointer per chunk of 1024 pages, a page id and a prefix count
    per page and one more prefix count"""
    total = 0
    for tape in D.tapes(pl)[0]:
        total += 8192 * len(tape) + 8 * (-(-len(tape) // D.CHUNK_PAGES)) + 8 * len(tape) + 4
    return total


def test_four_threads_each_get_their_own_result():
    """three valid relations (800, 1500 and 3000 documents) and a damaged copy of the first, read at once from four threads of one
    process: each thread has its own segment or its own error, and the statistics of its own call"""
    pl800, pl3000 = rel800(), rel3000()[2]
    pl1500 = cached("damage", D.damage_relation)
    name, edit = D.named_damage(pl800)[9]
    assert name == "a line pointer with flags != 1"
    bad = [p.copy() for p in pl800]
    edit(bad)
    want_error = D.host_error(bad)
    assert want_error[0] == -2
    jobs = [pl800, pl1500, pl3000, bad]
    wants = [vb.segment_from_pages(p) for p in jobs[:3]]
    assert len({w.n_docs for w in wants}) == 3
    out = [None] * 4
    start = threading.Barrier(4)

    def work(i):
        try:
            start.wait()
            ds = vb.DeviceSegment.from_pages(jobs[i])
            out[i] = ("ok", ds, pages_device_stats())
        except vb.Vbm25Error as e:
            out[i] = ("error", (e.code, str(e)), None)
        except BaseException as e:  # (a thread's exception must not vanish)
            out[i] = ("raised", repr(e), None)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(3):
        kind, ds, stats = out[i]
        assert kind == "ok", out[i]
        assert_same_segment(ds.download(), wants[i])
        assert stats[1] == expected_bytes_up(jobs[i]), i
    assert len({out[i][2][1] for i in range(3)}) == 3
    assert out[3] == ("error", want_error, None)


def test_a_read_while_a_stream_has_batches_in_flight():
    c, host, dev = rel12000()
    seg, pages, pl = rel3000()
    batches = [make_queries(c, 16, 4, seed=s) for s in (1, 2, 3)]
    want = [vb.search_batch(dev, terms, off, 10) for terms, off in batches]
    st = vb.Stream(dev, 3, 16, max(len(t) for t, _ in batches), 10)
    for terms, off in batches:
        st.submit(terms, off)
    assert st.in_flight == 3
    ds = vb.DeviceSegment.from_pages(pl)
    for h0, n0 in want:
        h1, n1 = st.collect()
        assert int(n0.sum()) > 0 and np.array_equal(n0, n1) and h0.tobytes() == h1.tobytes()
    assert_same_segment(ds.download(), vb.segment_from_pages(pl))
