"""The device reader of the growing segment (vbm25_device_growing_from_pages, csrc/pages_device.hip + csrc/vectors_parse.h): the
vectors tape of a relation in the reference's on-disk format read on the device into a device growing segment.  The yardstick is
the host composition vbm25_growing_from_pages + vbm25_growing_upload: the CSR that comes back is byte for byte the host reader's,
every search through the new segment returns the records of one through the composed segment, what the composition refuses is
refused with its code (and, for one damage, its message and page), and the segment is an ordinary one afterwards.  -m gpu only.

Out-of-bounds reads are not hunted here: tests/test_vectors_device_host.py runs the same lane functions under AddressSanitizer on
the CPU, on the relations and the damage of this file."""
import ctypes as C
import threading

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import pages_device_data as D
import vectors_device_data as V
from corpus import make_queries
from growing_data import make_growing

pytestmark = pytest.mark.gpu
KS = (1, 10, 256, 1500)
_C = {}


def cached(name, make):
    if name not in _C:
        _C[name] = make()
    return _C[name]


def interleaved():
    """(corpus, sealed segment as the host reader flattens it, its index, page list, the host reader's CSR)"""
    def make():
        c, seg, pl = V.interleaved_relation()
        flat = vb.segment_from_pages(pl)
        return c, flat, vb.GpuIndex(flat), pl, vb.growing_from_pages(pl)
    return cached("inter", make)


def empty_sealed(name, pages_of_tuples):
    def make():
        pl = V.hand_relation(pages_of_tuples)
        flat = vb.segment_from_pages(pl)
        return flat, vb.GpuIndex(flat), pl, vb.growing_from_pages(pl)
    return cached(name, make)


def interleaved_queries(c, seg):
    """1 to 8 terms and a 20-term query over the corpus, the terms of the documents that exist in both segments (ties), and ids the
    sealed vocabulary lacks at the end of a query"""
    n_terms = seg.n_terms
    rows = []
    for nterms in (1, 2, 3, 4, 5, 6, 7, 8, 20):
        t, o = make_queries(c, 2, nterms, seed=40 + nterms)
        rows += [np.unique(t[o[q]:o[q + 1]]) for q in range(2)]
    rows += V.tie_queries(seg)   # queries 18, 19, 20
    rows.append(np.r_[rows[4], np.uint32(n_terms + 3), np.uint32(0xFFFFFFFF)].astype(np.uint32))
    terms = np.concatenate(rows).astype(np.uint32)
    off = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint32)
    return terms, off


def assert_same_records(gix, gs, ref, terms, off, k, what):
    hits, nh = vb.search_batch_growing(gix, gs, terms, off, k)
    want, wn = vb.search_batch_growing(gix, ref, terms, off, k)
    assert nh.tobytes() == wn.tobytes(), f"{what} k={k}: counts differ"
    for q in range(len(nh)):
        assert hits[q, :nh[q]].tobytes() == want[q, :wn[q]].tobytes(), f"{what} k={k} q{q}: records differ"
    return hits, nh


# ---- 1. byte for byte

def test_interleaved_relation_csr_and_records():
    c, seg, gix, pl, want = interleaved()
    assert len(V.vectors_tape(pl)) > 3 and want["g_deleted"].sum() == 5
    gs, csr = vb.GrowingSegment.from_pages(gix, pl, return_csr=True)
    V.assert_same_csr(csr, want, "interleaved")
    assert gs.n_docs == len(want["g_start"]) - 1 == 303 and gs.device_bytes > 0
    ref = vb.GrowingSegment.from_dict(gix, want)
    terms, off = interleaved_queries(c, seg)
    grow_hits = 0
    for k in KS:
        hits, nh = assert_same_records(gix, gs, ref, terms, off, k, "interleaved")
        grow_hits += sum(int((hits[q, :nh[q]]["doc_id"] > 0xFFFFFFFF - gs.n_docs).sum()) for q in range(len(nh)))
        if k == 1500:
            # ties across the segments: the copy of a sealed document scores what the document scores
            for i, d in enumerate(V.TIE_DOCS):
                q = 18 + i
                h = hits[q, :nh[q]]
                s = h["score"][h["doc_id"] == d]
                g = h["score"][h["doc_id"] == 0xFFFFFFFF - (300 + i)]
                assert len(s) == 1 and len(g) == 1 and s[0] == g[0], (d, s, g)
    assert grow_hits > 0
    # deleted growing documents are in no record
    deleted = 0xFFFFFFFF - np.flatnonzero(want["g_deleted"]).astype(np.uint64)
    hits, nh = vb.search_batch_growing(gix, gs, terms, off, 1500)
    assert not any(np.isin(hits[q, :nh[q]]["doc_id"], deleted).any() for q in range(len(nh)))
    # without the CSR nothing else changes; the callable form of `pages`
    gs2 = vb.GrowingSegment.from_pages(gix, lambda i: pl[i].ctypes.data if i < len(pl) else None)
    assert_same_records(gix, gs2, ref, terms, off, 10, "no csr, callable pages")


@pytest.mark.parametrize("shape", ["hand-made tape", "tape without tuples", "golden fixture"])
def test_other_shapes(shape):
    if shape == "golden fixture":
        import os
        raw = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "page_fixture.bin"), "rb").read()
        pl = [np.frombuffer(raw[i:i + 8192], np.uint8).copy() for i in range(0, len(raw), 8192)]
        seg = vb.segment_from_pages(pl)
        gix, want = vb.GpuIndex(seg), vb.growing_from_pages(pl)
    else:
        tapes = {name: t for name, t, _ in V.hand_tapes()}
        tuples = tapes["a tape of pages without tuples"] if shape == "tape without tuples" else \
            tapes["a document of 1000 elements across three pages"] + tapes["a _2 followed by a _2: a dropped attempt with _1 tuples in it"] + \
            tapes["documents of 0 elements"] + tapes["a trailing _2 without a _0"]
        seg, gix, pl, want = empty_sealed(shape, tuples)
        assert seg.n_docs == 0
    gs, csr = vb.GrowingSegment.from_pages(gix, pl, return_csr=True)
    V.assert_same_csr(csr, want, shape)
    assert gs.n_docs == len(want["g_start"]) - 1 and (gs.n_docs == 0) == (shape == "tape without tuples")
    ref = vb.GrowingSegment.from_dict(gix, want)
    if seg.n_terms:   # (the fixture has two terms)
        terms, off = np.array([0, 1, 0, 3, 1], np.uint32), np.array([0, 2, 4, 5, 5], np.uint32)
    else:
        terms, off = np.array([1, 0xFFFFFFFF], np.uint32), np.array([0, 1, 2, 2], np.uint32)
    for k in KS:
        assert_same_records(gix, gs, ref, terms, off, k, shape)


# ---- 2. an ordinary segment afterwards

def test_append_delete_filter_and_stream_on_the_new_segment():
    c, seg, gix, pl, want = interleaved()
    gs = vb.GrowingSegment.from_pages(gix, pl)
    ref = vb.GrowingSegment.from_dict(gix, want)
    terms, off = interleaved_queries(c, seg)
    nq = len(off) - 1
    G, _ = make_growing(seg.arrays()["term_key"], 50, seed=6, pool=terms[terms < seg.n_terms])
    for s in (gs, ref):
        s.append(**G)
    assert gs.n_docs == ref.n_docs == 353
    for k in (10, 1500):
        assert_same_records(gix, gs, ref, terms, off, k, "after append")
    gone = np.array([1, 2, 300, 310, 352], np.uint32)
    for s in (gs, ref):
        s.delete(gone)
    hits, nh = assert_same_records(gix, gs, ref, terms, off, 1500, "after delete")
    assert not any(np.isin(hits[q, :nh[q]]["doc_id"], 0xFFFFFFFF - gone.astype(np.uint64)).any() for q in range(nq))
    # filters: one sealed and one growing bitmap per query
    rng = np.random.default_rng(8)
    keeps, gkeeps = rng.random((nq, seg.n_docs)) < 0.5, rng.random((nq, gs.n_docs)) < 0.5
    sel = np.arange(nq, dtype=np.uint32)
    sel[3] = vb.NO_FILTER
    out = []
    for s in (gs, ref):
        f = vb.DocFilter(gix, keeps)
        f.set_growing(s, gkeeps)
        out.append(vb.search_batch_growing_masked(gix, s, terms, off, 100, f, sel))
    assert out[0][1].tobytes() == out[1][1].tobytes() and out[0][0].tobytes() == out[1][0].tobytes()
    kept_ids = [set((0xFFFFFFFF - np.flatnonzero(gkeeps[q])).tolist()) | set(np.flatnonzero(keeps[q]).tolist()) for q in range(nq)]
    assert all(set(out[0][0][q, :out[0][1][q]]["doc_id"].tolist()) <= kept_ids[q] for q in range(nq) if q != 3)
    # the pipelined ring
    got = []
    for s in (gs, ref):
        st = vb.Stream(gix, 2, nq, len(terms), 10)
        st.set_growing(s)
        st.submit(terms, off)
        st.submit(terms, off)
        got.append([st.collect(), st.collect()])
    for (h, n), (wh, wn) in zip(got[0], got[1]):
        assert n.tobytes() == wn.tobytes() and all(h[q, :n[q]].tobytes() == wh[q, :wn[q]].tobytes() for q in range(nq))
    one, n_one = vb.search_batch_growing(gix, gs, terms, off, 10)
    assert all(got[0][0][0][q, :n_one[q]].tobytes() == one[q, :n_one[q]].tobytes() for q in range(nq))


# ---- 3. past one chunk and one grid pass

def test_tape_past_a_chunk_and_a_grid_pass():
    """one tape of more pages than a chunk holds (CHUNK_PAGES) and than one grid-stride pass of the wave-per-page kernels covers
    (MAX_GRID workgroups of 4 waves), with documents that straddle every page boundary, pages without tuples and dropped attempts;
    and a page of 400 _2 tuples (more slots than a wave has lanes)"""
    seg, gix, pl, want = empty_sealed("long", V.long_tape(V.PAGES_PER_PASS + 70) + V.only_starts_tape())
    assert len(V.vectors_tape(pl)) > V.PAGES_PER_PASS > V.CHUNK_PAGES and len(want["g_start"]) - 1 > V.PAGES_PER_PASS - 300
    gs, csr = vb.GrowingSegment.from_pages(gix, pl, return_csr=True)
    V.assert_same_csr(csr, want, "long tape")
    assert csr["g_fieldnorm"][-1] == 399 % 256 and csr["g_tf"][-3:].tolist() == [1, 2, 3]
    ref = vb.GrowingSegment.from_dict(gix, want)
    assert_same_records(gix, gs, ref, np.array([0, 5], np.uint32), np.array([0, 1, 2], np.uint32), 10, "long tape")


# ---- 4. refusals

def composition_error(gix, pl):
    """(code, message) of the host composition's refusal"""
    try:
        vb.GrowingSegment.from_dict(gix, vb.growing_from_pages(pl))
    except vb.Vbm25Error as e:
        return e.code, str(e)
    raise AssertionError("the host composition accepts the relation")


def raw_read(gix, pl):
    """(code, message, *out, *csr) of the C call"""
    cb, keep = vb.api._page_reader(pl)
    out, csr = C.c_void_p(1), C.c_void_p(1)
    rc = vb.lib().vbm25_device_growing_from_pages(gix.h, C.cast(cb, C.c_void_p), None, C.byref(out), C.byref(csr))
    return rc, f"vbm25 error {rc}: " + vb.lib().vbm25_last_error().decode(), out.value, csr.value


def assert_refused_like_the_composition(gix, pl, name, message=True):
    code, msg = composition_error(gix, pl)
    rc, got, out, csr = raw_read(gix, pl)
    assert rc == code and not out and not csr, (name, rc, got, code, msg)
    if message:
        assert got == msg, (name, got, msg)
    return code


def assert_still_serves(gix, pl, want, terms, off):
    gs, csr = vb.GrowingSegment.from_pages(gix, pl, return_csr=True)
    V.assert_same_csr(csr, want, "a good read after a refusal")
    hits, nh = vb.search_batch_growing(gix, gs, terms, off, 10)
    assert nh.sum() > 0


def test_refusals_equal_the_host_composition():
    c, seg, gix, pl, want = interleaved()
    terms, off = interleaved_queries(c, seg)
    named, late = V.named_damage(pl), V.named_damage(pl, skip=5)
    cases = [(name, [edit], True) for name, edit, _ in named]
    cases += [(f"{n1} + later {n2}", [e2, e1], True) for (n1, e1, _), (n2, e2, _) in zip(named[:5], late[5:])]
    cases.append(("keys not ascending", [V.unordered_keys(pl, skip=4)[1]], True))
    cases.append(("keys not ascending twice", [V.unordered_keys(pl, skip=40)[1], V.unordered_keys(pl, skip=4)[1]], True))
    tape = V.vectors_tape(pl)
    cases.append(("special area of the last page", [D.put("<H", tape[-1], 16, 8176)], True))
    cases.append(("a page linked twice", [D.put("<I", tape[2], 8184, tape[1])], True))
    codes = set()
    for name, edits, message in cases:
        cp = [p.copy() for p in pl]
        for e in edits:
            e(cp)
        codes.add(assert_refused_like_the_composition(gix, cp, name, message))
        assert_still_serves(gix, pl, want, terms, off)
    assert codes == {-2, -1}
    # the hand-made tapes the host reader refuses, on an empty sealed segment
    seg0, gix0, pl0, want0 = empty_sealed("tape without tuples", [[], [], []])
    for name, tuples, text in V.hand_tapes():
        if text != "ok":
            assert assert_refused_like_the_composition(gix0, V.hand_relation(tuples), name) == -2
    # no vectors tape at all
    assert assert_refused_like_the_composition(gix0, V.hand_relation([]), "no vectors tape") == -2
    gs0 = vb.GrowingSegment.from_pages(gix0, pl0)
    assert gs0.n_docs == 0


def test_damage_in_a_later_chunk_and_a_page_that_cannot_be_read():
    """damage beyond chunk 0 (a tuple and, in the second grid pass, keys out of order), and a read_page that returns NULL after
    the first chunk went up: refused as the host composition refuses, and the index serves a good read afterwards"""
    seg, gix, pl, want = empty_sealed("long", V.long_tape(V.PAGES_PER_PASS + 70) + V.only_starts_tape())
    tape = V.vectors_tape(pl)
    p = tape[V.CHUNK_PAGES + 10]
    assert assert_refused_like_the_composition(gix, D.damaged(pl, [p], D.put("<Q", p, D.slots(pl[p])[1][0], 3)), "tag 3 in chunk 1") == -2
    # a kept _1 of two elements or more beyond the first grid pass: its first key becomes the largest there is
    at = next(i for i in range(V.PAGES_PER_PASS + 20, len(tape)) if i % 50 != 49 and D.slots(pl[tape[i]]) and D.slots(pl[tape[i]])[-1][1] >= 16 + 40)
    p = tape[at]
    off, size = D.slots(pl[p])[-1]
    cp = D.damaged(pl, [p], D.put("<16s", p, off + 16, b"\xff" * 16))
    code, msg = composition_error(gix, cp)
    rc, got, out, csr = raw_read(gix, cp)
    assert (rc, got) == (code, msg) and code == -1 and "strictly ascending" in msg and not out and not csr
    # NULL in the middle of the walk, uploads in flight
    stop = tape[V.CHUNK_PAGES + 500]
    reader = lambda i: None if i == stop else (pl[i].ctypes.data if i < len(pl) else None)
    with pytest.raises(vb.Vbm25Error) as e:
        vb.GrowingSegment.from_pages(gix, reader)
    with pytest.raises(vb.Vbm25Error) as e_host:
        vb.growing_from_pages(reader)
    assert (e.value.code, str(e.value)) == (e_host.value.code, str(e_host.value)) and f"page cannot be read (page {stop})" in str(e.value)
    gs, csr = vb.GrowingSegment.from_pages(gix, pl, return_csr=True)
    V.assert_same_csr(csr, want, "after the refusals")


# ---- 5. concurrency

def test_four_threads_and_a_stream_in_flight():
    c, seg, gix, pl, want = interleaved()
    terms, off = interleaved_queries(c, seg)
    nq = len(off) - 1
    ref = vb.GrowingSegment.from_dict(gix, want)
    results, errors = [None] * 4, []

    def work(i):
        try:
            results[i] = vb.GrowingSegment.from_pages(gix, pl, return_csr=True)
        except Exception as e:   # noqa: BLE001 -- reported below, in the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, (gs, csr) in enumerate(results):
        V.assert_same_csr(csr, want, f"thread {i}")
        assert_same_records(gix, gs, ref, terms, off, 10, f"thread {i}")
    # a read beside a stream with batches in flight
    st = vb.Stream(gix, 3, nq, len(terms), 10)
    st.set_growing(ref)
    for _ in range(3):
        st.submit(terms, off)
    gs, csr = vb.GrowingSegment.from_pages(gix, pl, return_csr=True)
    V.assert_same_csr(csr, want, "beside the stream")
    one, n_one = vb.search_batch_growing(gix, ref, terms, off, 10)
    for _ in range(3):
        h, n = st.collect()
        assert n.tobytes() == n_one.tobytes() and all(h[q, :n[q]].tobytes() == one[q, :n[q]].tobytes() for q in range(nq))
    assert_same_records(gix, gs, ref, terms, off, 10, "beside the stream")
