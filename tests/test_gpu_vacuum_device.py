"""VACUUM's inputs read and consumed on the device: vbm25_device_vacuum_from_pages (csrc/pages_device.hip), vbm25_index_maintain_device
and vbm25_filter_remap_device (csrc/maintain.hip).  The yardstick everywhere is the host-input route on the same pages: the host
readers' outputs (vbm25_sealed_deleted_from_pages, vbm25_growing_from_pages) fed to DeviceSegment.maintain and DocFilter.remap.  The
new route is never compared against itself.  -m gpu only.

Out-of-bounds reads are not hunted here: tests/test_vacuum_device_host.py runs the flag function and the word packing under
AddressSanitizer on the CPU, on the relations and the damage of this file."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import pages_device_data as D
import vectors_device_data as V
import vacuum_device_data as X
from corpus import make_queries

pytestmark = pytest.mark.gpu
INVALID, CORRUPT, UNSUPPORTED = -1, -2, -4
_C = {}


def cached(name, make):
    if name not in _C:
        _C[name] = make()
    return _C[name]


def base():
    """(corpus, the sealed segment as the host reader flattens it, its index, page list, (page, offset) per document, documents per
    page, the flag patterns) of vacuum_relation()"""
    def make():
        c, seg, pl = X.vacuum_relation()
        flat = vb.segment_from_pages(pl)
        where, per_page = X.doc_slots(pl)
        assert per_page == [680, 680, 680, 680, 280]
        return c, flat, vb.GpuIndex(flat), pl, where, per_page, X.flag_patterns(flat.n_docs, per_page)
    return cached("base", make)


def small(n):
    def make():
        seg, pl = X.small_relation(n)
        flat = vb.segment_from_pages(pl)
        return flat, vb.GpuIndex(flat), pl
    return cached(("small", n), make)


def host_inputs(pl):
    """the host readers' outputs: (n_docs, n_deleted, words, the growing CSR)"""
    n, n_del, words = X.host_flags(pl)
    return n, n_del, words, vb.growing_from_pages(pl)


def assert_same_inputs(dv, pl, what):
    """the handle's counts and deletion inputs equal the host readers'; returns the host readers' outputs"""
    n, n_del, words, csr = host_inputs(pl)
    got_words, got_gdel = dv.read()
    assert (dv.n_sealed, dv.n_sealed_deleted) == (n, n_del), (what, dv.n_sealed, dv.n_sealed_deleted, n, n_del)
    assert got_words.dtype == np.uint64 and got_words.tobytes() == words.tobytes(), f"{what}: words differ at {np.flatnonzero(got_words != words)[:8]}"
    if n % 64:
        assert int(got_words[-1]) >> (n % 64) == 0, f"{what}: bits beyond n_docs"
    assert dv.n_grow == len(csr["g_start"]) - 1 and dv.n_elements == len(csr["g_tf"]), what
    assert got_gdel.tobytes() == np.asarray(csr["g_deleted"], np.uint8).tobytes() and dv.n_grow_deleted == int((csr["g_deleted"] != 0).sum()), what
    return words, csr


def assert_same_segment(got, want, what):
    """two DeviceSegments: download() arrays byte for byte"""
    a, b = got.download(), want.download()
    assert a.meta() == b.meta(), (what, a.meta(), b.meta())
    x, y = a.arrays(), b.arrays()
    assert sorted(x) == sorted(y)
    for name in y:
        assert x[name].dtype == y[name].dtype and x[name].tobytes() == y[name].tobytes(), f"{what}: {name} differs"
    return a


def compact_both(gix, pl, what):
    """the handle, its compaction and the host-input route's: segments and relabel equal"""
    dv = vb.DeviceVacuum.from_pages(gix, pl)
    words, csr = assert_same_inputs(dv, pl, what)
    want, want_relabel = vb.DeviceSegment.maintain(gix, words, csr, return_relabel=True)
    got, relabel = vb.DeviceSegment.maintain_device(gix, dv, return_relabel=True)
    flat = assert_same_segment(got, want, what)
    assert relabel.tobytes() == want_relabel.tobytes(), f"{what}: relabel differs"
    return dv, got, want, flat, words, csr


def raw_vacuum(gix, pl):
    """(code, message, *out) of the C call"""
    cb, keep = vb.api._page_reader(pl)
    out = C.c_void_p(1)
    rc = vb.lib().vbm25_device_vacuum_from_pages(gix.h, C.cast(cb, C.c_void_p), None, C.byref(out))
    return rc, f"vbm25 error {rc}: " + vb.lib().vbm25_last_error().decode(), out.value


def error_of(fn):
    with pytest.raises(vb.Vbm25Error) as e:
        fn()
    return e.value.code, str(e.value)


# ---- 1. flags, sealed only

@pytest.mark.parametrize("pattern", ["none", "all", "document 0 only", "the last document only", "every 64th", "every 63rd", "every 65th",
                                     "the 40 documents around each page boundary", "a random half"])
def test_flags_on_five_pages(pattern):
    """3000 documents on pages of 680, 680, 680, 680 and 280 tuples: a wave makes 11 rounds per full page and the words straddle every
    page boundary.  Flag bytes 1, 2, 0x80 and 0xFF all count as deleted."""
    c, seg, gix, pl, where, per_page, patterns = base()
    flags = patterns[pattern]
    cp = X.with_flags(pl, where, flags)
    dv = vb.DeviceVacuum.from_pages(gix, cp)
    words, csr = assert_same_inputs(dv, cp, pattern)
    assert words.tobytes() == X.packed(flags).tobytes() and dv.n_sealed_deleted == int((flags != 0).sum())
    if pattern == "all":
        assert set(np.unique(flags).tolist()) == set(X.FLAG_BYTES)


@pytest.mark.parametrize("n_docs", X.SMALL_DOC_COUNTS)
def test_flags_of_small_document_counts(n_docs):
    seg, gix, pl = small(n_docs)
    where, per_page = X.doc_slots(pl)
    assert seg.n_docs == n_docs == sum(per_page)
    for name, flags in X.flag_patterns(n_docs, per_page, seed=n_docs).items():
        cp = X.with_flags(pl, where, flags)
        dv = vb.DeviceVacuum.from_pages(gix, cp)
        words, _ = assert_same_inputs(dv, cp, f"{n_docs}: {name}")
        assert words.tobytes() == X.packed(flags).tobytes()
        assert dv.n_grow == 0 and dv.n_elements == 0


def test_the_empty_relation_and_read_page_once_per_page():
    # empty_relation() has no vectors tape, which the reader of the growing segment refuses; with a tape of one page without tuples
    # it is the relation of an index whose table is empty
    pl0 = D.empty_relation()
    flat = vb.segment_from_pages(pl0)
    gix0 = vb.GpuIndex(flat)
    code, msg = error_of(lambda: vb.growing_from_pages(pl0))
    assert raw_vacuum(gix0, pl0) == (code, msg, None) and "no vectors tape" in msg
    pl = V.hand_relation([[]])
    dv = vb.DeviceVacuum.from_pages(gix0, pl)
    words, csr = assert_same_inputs(dv, pl, "empty")
    assert (dv.n_sealed, dv.n_sealed_deleted, dv.n_grow, dv.n_grow_deleted, dv.n_elements) == (0, 0, 0, 0, 0) and len(words) == 0
    got = vb.DeviceSegment.maintain_device(gix0, dv)
    assert_same_segment(got, vb.DeviceSegment.maintain(gix0, words, csr), "empty")
    assert got.n_docs == 0
    # Meta, Jump and every page of the two tapes are read once, and no other page
    c, seg, gix, pl, where, per_page, patterns = base()
    calls = []

    def reader(i):
        calls.append(i)
        return pl[i].ctypes.data if i < len(pl) else None
    vb.DeviceVacuum.from_pages(gix, reader)
    (docs, _, _, _), (ptr_jump, _) = D.tapes(pl)
    assert sorted(calls) == sorted([0, ptr_jump] + docs + V.vectors_tape(pl)) and calls[:2] == [0, ptr_jump]


# ---- 2. compaction equality

@pytest.mark.parametrize("pattern", ["none", "all", "document 0 only", "the last document only", "every 64th", "every 63rd", "every 65th",
                                     "the 40 documents around each page boundary", "a random half"])
def test_compaction_equals_the_host_input_route(pattern):
    """every flag pattern x growing documents deleted: none, some, all.  300 growing documents, 15 % of them with keys the sealed
    vocabulary lacks, and an unfinished insert at the tape's end."""
    c, seg, gix, pl, where, per_page, patterns = base()
    sealed = X.with_flags(pl, where, patterns[pattern])
    for gname, which in X.GROWING_DELETED.items():
        what = f"{pattern} x growing deleted: {gname}"
        cp = X.with_growing_deleted(sealed, which)
        dv, got, want, flat, words, csr = compact_both(gix, cp, what)
        assert dv.n_grow == 300 and dv.n_grow_deleted == len(which)
        assert got.n_docs == seg.n_docs - dv.n_sealed_deleted + 300 - len(which), what
        if pattern == "all" and gname == "all":
            assert got.n_docs == 0 and got.n_terms == 0 and got.n_blocks == 0   # everything deleted on both sides: the empty segment
        # the handle is only read: a second compaction gives the same bytes, and the deletion inputs read back as before
        assert_same_segment(vb.DeviceSegment.maintain_device(gix, dv), want, what + ", again")
        assert dv.read()[0].tobytes() == words.tobytes()
        if gname == "some":
            # once more as page images, and the images read back on the device
            rel = got.to_relation()
            rel_want = want.to_relation()
            assert len(rel) == len(rel_want) and all(a.tobytes() == b.tobytes() for a, b in zip(rel, rel_want)), what
            back = vb.DeviceSegment.from_pages(rel).download()
            assert back.meta() == flat.meta() and all(back.arrays()[k].tobytes() == v.tobytes() for k, v in flat.arrays().items()), what


def test_unknown_keys_become_tokens():
    c, seg, gix, pl, where, per_page, patterns = base()
    dv, got, want, flat, words, csr = compact_both(gix, pl, "nothing deleted")
    known = set(seg.arrays()["term_key"].reshape(-1, 16).view("S16").reshape(-1).tolist())
    new = set(flat.arrays()["term_key"].reshape(-1, 16).view("S16").reshape(-1).tolist()) - known
    assert len(new) > 20 and got.n_terms == seg.n_terms + len(new)


# ---- 3. filter equality

def filter_bits(kind, F, n, rng):
    return np.zeros((F, n), bool) if kind == "none" else np.ones((F, n), bool) if kind == "all" else rng.random((F, n)) < 0.5


@pytest.mark.parametrize("bits", ["none", "all", "random"])
def test_remap_equals_the_host_input_remap(bits):
    c, seg, gix, pl, where, per_page, patterns = base()
    rng = np.random.default_rng(5)
    F = 3
    cp = X.with_growing_deleted(X.with_flags(pl, where, patterns["a random half"]), X.GROWING_DELETED["some"])
    dv, got, want, flat, words, csr = compact_both(gix, cp, "remap")
    nix = vb.GpuIndex(got)
    gs = vb.GrowingSegment.from_pages(gix, cp)
    f = vb.DocFilter(gix, filter_bits(bits, F, seg.n_docs, rng))
    f.set_growing(gs, filter_bits(bits, F, 300, rng))
    want_f = f.remap(nix, words, csr["g_deleted"])
    got_f = f.remap_device(nix, dv)
    assert got_f.n_bitmaps == F and got_f.index is nix
    kept = 0
    for i in range(F):
        a, b = got_f.read(i), want_f.read(i)
        assert len(a) == (nix.n_docs + 63) // 64 and a.tobytes() == b.tobytes(), f"bitmap {i} differs at words {np.flatnonzero(a != b)[:8]}"
        kept += int(np.unpackbits(a.view(np.uint8)).sum())
    assert kept == {"none": 0, "all": F * nix.n_docs}.get(bits, kept) and (bits != "random" or 0 < kept < F * nix.n_docs)
    assert error_of(lambda: got_f.read(0, growing=True))[0] == INVALID   # no growing bitmaps yet, as after remap
    # the handle serves the remap again, and another compaction
    assert f.remap_device(nix, dv).read(1).tobytes() == want_f.read(1).tobytes()
    assert_same_segment(vb.DeviceSegment.maintain_device(gix, dv), want, "after the remaps")


def test_remap_without_growing_documents_and_its_refusals():
    c, seg, gix, pl, where, per_page, patterns = base()
    rng = np.random.default_rng(6)
    F = 3
    bits_s = filter_bits("random", F, seg.n_docs, rng)
    # n_grow = 0: a relation whose vectors tape holds nothing; the filter's growing bitmaps (of another growing segment) are ignored
    sealed_only = V.with_vectors_tape(X.with_flags(pl, where, patterns["every 63rd"]), [[]])
    dv0, got0, want0, flat0, words0, csr0 = compact_both(gix, sealed_only, "no growing documents")
    assert dv0.n_grow == 0
    nix0 = vb.GpuIndex(got0)
    gs = vb.GrowingSegment.from_pages(gix, pl)
    f = vb.DocFilter(gix, bits_s)
    f.set_growing(gs, filter_bits("random", F, 300, rng))
    want_f = f.remap(nix0, words0, np.zeros(0, np.uint8))
    got_f = f.remap_device(nix0, dv0)
    assert all(got_f.read(i).tobytes() == want_f.read(i).tobytes() for i in range(F))
    # refusals, each with the host-input remap's code
    cp = X.with_growing_deleted(X.with_flags(pl, where, patterns["every 65th"]), X.GROWING_DELETED["some"])
    dv, got, want, flat, words, csr = compact_both(gix, cp, "refusals")
    nix = vb.GpuIndex(got)
    plain = vb.DocFilter(gix, bits_s)   # no growing bitmaps while n_grow > 0
    code, msg = error_of(lambda: plain.remap(nix, words, csr["g_deleted"]))
    assert error_of(lambda: plain.remap_device(nix, dv)) == (code, msg) and code == UNSUPPORTED
    # growing bitmaps that cover another document count
    more = V.with_vectors_tape(cp, [[V.t2(3), V.t0(V.elements([V.key_of(1)], [2]))]])
    dv1 = vb.DeviceVacuum.from_pages(gix, more)
    assert dv1.n_grow == 1
    code, msg = error_of(lambda: f.remap(nix, words, np.zeros(1, np.uint8)))
    assert error_of(lambda: f.remap_device(nix, dv1)) == (code, msg) and code == INVALID
    # the handle of a relation of another document count
    seg_s, gix_s, pl_s = small(681)
    dv_s = vb.DeviceVacuum.from_pages(gix_s, pl_s)
    assert error_of(lambda: f.remap_device(nix, dv_s))[0] == INVALID
    # a new_index of another compaction
    code, msg = error_of(lambda: f.remap(nix0, words, csr["g_deleted"]))
    assert error_of(lambda: f.remap_device(nix0, dv)) == (code, msg) and code == INVALID and "another compaction" in msg
    # nothing is left behind: the same filter and handle remap as before
    ok, ok_want = f.remap_device(nix, dv), f.remap(nix, words, csr["g_deleted"])
    assert all(ok.read(i).tobytes() == ok_want.read(i).tobytes() for i in range(F))


# ---- 4. refusals

def assert_serves_a_valid_call(gix, pl, want_words):
    dv = vb.DeviceVacuum.from_pages(gix, pl)
    assert dv.read()[0].tobytes() == want_words.tobytes()
    vb.lib().vbm25_device_vacuum_free(None)


def test_documents_tape_refusals_equal_the_host_reader():
    c, seg, gix, pl, where, per_page, patterns = base()
    cp = X.with_flags(pl, where, patterns["a random half"])
    want_words = X.packed(patterns["a random half"])
    named, pairs = X.docs_damage(cp), X.docs_damage_pairs(cp)
    cases = [(n, [e]) for n, e in named] + pairs
    # one damage on each tape: the documents tape's is reported
    vnamed = V.named_damage(cp)
    cases += [(f"{n} + vectors tape: {vn}", [ve, e]) for (n, e), (vn, ve, _) in zip(named[4:8], vnamed[:4])]
    texts = set()
    for name, edits in cases:
        bad = X.apply(cp, edits)
        code, msg = X.host_flags(bad)
        assert code == CORRUPT, (name, code, msg)
        assert raw_vacuum(gix, bad) == (code, msg, None), (name, raw_vacuum(gix, bad)[:2], msg)
        texts.add(msg.split(": ", 2)[2].rsplit(" (page", 1)[0])
        assert_serves_a_valid_call(gix, cp, want_words)
    assert {"line pointer is not LP_NORMAL", "line pointer out of range", "document tuple too short", "page cannot be read",
            "page linked twice", "special area is not Opaque", "page header out of range", "document count differs from the Jump tuple"} <= texts
    # damage of the tapes neither host reader follows is no refusal
    for name, edit in D.named_damage(cp):
        if name in ("special != 8184", "a token with df = 0", "a summary with n = 0"):
            assert vb.DeviceVacuum.from_pages(gix, X.apply(cp, [edit])).read()[0].tobytes() == want_words.tobytes(), name


def test_vectors_tape_refusals_equal_the_device_reader_of_the_growing_segment():
    c, seg, gix, pl, where, per_page, patterns = base()
    cp = X.with_flags(pl, where, patterns["every 64th"])
    want_words = X.packed(patterns["every 64th"])
    cases = [(n, [e]) for n, e, _ in V.named_damage(cp)]
    cases.append(("keys not ascending", [V.unordered_keys(cp, skip=4)[1]]))
    cases.append(("keys not ascending twice", [V.unordered_keys(cp, skip=40)[1], V.unordered_keys(cp, skip=4)[1]]))
    tape = V.vectors_tape(cp)
    cases.append(("special area of the last page", [D.put("<H", tape[-1], 16, 8176)]))
    cases.append(("a page linked twice", [D.put("<I", tape[2], 8184, tape[1])]))
    cases.append(("an unreadable page", [D.put("<I", tape[1], 8184, 10**6)]))
    codes = set()
    for name, edits in cases:
        bad = X.apply(cp, edits)
        code, msg = error_of(lambda: vb.GrowingSegment.from_pages(gix, bad))
        assert raw_vacuum(gix, bad) == (code, msg, None), (name, raw_vacuum(gix, bad)[:2], msg)
        if code == CORRUPT:   # ... which is the host reader's text
            assert error_of(lambda: vb.growing_from_pages(bad)) == (code, msg), name
        codes.add(code)
        assert_serves_a_valid_call(gix, cp, want_words)
    assert codes == {CORRUPT, INVALID}


def test_tf_zero_is_accepted_by_the_reader_and_refused_by_the_compaction():
    c, seg, gix, pl, where, per_page, patterns = base()
    cp = X.with_flags(pl, where, patterns["every 65th"])
    edits = []
    for skip in (60, 25):   # (the later one first: the first in CSR order is named, not the first found)
        p, i, off, size = V.find_tuple(cp, 0, min_elements=2, skip=skip)
        s = struct.unpack_from("<H", bytes(cp[p]), off + 16)[0]
        edits.append(D.put("<I", p, off + s + 20 + 16, 0))   # the tf of the tuple's second element
    bad = X.apply(cp, edits)
    dv = vb.DeviceVacuum.from_pages(gix, bad)   # the handle is made
    words, csr = assert_same_inputs(dv, bad, "tf 0")
    zero_docs = np.unique(np.searchsorted(csr["g_start"], np.flatnonzero(csr["g_tf"] == 0), side="right") - 1)
    assert len(zero_docs) == 2
    code, msg = error_of(lambda: vb.DeviceSegment.maintain(gix, words, csr))
    assert error_of(lambda: vb.DeviceSegment.maintain_device(gix, dv)) == (code, msg)
    assert code == INVALID and msg.endswith(f"growing document {zero_docs[0]}: tf 0")
    # the index still serves, and so does the reader
    terms, off = make_queries(c, 4, 3, seed=2)
    hits, nh = vb.search_batch(gix, terms, off, 10)
    assert nh.sum() > 0
    compact_both(gix, cp, "after the tf 0 refusal")


def test_handles_of_another_document_count():
    c, seg, gix, pl, where, per_page, patterns = base()
    seg_s, gix_s, pl_s = small(681)
    rc, msg, out = raw_vacuum(gix, pl_s)   # the relation of another index
    assert rc == INVALID and not out and "another relation" in msg
    dv_s = vb.DeviceVacuum.from_pages(gix_s, pl_s)
    assert error_of(lambda: vb.DeviceSegment.maintain_device(gix, dv_s))[0] == INVALID
    assert_same_segment(vb.DeviceSegment.maintain_device(gix_s, dv_s), vb.DeviceSegment.maintain(gix_s, X.host_flags(pl_s)[2], vb.growing_from_pages(pl_s)),
                        "the small relation on its own index")
    assert_serves_a_valid_call(gix, pl, X.packed(patterns["none"]))


# ---- 5. past one chunk

def test_documents_tape_past_one_chunk():
    """700 000 documents of mean length 4: a documents tape of 1030 pages, more than CHUNK_PAGES = 1024, so the last pages lie in a
    second chunk.  None of the new kernels caps its grid and strides: doc_deleted_kernel runs one wave per page,
    mt_tf_zero_kernel one thread per growing element, mt_pack_deleted_kernel one wave per word of growing flags (the counts are
    hipcub's reductions).  So there is no second pass to provoke, and the chunk boundary is the one path this size adds."""
    ds = vb.DeviceSegment.synth(700_000, 3000, mean_len=4, seed=7)
    gix = vb.GpuIndex(ds)
    pl = ds.to_relation()
    (docs, _, _, _), _ = D.tapes(pl)
    assert len(docs) == 1030 > V.CHUNK_PAGES
    # flags flipped with numpy on the images: a random 1 %, and the documents on both sides of the chunk boundary
    per_page = np.array([D.page_tuples(pl[p]) for p in docs])
    first = np.r_[0, np.cumsum(per_page)]
    boundary = int(first[V.CHUNK_PAGES])
    rng = np.random.default_rng(9)
    flags = rng.random(700_000) < 0.01
    flags[boundary - 70:boundary + 70] = False
    flags[[boundary - 65, boundary - 64, boundary - 1, boundary, boundary + 1, boundary + 63, boundary + 64, 700_000 - 1]] = True
    for i, p in enumerate(docs):
        idx = np.flatnonzero(flags[first[i]:first[i + 1]])
        if len(idx):
            offs = pl[p][24:24 + 4 * per_page[i]].view("<u4") & 0x7fff
            pl[p][offs[idx]] = 1
    # a few hundred inserted documents: sealed keys, and for one in seven a key the vocabulary lacks
    keys = ds.download().arrays()["term_key"].reshape(-1, 16)
    tuples, page = [], []
    for g in range(300):
        ks = sorted([keys[r].tobytes() for r in rng.choice(len(keys), 5, replace=False)] + ([V.key_of(g, b"zz")] if g % 7 == 0 else []))
        page += [V.t2(g % 200), V.t0(V.elements(ks, rng.integers(1, 9, len(ks))), (g >> 8, g & 0xff, 1), deleted=int(g % 10 == 3))]
        if len(page) == 40:
            tuples.append(page)
            page = []
    tuples.append(page)
    pl = V.with_vectors_tape(pl, tuples)
    dv, got, want, flat, words, csr = compact_both(gix, pl, "past one chunk")
    assert words.tobytes() == X.packed(flags).tobytes() and dv.n_grow == 300 and dv.n_grow_deleted == 30
    assert got.n_docs == 700_000 - int(flags.sum()) + 270
    # the remap
    nix = vb.GpuIndex(got)
    F = 3
    gs = vb.GrowingSegment.from_pages(gix, pl)
    f = vb.DocFilter(gix, rng.random((F, 700_000)) < 0.5)
    f.set_growing(gs, rng.random((F, 300)) < 0.5)
    got_f, want_f = f.remap_device(nix, dv), f.remap(nix, words, csr["g_deleted"])
    assert all(got_f.read(i).tobytes() == want_f.read(i).tobytes() for i in range(F))
    # damage in the second chunk, and a page that cannot be read after the first chunk went up
    p = docs[V.CHUNK_PAGES + 3]
    bad = D.damaged(pl, [p], D.set_lp(p, 100, size=7))
    code, msg = X.host_flags(bad)
    assert raw_vacuum(gix, bad) == (code, msg, None) and code == CORRUPT and f"(page {p})" in msg
    stop = docs[V.CHUNK_PAGES + 4]
    rc, msg, out = raw_vacuum(gix, lambda i: None if i == stop else (pl[i].ctypes.data if i < len(pl) else None))
    assert rc == CORRUPT and not out and f"page cannot be read (page {stop})" in msg
    assert vb.DeviceVacuum.from_pages(gix, pl).read()[0].tobytes() == words.tobytes()


# ---- 6. concurrency

def test_four_threads_and_a_stream_in_flight():
    c, seg, gix, pl, where, per_page, patterns = base()
    names = ["a random half", "every 63rd", "all", "the 40 documents around each page boundary"]
    rels = [X.with_growing_deleted(X.with_flags(pl, where, patterns[n]), X.GROWING_DELETED["some" if i % 2 else "none"]) for i, n in enumerate(names)]
    results, errors = [None] * 4, []

    def work(i):
        try:
            dv = vb.DeviceVacuum.from_pages(gix, rels[i])
            results[i] = (dv, vb.DeviceSegment.maintain_device(gix, dv))
        except Exception as e:   # noqa: BLE001 -- reported below, in the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, (dv, ds) in enumerate(results):
        words, csr = assert_same_inputs(dv, rels[i], f"thread {i}")
        assert_same_segment(ds, vb.DeviceSegment.maintain(gix, words, csr), f"thread {i}")
    # a read beside a stream with batches in flight: the stream's results are what they are without it
    terms, off = make_queries(c, 16, 4, seed=3)
    nq = len(off) - 1
    one, n_one = vb.search_batch(gix, terms, off, 10)
    st = vb.Stream(gix, 3, nq, len(terms), 10)
    for _ in range(3):
        st.submit(terms, off)
    dv = vb.DeviceVacuum.from_pages(gix, rels[0])
    ds = vb.DeviceSegment.maintain_device(gix, dv)
    for _ in range(3):
        h, n = st.collect()
        assert n.tobytes() == n_one.tobytes() and all(h[q, :n[q]].tobytes() == one[q, :n[q]].tobytes() for q in range(nq))
    words, csr = assert_same_inputs(dv, rels[0], "beside the stream")
    assert_same_segment(ds, vb.DeviceSegment.maintain(gix, words, csr), "beside the stream")
