"""The device reader of the growing segment without a device: its per-tuple and per-element functions (csrc/vectors_parse.h) under
AddressSanitizer + UBSan on the CPU against vbm25_growing_from_pages, the ABI of vbm25_device_growing_from_pages, and
vbm25_sealed_deleted_from_pages (host only).  No GPU use."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import pages_device_data as D
import vectors_device_data as V
import maintain_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_vectors_device.cpp built with AddressSanitizer + UBSan: a stand-alone program over the header alone, nothing
    of it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_vectors_device")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests/native/fuzz_vectors_device.cpp"), "-o", exe])
    return exe


def run_harness(harness, tmp_path, pl, cases):
    """the harness' line per case: (0, docs, elements, [crc x 6]) | (-2, page, text) | (-1, document)"""
    case_file = str(tmp_path / "cases.bin")
    D.write_case_file(case_file, pl, cases)
    out = subprocess.run([harness, case_file], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == f"done: {len(cases)} cases"
    got = []
    for i, line in enumerate(lines[:-1]):
        m = re.fullmatch(rf"case {i}: rc (-?\d+) (.*)", line)
        assert m, line
        rc, rest = int(m.group(1)), m.group(2)
        if rc == 0:
            f = rest.split()
            got.append((0, int(f[1]), int(f[3]), [int(x, 16) for x in f[5:11]]))
        elif rc == -2:
            m = re.fullmatch(r"page (\d+) what (.*)", rest)
            got.append((-2, int(m.group(1)), m.group(2)))
        else:
            got.append((rc, int(rest.split()[1])))
    return got


def expected(pl):
    """what the host composition says of the relation, in the harness' form: vbm25_growing_from_pages, then vbm25_growing_upload's
    rule on the keys (the upload itself needs an index, hence a device)"""
    kind, g = V.host_growing(pl)
    if kind == "corrupt":
        m = re.fullmatch(r"vbm25 error -2: data corruption: (.*) \(page (\d+)\)", g)
        return (-2, int(m.group(2)), m.group(1))
    bad = V.first_unordered_document(g)
    if bad is not None:
        return (-1, bad)
    return (0, len(g["g_start"]) - 1, len(g["g_tf"]), V.crcs(g))


def check_cases(harness, tmp_path, pl, cases, names, exact_page=True):
    got = run_harness(harness, tmp_path, pl, cases)
    seen = set()
    for name, edits, g in zip(names, cases, got):
        want = expected(D.apply_edits(pl, edits) if edits else pl)
        seen.add(want[0])
        if want[0] == -2 and not exact_page:
            # several damages: a refusal of the page walk may come before a tuple's on an earlier page -- the code is the same
            assert g[0] == -2, (name, g, want)
        else:
            assert g == want, (name, g, want)
    return seen


def edits_of(pl, *edit_fns):
    cp = [p.copy() for p in pl]
    for e in edit_fns:
        e(cp)
    return D.byte_edits(pl, cp, range(len(pl)))


def test_golden_fixture_and_interleaved_relation(tmp_path, harness):
    """the struct.pack fixture and relation() with 300 inserts of lognormal length (documents across pages, of 0 elements, unknown
    keys, deleted ones): every array equals vbm25_growing_from_pages'"""
    raw = open(os.path.join(GOLD, "page_fixture.bin"), "rb").read()
    gold = [np.frombuffer(raw[i:i + 8192], np.uint8).copy() for i in range(0, len(raw), 8192)]
    assert check_cases(harness, tmp_path, gold, [[]], ["golden"]) == {0}
    c, seg, pl = V.interleaved_relation()
    g = vb.growing_from_pages(pl)
    assert len(g["g_start"]) == 304 and g["g_deleted"].sum() == 5 and (np.diff(g["g_start"].astype(np.int64)) == 0).sum() >= 3
    assert 1 in _tags(pl)   # documents that do not fit the rest of a page: _1 tuples
    assert check_cases(harness, tmp_path, pl, [[]], ["interleaved"]) == {0}


def _tags(pl):
    return [struct.unpack_from("<Q", bytes(pl[p]), off)[0] for p in V.vectors_tape(pl) for off, _ in D.slots(pl[p])]


@pytest.mark.parametrize("case", V.hand_tapes(), ids=lambda c: c[0])
def test_hand_made_tapes(tmp_path, harness, case):
    """the state machine's corners on hand-made tapes: the host reader says what the construction says, the lanes agree with it"""
    name, pages_of_tuples, text = case
    pl = V.hand_relation(pages_of_tuples)
    kind, g = V.host_growing(pl)
    if text == "ok":
        assert kind == "ok", (name, g)
    else:
        assert kind == "corrupt" and text in g, (name, g)
    check_cases(harness, tmp_path, pl, [[]], [name])
    if name.startswith("a document of 1000"):
        assert np.diff(g["g_start"].astype(np.int64)).tolist() == [2, 1000, 2] and g["g_deleted"].tolist() == [0, 0, 1]
    if "dropped attempt with" in name:
        assert g["g_fieldnorm"].tolist() == [7, 8, 7] and len(g["g_tf"]) == 2 + 3 + 2
    if name == "a tape of pages without tuples":
        assert len(g["g_start"]) == 1


def test_named_damage_of_a_vector_tuple(tmp_path, harness):
    """every named single-field damage: refused with the host reader's message and page; two damages: the first in tape order; keys
    not ascending: the first such document"""
    c, seg, pl = V.interleaved_relation()
    named = V.named_damage(pl)
    for name, edit, text in named:
        kind, msg = V.host_growing(D.apply_edits(pl, edits_of(pl, edit)))
        assert kind == "corrupt" and text in msg, (name, msg)
    cases = [edits_of(pl, edit) for _, edit, _ in named]
    names = [n for n, _, _ in named]
    # pairs: an early and a late damage, in both orders of application
    late = V.named_damage(pl, skip=5)
    for (n1, e1, _), (n2, e2, _) in zip(named[:5], late[5:]):
        cases.append(edits_of(pl, e2, e1))
        names.append(f"{n1} + later {n2}")
    p, unordered = V.unordered_keys(pl, skip=4)
    p2, unordered2 = V.unordered_keys(pl, skip=40)
    cases += [edits_of(pl, unordered), edits_of(pl, unordered2, unordered)]
    names += ["keys not ascending", "keys not ascending twice"]
    seen = check_cases(harness, tmp_path, pl, cases, names)
    assert seen == {-2, -1}


def test_random_byte_edits_of_the_tape(tmp_path, harness):
    """200 seeded random edits of 1 to 3 bytes on the vectors tape's pages (half of them in the header, the line pointers and the
    special area): accepted with equal arrays or refused with the host composition's code -- and, as one edit is one damage, its
    message and page -- and never an access outside the arrays"""
    c, seg, pl = V.interleaved_relation()
    tape = V.vectors_tape(pl)
    cases = [[(tape[pg], pos, val) for pg, pos, val in edits] for edits in D.random_damage(len(tape), 200, seed=2)]
    single = [e for e in cases if len(e) == 1]
    multi = [e for e in cases if len(e) > 1]
    seen = check_cases(harness, tmp_path, pl, single, [str(e) for e in single])
    seen |= check_cases(harness, tmp_path, pl, multi, [str(e) for e in multi], exact_page=False)
    assert {0, -2} <= seen


def test_long_tapes_under_asan(tmp_path, harness):
    """the tapes tests/test_gpu_vectors_device.py reads past one chunk: the lanes reach p / CHUNK_PAGES >= 1 with the chunks allocated
    as the device allocates them; and a page of 400 _2 tuples"""
    pl = V.hand_relation(V.long_tape(V.CHUNK_PAGES + 40))
    assert len(V.vectors_tape(pl)) > V.CHUNK_PAGES
    p = V.vectors_tape(pl)[V.CHUNK_PAGES + 10]
    off = D.slots(pl[p])[1][0]
    damaged = edits_of(pl, D.put("<Q", p, off, 3))
    assert check_cases(harness, tmp_path, pl, [[], damaged], ["long", "long, damaged in chunk 1"]) == {0, -2}
    pl = V.hand_relation(V.only_starts_tape())
    g = vb.growing_from_pages(pl)
    assert g["g_fieldnorm"].tolist() == [399 % 256] and g["g_tf"].tolist() == [1, 2, 3]
    assert check_cases(harness, tmp_path, pl, [[]], ["only starts"]) == {0}


# ---- vbm25_sealed_deleted_from_pages

def _flag_relation():
    c, seg, oix, pages = D.relation(n_docs=2500, vocab=100)
    pl = [p.copy() for p in D.page_list(pages)]
    (docs, _, _, _), _ = D.tapes(pl)
    assert len(docs) > 2 and seg.n_docs % 64 != 0
    where = [(p, off) for p in docs for off, _ in D.slots(pl[p])]
    assert len(where) == seg.n_docs
    return seg, pl, where


@pytest.mark.parametrize("pattern", ["none", "all", "every 7th", "bytes 1, 2 and 255"])
def test_sealed_deleted_flags(pattern):
    seg, pl, where = _flag_relation()
    n = seg.n_docs
    flags = np.zeros(n, np.uint8)
    if pattern == "all":
        flags[:] = 1
    elif pattern == "every 7th":
        flags[::7] = 1
    elif pattern == "bytes 1, 2 and 255":
        flags[5], flags[64], flags[n - 1], flags[n - 2] = 1, 2, 255, 2
    cp = [p.copy() for p in pl]
    for d in np.flatnonzero(flags):
        D.put("<B", where[d][0], where[d][1], int(flags[d]))(cp)
    got = vb.sealed_deleted_from_pages(cp)
    assert got.dtype == np.bool_ and np.array_equal(got, flags != 0)
    # the words themselves, through the C ABI: np.packbits of the pattern, the bits beyond n_docs clear
    cb, keep = vb.api._page_reader(cp)
    nd, ndel = C.c_uint32(), C.c_uint32()
    assert vb.lib().vbm25_sealed_deleted_from_pages(C.cast(cb, C.c_void_p), None, None, 0, C.byref(nd), C.byref(ndel)) == 0
    assert (nd.value, ndel.value) == (n, int((flags != 0).sum()))
    words = np.full((n + 63) // 64 + 1, 0xdeadbeef, np.uint64)
    assert vb.lib().vbm25_sealed_deleted_from_pages(C.cast(cb, C.c_void_p), None, words.ctypes.data_as(C.c_void_p), len(words),
                                                    C.byref(nd), None) == 0
    want = np.packbits(np.r_[flags != 0, np.zeros(64 * (len(words) - 1) - n, bool)], bitorder="little").view(np.uint64)
    assert np.array_equal(words[:-1], want) and words[-1] == 0xdeadbeef
    # DeviceSegment.maintain's numpy model takes the words: a compaction that drops exactly these documents
    a = seg.arrays()
    assert np.array_equal(maintain_model.deleted_flags(want, n), flags != 0)
    build_args, relabel = maintain_model.maintain(a, seg.meta(), deleted=want)
    assert len(build_args[2]) == n - int(got.sum()) and np.array_equal(relabel[:n] == 0xFFFFFFFF, flags != 0)
    # the sealed segment is read as before, whatever the flags
    again = vb.segment_from_pages(cp)
    assert np.array_equal(again.arrays()["doc_fieldnorm"], a["doc_fieldnorm"])


def test_sealed_deleted_refusals():
    seg, pl, where = _flag_relation()
    L = vb.lib()
    cb, keep = vb.api._page_reader(pl)
    fn = C.cast(cb, C.c_void_p)
    nd = C.c_uint32(7)
    words = np.zeros((seg.n_docs + 63) // 64, np.uint64)
    assert L.vbm25_sealed_deleted_from_pages(None, None, None, 0, C.byref(nd), None) == -1
    assert L.vbm25_sealed_deleted_from_pages(fn, None, None, 0, None, None) == -1
    words[:] = 5
    assert L.vbm25_sealed_deleted_from_pages(fn, None, words.ctypes.data_as(C.c_void_p), len(words) - 1, C.byref(nd), None) == -1
    assert (words == 5).all() and "words" in L.vbm25_last_error().decode()
    # a damaged documents tape: refused as vbm25_segment_from_pages refuses it, nothing written
    (docs, _, _, _), (ptr_jump, joff) = D.tapes(pl)
    for name, pages, edit in [("line pointer", [docs[1]], D.set_lp(docs[1], 3, flags=2)),
                              ("tuple size 4", [docs[0]], D.set_lp(docs[0], 2, size=4)),
                              ("next -> 10^6", [docs[0]], D.put("<I", docs[0], 8184, 10**6)),
                              ("pd_lower - 4", [docs[-1]], D.add(docs[-1], 12, -4, "<H")),
                              ("Jump n_docs + 1", [ptr_jump], D.add(ptr_jump, joff + 4, 1, "<I")),
                              ("bad magic", [0], D.put("<8s", 0, D.slots(pl[0])[0][0], b"notmagic"))]:
        cp = D.damaged(pl, pages, edit)
        code, msg = D.host_error(cp)
        with pytest.raises(vb.Vbm25Error) as e:
            vb.sealed_deleted_from_pages(cp)
        assert (e.value.code, str(e.value)) == (code, msg) and code == -2, name
        cb2, keep2 = vb.api._page_reader(cp)
        assert L.vbm25_sealed_deleted_from_pages(C.cast(cb2, C.c_void_p), None, words.ctypes.data_as(C.c_void_p), len(words),
                                                 C.byref(nd), None) == -2
        assert (words == 5).all() and nd.value == 0, name


# ---- the ABI of vbm25_device_growing_from_pages

def test_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    assert "int vbm25_device_growing_from_pages(vbm25_index *index, vbm25_read_page_fn read_page, void *ctx, vbm25_device_growing **out," in header
    assert "int vbm25_sealed_deleted_from_pages(vbm25_read_page_fn read_page, void *ctx, uint64_t *words, uint32_t n_words," in header
    lib = C.CDLL(vb.library_path())
    assert hasattr(lib, "vbm25_device_growing_from_pages") and hasattr(lib, "vbm25_sealed_deleted_from_pages")
    assert hasattr(vb.GrowingSegment, "from_pages") and hasattr(vb, "sealed_deleted_from_pages")


def test_null_arguments_are_invalid():
    L = vb.lib()
    cb = vb.api.READ_PAGE_FN(lambda ctx, i: None)
    fn = C.cast(cb, C.c_void_p)
    index = C.create_string_buffer(64)   # never looked into: the arguments are checked first
    out, csr = C.c_void_p(1), C.c_void_p(1)
    assert L.vbm25_device_growing_from_pages(None, fn, None, C.byref(out), C.byref(csr)) == -1 and not out.value and not csr.value
    out, csr = C.c_void_p(1), C.c_void_p(1)
    assert L.vbm25_device_growing_from_pages(C.addressof(index), None, None, C.byref(out), C.byref(csr)) == -1 and not out.value and not csr.value
    csr = C.c_void_p(1)
    assert L.vbm25_device_growing_from_pages(C.addressof(index), fn, None, None, C.byref(csr)) == -1 and not csr.value


def test_no_host_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c, seg, pl = V.interleaved_relation()
    cb, keep = vb.api._page_reader(pl)
    index = C.create_string_buffer(64)   # without a device there is no index: the reader answers before it looks into one
    out, csr = C.c_void_p(1), C.c_void_p(1)
    rc = vb.lib().vbm25_device_growing_from_pages(C.addressof(index), C.cast(cb, C.c_void_p), None, C.byref(out), C.byref(csr))
    assert rc == -3 and not out.value and not csr.value   # VBM25_ERR_DEVICE: the host reader is another entry point, not a fallback
