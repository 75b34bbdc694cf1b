"""The device reader of VACUUM's inputs without a device: its per-document function and its word packing (csrc/pages_parse.h:
doc_deleted_lane, flag_round_words) under AddressSanitizer + UBSan on the CPU against vbm25_sealed_deleted_from_pages, and the ABI of
vbm25_device_vacuum_*, vbm25_index_maintain_device and vbm25_filter_remap_device.  No GPU use."""
import ctypes as C
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import pages_device_data as D
import vacuum_device_data as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vbm25_device_vacuum_from_pages", "vbm25_device_vacuum_info", "vbm25_device_vacuum_read", "vbm25_device_vacuum_free",
               "vbm25_index_maintain_device", "vbm25_filter_remap_device")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_sealed_deleted.cpp built with AddressSanitizer + UBSan: a stand-alone program over the header alone, nothing
    of it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_sealed_deleted")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests/native/fuzz_sealed_deleted.cpp"), "-o", exe])
    return exe


def run_harness(harness, tmp_path, pl, cases):
    """the harness' line per case: (0, docs, deleted, crc) | (-2, page, text)"""
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
            got.append((0, int(f[1]), int(f[3]), int(f[5], 16)))
        else:
            m = re.fullmatch(r"page (\d+) what (.*)", rest)
            got.append((rc, int(m.group(1)), m.group(2)))
    return got


def expected(pl):
    """what vbm25_sealed_deleted_from_pages says of the relation, in the harness' form"""
    r = X.host_flags(pl)
    if len(r) == 2:
        m = re.fullmatch(r"vbm25 error -2: data corruption: (.*) \(page (\d+)\)", r[1])
        assert r[0] == -2 and m, r
        return (-2, int(m.group(2)), m.group(1))
    return (0, r[0], r[1], zlib.crc32(r[2].tobytes()))


def check_cases(harness, tmp_path, pl, cases, names):
    got = run_harness(harness, tmp_path, pl, cases)
    seen = set()
    for name, edits, g in zip(names, cases, got):
        want = expected(D.apply_edits(pl, edits) if edits else pl)
        seen.add(want[0])
        assert g == want, (name, g, want)
    return seen


def edits_of(pl, *edit_fns):
    cp = [p.copy() for p in pl]
    for e in edit_fns:
        e(cp)
    return D.byte_edits(pl, cp, range(len(pl)))


def flag_edits(where, flags):
    return [(where[d][0], where[d][1], int(flags[d])) for d in np.flatnonzero(flags)]


def test_flag_patterns_on_five_pages(tmp_path, harness):
    """3000 documents on pages of 680, 680, 680, 680 and 280: the words straddle every page boundary (680 = 10 x 64 + 40).  Every
    pattern's words, count and document count equal the host reader's; the host reader's equal np.packbits of the pattern"""
    c, seg, pl = X.vacuum_relation()
    where, per_page = X.doc_slots(pl)
    assert per_page == [680, 680, 680, 680, 280] and all(int(b) % 64 for b in np.cumsum(per_page)[:-1])
    patterns = X.flag_patterns(seg.n_docs, per_page)
    assert len(patterns) == 9
    for name, flags in patterns.items():
        n, n_del, words = X.host_flags(X.with_flags(pl, where, flags))
        assert (n, n_del) == (seg.n_docs, int((flags != 0).sum())) and np.array_equal(words, X.packed(flags)), name
    assert set(np.unique(patterns["all"]).tolist()) == set(X.FLAG_BYTES)
    seen = check_cases(harness, tmp_path, pl, [flag_edits(where, f) for f in patterns.values()], list(patterns))
    assert seen == {0}


def test_small_document_counts_and_the_empty_relation(tmp_path, harness):
    for n in X.SMALL_DOC_COUNTS:
        seg, pl = X.small_relation(n)
        where, per_page = X.doc_slots(pl)
        assert sum(per_page) == n == seg.n_docs
        patterns = X.flag_patterns(n, per_page, seed=n)
        assert check_cases(harness, tmp_path, pl, [flag_edits(where, f) for f in patterns.values()], [f"{n}: {p}" for p in patterns]) == {0}
    assert X.SMALL_DOC_COUNTS[-1] == 681 and X.doc_slots(X.small_relation(681)[1])[1] == [680, 1]
    assert check_cases(harness, tmp_path, D.empty_relation(), [[]], ["empty"]) == {0}
    assert expected(D.empty_relation()) == (0, 0, 0, zlib.crc32(b""))


def test_damage_of_the_documents_tape(tmp_path, harness):
    """every named damage: the host reader's message and page; two damages: the first in tape order, a page's tuples ahead of its
    link; damage the host reader of the flags never meets (the other tapes) changes nothing"""
    c, seg, pl = X.vacuum_relation()
    where, per_page = X.doc_slots(pl)
    flags = X.flag_patterns(seg.n_docs, per_page)["a random half"]
    base = X.with_flags(pl, where, flags)
    named, pairs = X.docs_damage(base), X.docs_damage_pairs(base)
    cases = [edits_of(base, e) for _, e in named] + [edits_of(base, *es) for _, es in pairs]
    names = [n for n, _ in named] + [n for n, _ in pairs]
    assert check_cases(harness, tmp_path, base, cases, names) == {-2}
    texts = {expected(D.apply_edits(base, e))[2] for e in cases}
    assert {"line pointer is not LP_NORMAL", "line pointer out of range", "document tuple too short", "page cannot be read",
            "page linked twice", "special area is not Opaque", "page header out of range",
            "document count differs from the Jump tuple", "bad magic number"} <= texts
    other = [(n, e) for n, e in D.named_damage(base) if n in ("special != 8184", "a token with df = 0", "a summary with n = 0")]
    assert len(other) == 3
    assert check_cases(harness, tmp_path, base, [edits_of(base, e) for _, e in other], [n for n, _ in other]) == {0}


def test_random_byte_edits_of_the_documents_tape(tmp_path, harness):
    """200 seeded random edits of 1 to 3 bytes on the documents tape's pages (half of them in the header, the line pointers and the
    special area): the host reader's verdict exactly -- the words and counts, or the message and page, also where several edits
    damage several pages: a page's tuples are looked at before its link is followed, as the host reader does -- and never an access
    outside the arrays"""
    c, seg, pl = X.vacuum_relation()
    (docs, _, _, _), _ = D.tapes(pl)
    cases = [[(docs[pg], pos, val) for pg, pos, val in edits] for edits in D.random_damage(len(docs), 200, seed=4)]
    assert any(len(e) > 1 for e in cases)
    assert check_cases(harness, tmp_path, pl, cases, [str(e) for e in cases]) == {0, -2}


# ---- the ABI

def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    lib = C.CDLL(vb.library_path())
    from vectorchord_bm25_amd._lib import ABI
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(lib, name) and name in ABI, name
    assert "typedef struct vbm25_device_vacuum vbm25_device_vacuum;" in header
    assert hasattr(vb, "DeviceVacuum") and hasattr(vb.DeviceVacuum, "from_pages") and hasattr(vb.DeviceVacuum, "read")
    assert hasattr(vb.DeviceSegment, "maintain_device") and hasattr(vb.DocFilter, "remap_device")
    hpp = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    assert "class DeviceVacuum" in hpp and "vbm25_index_maintain_device" in hpp and "vbm25_filter_remap_device" in hpp


def test_null_arguments_are_invalid():
    L = vb.lib()
    cb = vb.api.READ_PAGE_FN(lambda ctx, i: None)
    fn = C.cast(cb, C.c_void_p)
    fake = C.create_string_buffer(256)   # never looked into: the arguments are checked first
    h = C.addressof(fake)
    out = C.c_void_p(1)
    assert L.vbm25_device_vacuum_from_pages(None, fn, None, C.byref(out)) == -1 and not out.value
    out = C.c_void_p(1)
    assert L.vbm25_device_vacuum_from_pages(h, None, None, C.byref(out)) == -1 and not out.value
    assert L.vbm25_device_vacuum_from_pages(h, fn, None, None) == -1
    n = C.c_uint32(7)
    assert L.vbm25_device_vacuum_info(None, C.byref(n), None, None, None, None) == -1 and n.value == 7
    words = np.full(2, 5, np.uint64)
    assert L.vbm25_device_vacuum_read(None, words.ctypes.data_as(C.c_void_p), None) == -1 and (words == 5).all()
    out = C.c_void_p(1)
    assert L.vbm25_index_maintain_device(None, h, None, C.byref(out)) == -1 and not out.value
    out = C.c_void_p(1)
    assert L.vbm25_index_maintain_device(h, None, None, C.byref(out)) == -1 and not out.value
    assert L.vbm25_index_maintain_device(h, h, None, None) == -1
    for args in ((None, h, h), (h, None, h), (h, h, None)):
        out = C.c_void_p(1)
        assert L.vbm25_filter_remap_device(*args, C.byref(out)) == -1 and not out.value
    assert L.vbm25_filter_remap_device(h, h, h, None) == -1
    L.vbm25_device_vacuum_free(None)   # a no-op


def test_no_host_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c, seg, pl = X.vacuum_relation()
    cb, keep = vb.api._page_reader(pl)
    fake = C.create_string_buffer(256)   # without a device there is no index, filter or handle: the answer comes before a look into one
    h = C.addressof(fake)
    L = vb.lib()
    out = C.c_void_p(1)
    assert L.vbm25_device_vacuum_from_pages(h, C.cast(cb, C.c_void_p), None, C.byref(out)) == -3 and not out.value
    out = C.c_void_p(1)
    assert L.vbm25_index_maintain_device(h, h, None, C.byref(out)) == -3 and not out.value
    out = C.c_void_p(1)
    assert L.vbm25_filter_remap_device(h, h, h, C.byref(out)) == -3 and not out.value
    assert b"no HIP device" in L.vbm25_last_error()
