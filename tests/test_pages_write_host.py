"""The device writer without a device: its layout and fill functions (csrc/pages_emit.h) under AddressSanitizer on the CPU against
the oracle's writer, and the ABI of vbm25_device_segment_page_count / _write_pages / _write_relation.  No GPU use."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import vectorchord_bm25_amd as vb
from vectorchord_bm25_amd._lib import ABI, Flushed
import pages_device_data as D
import pages_write_data as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vbm25_device_segment_page_count", "vbm25_device_segment_write_pages", "vbm25_device_segment_write_relation")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/native/fuzz_pages_write.cpp built with AddressSanitizer + UBSan (the build line of tests/test_pages_device_host.py): a
    stand-alone program, nothing of it is loaded into this process"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("harness") / "fuzz_pages_write")
    src = [os.path.join(ROOT, p) for p in ("tests/native/fuzz_pages_write.cpp", "vectorchord-bm25_amd/csrc/pages.cpp",
                                           "vectorchord-bm25_amd/csrc/segment.cpp", "vectorchord-bm25_amd/csrc/blake3.cpp", "oracle/oracle.cpp",
                                           "oracle/pages.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-pthread", *src, "-o", exe])
    return exe


def small_relations():
    """the oracle's relations of the small segments tests/test_gpu_pages_write.py writes on the GPU"""
    rels = [D.page_list(D.relation(800, 100)[3]), D.page_list(D.relation()[3]), W.oracle_relation(D.terms_of_interest_segment()),
            W.oracle_relation(vb.segment_from_pages(D.empty_relation())), W.oracle_relation(W.host_segment(W.docs_corpus(1, n_terms=1)))]
    rels += [D.single_posting_relation(n)[1] for n in (225, 226, 227, 290, 291, 292, 2000)]
    rels += [W.oracle_relation(W.host_segment(W.docs_corpus(n))) for n in (679, 680, 681)]
    return rels


def test_layout_and_fill_under_asan(tmp_path, harness):
    """tests/native/fuzz_pages_write.cpp: the writer's passes as plain loops over csrc/pages_emit.h, buffers sized exactly as the device
    allocates them, built with AddressSanitizer + UBSan.  First the small relations of the GPU test, then 2000 seeded random segments
    (1 .. 3000 documents, 1 .. 600 terms, df 1 .. 400): every page equal to orc_pages_build's, no sanitizer report."""
    rels = small_relations()
    # the empty segment: every tape one empty page, start_* NONE
    j = W.jump_fields(rels[3])
    assert len(rels[3]) == 10 and j["number_of_documents"] == 0 and j["start_documents"] == j["start_tokens"] == W.NONE
    case_file = str(tmp_path / "relations.bin")
    W.write_relation_file(case_file, rels)
    out = subprocess.run([harness, case_file], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert f"case file done: {len(rels)} relations rewritten" in out.stdout
    assert "fuzz done: 2000 segments" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_deep_address_trees_under_asan(tmp_path, harness):
    """The harness on the two relations whose address trees have a second level: 2036 x 680 + 1 documents (one documents page more than
    an address page holds: depth_documents 2) and single_posting_relation(540 000) (2390 tokens pages > 407: depth_tokens 2, and tapes
    of more than two chunks of 1024 images).  The case file only."""
    full = W.oracle_relation(W.host_segment(W.docs_corpus(W.ADDR_DOCS_WIDTH * W.DOCS_PER_PAGE)))
    over = W.oracle_relation(W.host_segment(W.docs_corpus(W.ADDR_DOCS_WIDTH * W.DOCS_PER_PAGE + 1)))
    big = D.single_posting_relation(540_000)[1]
    assert W.jump_fields(full)["depth_documents"] == 1 and W.jump_fields(over)["depth_documents"] == 2
    assert W.jump_fields(big)["depth_tokens"] == 2
    (docs, toks, sums, blks), _ = D.tapes(big)
    assert min(len(toks), len(blks)) > 2 * W.CHUNK_PAGES and len(sums) > W.CHUNK_PAGES
    case_file = str(tmp_path / "relations.bin")
    W.write_relation_file(case_file, [full, over, big])
    out = subprocess.run([harness, case_file, "only"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "case file done: 3 relations rewritten" in out.stdout and "fuzz done" not in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "vbm25.h")).read()
    assert "typedef int (*vbm25_write_page_fn)(void *ctx, uint32_t page_id, const uint8_t *image);" in header
    assert "typedef struct vbm25_flushed {" in header
    L = C.CDLL(vb.library_path())
    for name in SYMBOLS:
        assert f"int {name}(const vbm25_device_segment *" in header and hasattr(L, name) and name in ABI, name
    for method in ("page_count", "write_pages", "to_relation"):
        assert hasattr(vb.DeviceSegment, method), method
    hpp = open(os.path.join(ROOT, "include", "vbm25.hpp")).read()
    for method in ("uint32_t page_count() const", "vbm25_flushed write_pages(", "uint32_t write_relation("):
        assert method in hpp, method
    assert C.sizeof(Flushed) == 64 and Flushed.ptr_blocks.offset == 56 and Flushed.depth_documents.offset == 20


def test_null_arguments_are_invalid():
    L = vb.lib()
    cb = vb.api.WRITE_PAGE_FN(lambda ctx, i, image: 0)
    fn, n, f = C.cast(cb, C.c_void_p), C.c_uint32(7), Flushed()
    buf = C.create_string_buffer(4096)
    fake = C.c_void_p(C.addressof(buf))   # never looked at: a NULL argument is refused first
    assert L.vbm25_device_segment_page_count(None, C.byref(n)) == -1 and L.vbm25_device_segment_page_count(fake, None) == -1
    assert L.vbm25_device_segment_write_pages(None, None, 0, 0, fn, None, C.byref(f)) == -1
    assert L.vbm25_device_segment_write_pages(fake, None, 0, 0, None, None, C.byref(f)) == -1
    assert L.vbm25_device_segment_write_pages(fake, None, 0, 0, fn, None, None) == -1
    assert L.vbm25_device_segment_write_relation(None, None, fn, None, C.byref(n)) == -1 and n.value == 0
    assert L.vbm25_device_segment_write_relation(fake, None, None, None, None) == -1
    assert b"NULL" in L.vbm25_last_error()


def test_no_host_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = vb.lib()
    cb = vb.api.WRITE_PAGE_FN(lambda ctx, i, image: 0)
    fn, n, f = C.cast(cb, C.c_void_p), C.c_uint32(), Flushed()
    buf = C.create_string_buffer(4096)
    fake = C.c_void_p(C.addressof(buf))   # without a device nothing of the segment is read
    assert L.vbm25_device_segment_page_count(fake, C.byref(n)) == -3   # VBM25_ERR_DEVICE: there is no host writer to fall back to
    assert L.vbm25_device_segment_write_pages(fake, None, 0, 0, fn, None, C.byref(f)) == -3
    assert L.vbm25_device_segment_write_relation(fake, None, fn, None, C.byref(n)) == -3
    assert b"no CPU fallback" in L.vbm25_last_error()
