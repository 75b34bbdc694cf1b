"""The device writer (vbm25_device_segment_write_pages / _write_relation / _page_count: csrc/pages_write.hip) on the GPU: a device segment
goes out as the reference's page images.  The comparator is always the oracle's writer (orc.Pages: orc_pages_build) and the host
reader, never the code under test."""
import threading

import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
import pages_device_data as D
import pages_write_data as W
from growing_data import make_growing
from maintain_model import make_growing_new_keys

pytestmark = pytest.mark.gpu

_C = {}


def cached(name, make):
    if name not in _C:
        _C[name] = make()
    return _C[name]


def check_round_trip(oracle_pl, what):
    """DeviceSegment.from_pages(the oracle's relation) written again equals the oracle's relation"""
    ds = vb.DeviceSegment.from_pages(oracle_pl)
    W.assert_same_pages(ds.to_relation(W.SEED), oracle_pl, what)
    assert ds.page_count() == len(oracle_pl) - 4, what
    return ds


def check_built(c, what, k1=1.2, b=0.75):
    """a device build from the corpus arrays, written, equals the oracle's relation of the host build"""
    want = W.oracle_relation(W.host_segment(c, k1, b))
    ds = vb.DeviceSegment.build(k1, b, *W.build_args(c))
    W.assert_same_pages(ds.to_relation(W.SEED), want, what)
    return want


def test_byte_for_byte_small_relations():
    for args in ((800, 100), ()):   # relation(): several pages in every tape, the overflow pages of three tapes interleaved
        c, seg, oix, pages = D.relation(*args)
        pl = D.page_list(pages)
        (docs, toks, sums, blks), _ = D.tapes(pl)
        if not args:
            assert min(len(docs), len(toks), len(sums), len(blks)) > 1
        check_round_trip(pl, f"relation{args} read on the device")
        W.assert_same_pages(check_built(c, f"relation{args} built on the device"), pl, "the two oracle relations")
    check_round_trip(W.oracle_relation(D.terms_of_interest_segment()), "terms of interest")
    one = W.docs_corpus(1, n_terms=1)
    check_round_trip(check_built(one, "1 document, 1 term, built on the device"), "1 document, 1 term")


def test_empty_segment():
    """0 documents: every tape is one empty page, both address tapes one empty page, start_* NONE"""
    ds = vb.DeviceSegment.from_pages(D.empty_relation())
    assert (ds.n_docs, ds.n_terms, ds.n_blocks) == (0, 0, 0)
    want = W.oracle_relation(ds.download())
    got = ds.to_relation(W.SEED)
    W.assert_same_pages(got, want, "empty segment")
    j = W.jump_fields(got)
    assert len(got) == 10 and ds.page_count() == 6 and j["start_documents"] == j["start_tokens"] == W.NONE
    assert vb.segment_from_pages(got).n_docs == 0


@pytest.mark.parametrize("n_terms", [225, 226, 227, 290, 291, 292, 2000])
def test_token_summary_and_block_pages_exactly_full(n_terms):
    """226 tokens, 291 summaries, 226 one-posting blocks fill a page: one short, exactly full, one over; 2000: several pages of each"""
    seg, pl = D.single_posting_relation(n_terms)
    (docs, toks, sums, blks), _ = D.tapes(pl)
    assert len(toks) == (n_terms + 225) // 226 and len(sums) == (n_terms + 290) // 291 and len(blks) == (n_terms + 225) // 226
    check_round_trip(pl, f"{n_terms} terms of one posting")


@pytest.mark.parametrize("n_docs", [679, 680, 681])
def test_document_pages_exactly_full(n_docs):
    c = W.docs_corpus(n_docs)
    want = check_built(c, f"{n_docs} documents")
    assert len(D.tapes(want)[0][0]) == (n_docs + 679) // 680 and W.jump_fields(want)["width_0_documents"] == min(n_docs, 680)


def deep(extra):
    return cached(("deep", extra), lambda: W.docs_corpus(W.ADDR_DOCS_WIDTH * W.DOCS_PER_PAGE + extra))


@pytest.mark.parametrize("extra,depth", [(0, 1), (1, 2)])
def test_address_documents_gets_a_second_level(extra, depth):
    """2036 x 680 documents fill the documents' address page exactly; one more document is one more page and a second level (17 MB of
    pages, a documents tape of two chunks)"""
    want = check_built(deep(extra), f"2036 x 680 + {extra} documents")
    assert W.jump_fields(want)["depth_documents"] == depth and len(D.tapes(want)[0][0]) == W.ADDR_DOCS_WIDTH + extra


def test_variable_block_tuples():
    """wide_relation(): document widths 1 .. 20, tf widths 1 .. 31, every byte-packed tail, a documents tape of more than one chunk"""
    seg, pl, expect = D.wide_relation()
    assert len(D.tapes(pl)[0][0]) > W.CHUNK_PAGES
    check_round_trip(pl, "wide relation")


def test_past_a_chunk_and_a_grid_pass():
    """single_posting_relation(540 000): three tapes of more than 1024 pages, the tokens and blocks tapes more than 2 x 1024 (three
    chunks, the last one partial), depth_tokens 2.  540 000 blocks are more than the 2048 x 256 threads of next_kernel, double_kernel
    and the scan's tiles: those reach their second grid-stride pass.  The fill kernels and ids_kernel cannot be taken further: a fill
    launch covers one chunk of at most 1024 pages with 1024 waves, ids_kernel's 2048 x 256 threads would need more than 524 288 pages
    of one tape (118 M one-posting terms), so the 1 860 000-term relation adds no path here."""
    seg, pl = cached("540", lambda: D.single_posting_relation(540_000))
    (docs, toks, sums, blks), _ = D.tapes(pl)
    assert min(len(toks), len(blks)) > 2 * W.CHUNK_PAGES and len(sums) > W.CHUNK_PAGES and W.jump_fields(pl)["depth_tokens"] == 2
    assert seg.n_blocks > 2048 * 256
    check_round_trip(pl, "540 000 terms of one posting")


def test_callers_page_ids():
    c, seg, oix, pages = D.relation()
    pl = D.page_list(pages)
    ds = vb.DeviceSegment.build(1.2, 0.75, *W.build_args(c))
    count = ds.page_count()
    assert count == len(pl) - 4
    ids = np.random.default_rng(5).permutation(np.arange(100, 100 + count)).astype(np.uint32)
    got, flushed = ds.write_pages(page_ids=ids)
    assert sorted(got) == list(range(100, 100 + count))   # each id delivered (a dict: once is checked by the sequence below)
    seen = []
    ds.write_pages(page_ids=ids, write_page=lambda i, image: seen.append(i))
    assert sorted(seen) == list(range(100, 100 + count)) and len(set(seen)) == count
    # vbm25_flushed: the oracle relation's Jump fields through the permutation
    want = W.jump_fields(pl)
    for name, v in want.items():
        mapped = int(ids[v - 1]) if name in W.PAGE_FIELDS and v != W.NONE else v
        assert flushed[name] == mapped, name
    # un-permuted: the sequential images -- pages, next fields, summary and token pointers, address entries
    back = W.unmap_flush(got, ids, pl)
    W.assert_same_pages(back[1:], pl[1:count + 1], "un-permuted")
    # round trip through the host reader, the four fixed pages wrapped around the flush here
    rel = W.wrap_flush(got, flushed, 1.2, 0.75, W.SEED, 100 + count, 101 + count, 102 + count)
    host, down = vb.segment_from_pages(W.reader_of(rel)), ds.download()
    assert host.meta() == down.meta()
    for name, a in down.arrays().items():
        assert np.array_equal(host.arrays()[name].reshape(-1), a.reshape(-1)), name
    # first_page = 7: the sequential result, shifted
    got7, flushed7 = ds.write_pages(first_page=7)
    assert sorted(got7) == list(range(7, 7 + count))
    W.assert_same_pages(W.unmap_flush(got7, np.arange(7, 7 + count), pl)[1:], pl[1:count + 1], "first_page = 7")
    for name, v in want.items():
        assert flushed7[name] == (v + 6 if name in W.PAGE_FIELDS and v != W.NONE else v), name


def test_after_a_compaction():
    c = D.relation(n_docs=5000, vocab=300, seed=9)[0]
    seg = W.host_segment(c)
    gix = vb.GpuIndex(seg)
    keys = seg.arrays()["term_key"]
    G = make_growing_new_keys(keys, 300, seed=7)
    G2, _ = make_growing(keys, 200, seed=8, deleted=0.1)
    G = {k: np.concatenate([G[k], G2[k] if k != "g_start" else G2[k][1:] + G[k][-1]]) for k in G}
    ds = vb.DeviceSegment.maintain(gix, np.random.default_rng(1).random(seg.n_docs) < 0.2, G)
    rel = ds.to_relation(W.SEED)
    W.assert_same_pages(rel, W.oracle_relation(ds.download()), "compacted")
    # served from the written relation as from the compacted segment
    cix, rix = vb.GpuIndex(ds), vb.GpuIndex(vb.DeviceSegment.from_pages(rel))
    rng = np.random.default_rng(2)
    terms = np.sort(np.stack([rng.choice(ds.n_terms, 3, replace=False) for _ in range(32)]), axis=1).reshape(-1).astype(np.uint32)
    off = (np.arange(33) * 3).astype(np.uint32)
    h1, n1 = vb.search_batch(cix, terms, off, 10)
    h2, n2 = vb.search_batch(rix, terms, off, 10)
    assert n1.sum() > 0 and np.array_equal(n1, n2) and h1.tobytes() == h2.tobytes()


def test_refused_arguments():
    c, seg, oix, pages = D.relation(800, 100)
    pl = D.page_list(pages)
    ds = vb.DeviceSegment.build(1.2, 0.75, *W.build_args(c))
    count = ds.page_count()
    ids = np.arange(50, 50 + count, dtype=np.uint32)
    for what, kw in (("one id short", dict(page_ids=ids[:-1])), ("one id more", dict(page_ids=np.append(ids, 7))),
                     ("an id that is no page", dict(page_ids=np.where(ids == 60, W.NONE, ids))),
                     ("an id twice", dict(page_ids=np.where(ids == 60, 61, ids))),
                     ("ids beyond 2^32 - 1", dict(first_page=2**32 - count)), ("the first id 2^32 - 1", dict(first_page=2**32 - 1))):
        with pytest.raises(vb.Vbm25Error) as e:
            ds.write_pages(**kw)
        assert e.value.code == -1, what
    got, _ = ds.write_pages(first_page=2**32 - 1 - count)   # the last id is 2^32 - 2: fine
    assert max(got) == 2**32 - 2 and len(got) == count
    W.assert_same_pages(ds.to_relation(W.SEED), pl, "after the refusals")


def test_a_callback_that_stops_the_write():
    """write_page returns 1 at the 3rd page of the 2nd chunk: -1 naming that page; the segment then writes and serves as before"""
    c = deep(1)
    want = W.oracle_relation(W.host_segment(c))
    ds = vb.DeviceSegment.build(1.2, 0.75, *W.build_args(c))
    calls = []

    def stop(page_id, image):
        calls.append(page_id)
        return int(len(calls) == W.CHUNK_PAGES + 3)
    with pytest.raises(vb.Vbm25Error) as e:
        ds.write_pages(write_page=stop)
    assert e.value.code == -1 and len(calls) == W.CHUNK_PAGES + 3 and f"page {calls[-1]}:" in str(e.value), str(e.value)
    W.assert_same_pages(ds.to_relation(W.SEED), want, "after the stopped write")
    gix = vb.GpuIndex(ds)
    terms, off = np.array([0, 1, 2], np.uint32), np.array([0, 3], np.uint32)
    hits, n_hits = vb.search_batch(gix, terms, off, 10)
    down = ds.download()   # (its arrays are views: the segment has to outlive them)
    oix = orc.OracleIndex.from_arrays(down.meta(), down.arrays())
    ref, n_ref, _ = oix.search_batch(terms, off, 10, mode="brute", threads=4)
    assert n_hits[0] > 0 and np.array_equal(n_hits, n_ref) and np.array_equal(hits["doc_id"], ref["doc_id"])


def test_four_threads_write_four_segments():
    cases = [D.relation(800 + 300 * i, 100 + 40 * i, seed=20 + i) for i in range(4)]
    segs = [vb.DeviceSegment.build(1.2, 0.75, *W.build_args(c[0])) for c in cases]
    out, errors = [None] * 4, []

    def work(i):
        try:
            out[i] = [segs[i].to_relation(W.SEED) for _ in range(3)][-1]
        except Exception as e:   # noqa: BLE001 (reported below)
            errors.append((i, e))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(4):
        W.assert_same_pages(out[i], D.page_list(cases[i][3]), f"thread {i}")
