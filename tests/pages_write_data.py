"""Segments and helpers for the device writer's tests (tests/test_gpu_pages_write.py, tests/test_pages_write_host.py): corpora whose
tapes end exactly at, one short of and one past a page, the oracle's relation of a segment, the four pages build.rs puts around a
flush, and the inverse of a page id mapping applied to a written relation.  No GPU use."""
import struct

import numpy as np

import orc
import vectorchord_bm25_amd as vb
import pages_device_data as D

NONE = 0xFFFFFFFF
SEED = bytes(range(32))
DOCS_PER_PAGE, TOKENS_PER_PAGE, SUMMARIES_PER_PAGE = 680, 226, 291   # csrc/pages_emit.h
ADDR_DOCS_WIDTH, ADDR_TOKENS_WIDTH = 2036, 407
CHUNK_PAGES = 1024


def build_args(c):
    return (c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])


def docs_corpus(n_docs, seed=0, n_terms=3):
    """n_docs documents and a handful of postings (n_terms terms of up to five): a relation that is long in documents only"""
    rng = np.random.default_rng(seed + n_docs)
    post_doc, post_tf, term_start = [], [], [0]
    for _ in range(n_terms):
        df = min(n_docs, 5)
        post_doc.append(np.sort(rng.choice(n_docs, df, replace=False)).astype(np.uint32))
        post_tf.append(rng.integers(1, 9, df).astype(np.uint32))
        term_start.append(term_start[-1] + df)
    post_doc, post_tf = np.concatenate(post_doc), np.concatenate(post_tf)
    doc_len = rng.integers(1, 500, n_docs).astype(np.uint32)
    doc_len[post_doc] += 20
    ids = np.arange(n_docs)
    payload = np.stack([ids >> 16, ids & 0xffff, ids % 64 + 1], axis=1).astype(np.uint16)
    keys = np.zeros((n_terms, 16), np.uint8)
    for t in range(n_terms):
        keys[t, :2] = np.frombuffer(b"d%d" % t, np.uint8)
    return dict(doc_len=doc_len, doc_payload=payload, term_key=keys, term_start=np.array(term_start, np.uint64), post_doc=post_doc, post_tf=post_tf)


def host_segment(c, k1=1.2, b=0.75):
    return vb.Segment.build(k1, b, *build_args(c))


def oracle_relation(seg, seed=SEED):
    """the oracle's writer (orc_pages_build) on the segment's arrays: the comparator of every test"""
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    return D.page_list(orc.Pages(oix, seed=seed))


def assert_same_pages(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(np.asarray(g), np.asarray(w)):
            at = int(np.flatnonzero(np.asarray(g) != np.asarray(w))[0])
            raise AssertionError(f"{what}: page {i} differs from the oracle's at byte {at}")


def jump_fields(pl):
    """the Jump tuple of a relation as vbm25_flushed's dict"""
    _, (ptr_jump, joff) = D.tapes(pl)
    v = struct.unpack_from("<IIQHHIIIIIIIIII", bytes(pl[ptr_jump]), joff)
    names = ("number_of_documents", "sum_of_document_lengths", "width_1_documents", "width_0_documents", "depth_documents", "start_documents",
             "free_documents", "depth_tokens", "start_tokens", "free_tokens", "ptr_documents", "ptr_tokens", "ptr_summaries", "ptr_blocks")
    return dict(zip(names, v[1:]))


PAGE_FIELDS = ("start_documents", "free_documents", "start_tokens", "free_tokens", "ptr_documents", "ptr_tokens", "ptr_summaries", "ptr_blocks")


def back_chain(pl, head):
    out = []
    while head != NONE:
        out.append(head)
        head = D.next_page(pl[head])
    return out


def unmap_flush(pages, ids, oracle_pl):
    """`pages`: dict page id -> image of a flush whose i-th allocation got ids[i].  Returns the images with every page id in them (next,
    a summary's block, a token's first summary, the address entries) mapped back to 1 + i, as a list indexed by 1 + i (entry 0: None).
    Which page is of which kind is read off the ORACLE's relation of the same segment (`oracle_pl`), whose flush is pages 1 ..."""
    inv = {int(p): 1 + i for i, p in enumerate(ids)}
    (docs, toks, sums, blks), _ = D.tapes(oracle_pl)
    j = jump_fields(oracle_pl)
    adocs, atoks = back_chain(oracle_pl, j["free_documents"]), back_chain(oracle_pl, j["free_tokens"])
    kind = {}
    for name, tape in (("docs", docs), ("toks", toks), ("sums", sums), ("blks", blks), ("adocs", adocs), ("atoks", atoks)):
        kind.update({p: name for p in tape})
    assert sorted(kind) == list(range(1, len(ids) + 1))
    out = [None] * (len(ids) + 1)

    def back(pg, at):
        v = struct.unpack_from("<I", pg, at)[0]
        if v != NONE:
            struct.pack_into("<I", pg, at, inv[v])

    for i, p in enumerate(ids):
        pg = bytearray(pages[int(p)].tobytes())
        back(pg, 8184)
        k = kind[1 + i]
        for off, ln in D.slots(pg):
            if k == "sums":
                back(pg, off + 8)
            elif k == "toks":
                back(pg, off + 18)
            elif k in ("adocs", "atoks"):
                s, e = struct.unpack_from("<HH", pg, off)
                step = 4 if k == "adocs" else 20
                for at in range(off + s, off + e, step):
                    back(pg, at + step - 4)
        out[1 + i] = np.frombuffer(bytes(pg), np.uint8)
    return out


def wrap_flush(pages, flushed, k1, b, seed, vectors, jump, lock):
    """the four pages build.rs:40-70 puts around a flush (laid out as tests/golden/make_page_fixture.py lays pages out), added to a copy
    of `pages`: Meta at 0, the empty vectors tape, the Jump tuple and the lock page at the ids given"""
    f = flushed
    jt = struct.pack("<IIQHHIIIIIIIIII", vectors, f["number_of_documents"], f["sum_of_document_lengths"], f["width_1_documents"],
                     f["width_0_documents"], f["depth_documents"], f["start_documents"], f["free_documents"], f["depth_tokens"], f["start_tokens"],
                     f["free_tokens"], f["ptr_documents"], f["ptr_tokens"], f["ptr_summaries"], f["ptr_blocks"]) + bytes(4)
    mt = b"vchordbm" + struct.pack("<QddII", 1, k1, b, lock, jump) + bytes(seed)
    assert len(jt) == 64 and len(mt) == 72
    out = dict(pages)
    assert not {0, vectors, jump, lock} & set(out)
    out[0], out[vectors], out[jump], out[lock] = D._page([mt]), D._page([]), D._page([jt]), D._page([])
    return out


def reader_of(pages):
    """a page reader (page id -> address) over a dict of images, as segment_from_pages takes it"""
    return lambda i: pages[i].ctypes.data if i in pages else None


def write_relation_file(path, relations):
    """tests/native/fuzz_pages_write.cpp's case file: u32 n_relations, per relation u32 n_pages and the images"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(relations)))
        for pl in relations:
            f.write(struct.pack("<I", len(pl)))
            for p in pl:
                f.write(np.asarray(p).tobytes())
