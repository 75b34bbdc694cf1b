"""Python host mirror of the reference's interface for the query path.

Names follow the reference (crates/bm25): `intern` (vector.rs:19-35), `Query`
(vector.rs:96-134), `search(index, k, query)` (search.rs:28-36).  Everything here is a thin
wrapper over the C ABI in include/vbm25.h; no computation happens in Python.
"""
import ctypes as C
import weakref

import numpy as np

from ._lib import Flushed, IndexDesc, SynthParams, Vbm25Error, check, lib

HIT_DTYPE = np.dtype({"names": ["score", "doc_id", "payload"],
                      "formats": ["<f8", "<u4", ("<u2", (3,))],
                      "offsets": [0, 8, 12], "itemsize": 24})

# vbm25_rank: one entry of Scorer.topk's rows
RANK_DTYPE = np.dtype({"names": ["score", "pos", "doc"], "formats": ["<f8", "<u4", "<u4"], "offsets": [0, 8, 12], "itemsize": 16})

WIDTH = 16  # crates/bm25/src/lib.rs:37

_DESC_ARRAYS = [
    ("term_key", np.uint8), ("term_df", np.uint32), ("term_wand_fn", np.uint8),
    ("term_wand_tf", np.uint32), ("term_first_block", np.uint32), ("blk_min_doc", np.uint32),
    ("blk_max_doc", np.uint32), ("blk_n", np.uint8), ("blk_wand_fn", np.uint8),
    ("blk_wand_tf", np.uint32), ("blk_meta_doc", np.uint8), ("blk_meta_tf", np.uint8),
    ("blk_off8", np.uint32), ("blob", np.uint8), ("doc_fieldnorm", np.uint8),
    ("doc_payload", np.uint16),
]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def intern(string: bytes, seed: bytes = None) -> bytes:
    """vector.rs:19-35: strings shorter than 16 bytes without NUL are zero padded; the others are the first
    16 bytes of blake3::keyed_hash(seed, string) with the last byte forced non-zero.  `seed` = MetaTuple.seed
    of the index (pages_seed())."""
    string = bytes(string)
    out = (C.c_uint8 * WIDTH)()
    if seed is not None and len(seed) != 32:
        raise ValueError("the seed is 32 bytes")
    check(lib().vbm25_intern(seed, string, len(string), out))
    return bytes(out)


class Query:
    """Sorted, de-duplicated token keys (vector.rs:96-134)."""

    def __init__(self, keys):
        keys = [bytes(k) for k in keys]
        if any(len(k) != WIDTH for k in keys) or any(a >= b for a, b in zip(keys, keys[1:])):
            raise ValueError("invalid data")  # Query::new -> expect("invalid data")
        self.keys = keys

    @classmethod
    def from_tokens(cls, tokens, seed=None):
        """cast_tsvector_to_query (src/datatype/tsvector.rs:96-105): intern, sort, dedup."""
        return cls(sorted({intern(t, seed) for t in tokens}))


class Segment:
    """Host-side sealed segment (flattened arrays), built by the library."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        self.desc = IndexDesc()
        check(lib().vbm25_segment_desc(self.h, C.byref(self.desc)))

    @classmethod
    def build(cls, k1, b, doc_len, doc_payload, term_key, term_start, post_doc, post_tf, threads=0):
        doc_len = np.ascontiguousarray(doc_len, dtype=np.uint32)
        doc_payload = np.ascontiguousarray(doc_payload, dtype=np.uint16)
        term_key = np.ascontiguousarray(term_key, dtype=np.uint8)
        term_start = np.ascontiguousarray(term_start, dtype=np.uint64)
        post_doc = np.ascontiguousarray(post_doc, dtype=np.uint32)
        post_tf = np.ascontiguousarray(post_tf, dtype=np.uint32)
        out = C.c_void_p()
        check(lib().vbm25_segment_build(k1, b, len(doc_len), _p(doc_len), _p(doc_payload),
                                        len(term_start) - 1, _p(term_key), _p(term_start),
                                        _p(post_doc), _p(post_tf), threads, C.byref(out)))
        return cls(out)

    @classmethod
    def build_device(cls, k1, b, doc_len, doc_payload, term_key, term_start, post_doc, post_tf, device=0):
        """vbm25_segment_build_device: the same segment, encoded by the GPU (csrc/flush.hip)."""
        doc_len = np.ascontiguousarray(doc_len, dtype=np.uint32)
        doc_payload = np.ascontiguousarray(doc_payload, dtype=np.uint16)
        term_key = np.ascontiguousarray(term_key, dtype=np.uint8)
        term_start = np.ascontiguousarray(term_start, dtype=np.uint64)
        post_doc = np.ascontiguousarray(post_doc, dtype=np.uint32)
        post_tf = np.ascontiguousarray(post_tf, dtype=np.uint32)
        out = C.c_void_p()
        check(lib().vbm25_segment_build_device(device, k1, b, len(doc_len), _p(doc_len), _p(doc_payload),
                                               len(term_start) - 1, _p(term_key), _p(term_start),
                                               _p(post_doc), _p(post_tf), C.byref(out)))
        return cls(out)

    @classmethod
    def build_device_unsorted(cls, k1, b, doc_len, doc_payload, term_key, map_term, map_doc, map_tf, device=0):
        """vbm25_segment_build_device_unsorted: (token rank, document, tf) triples in any order; the device sorts and encodes."""
        doc_len = np.ascontiguousarray(doc_len, dtype=np.uint32)
        doc_payload = np.ascontiguousarray(doc_payload, dtype=np.uint16)
        term_key = np.ascontiguousarray(term_key, dtype=np.uint8)
        map_term = np.ascontiguousarray(map_term, dtype=np.uint32)
        map_doc = np.ascontiguousarray(map_doc, dtype=np.uint32)
        map_tf = np.ascontiguousarray(map_tf, dtype=np.uint32)
        out = C.c_void_p()
        check(lib().vbm25_segment_build_device_unsorted(device, k1, b, len(doc_len), _p(doc_len), _p(doc_payload),
                                                        len(term_key), _p(term_key), len(map_term), _p(map_term),
                                                        _p(map_doc), _p(map_tf), C.byref(out)))
        return cls(out)

    @classmethod
    def synth(cls, n_docs, vocab, mean_len=100, len_mode=1, zipf_s=0.0, k1=1.2, b=0.75,
              seed=20260925, threads=0):
        p = SynthParams(n_docs, vocab, mean_len, len_mode, zipf_s, k1, b, seed, threads, 0)
        out = C.c_void_p()
        check(lib().vbm25_segment_synth(C.byref(p), C.byref(out)))
        return cls(out)

    @classmethod
    def load(cls, path):
        out = C.c_void_p()
        check(lib().vbm25_segment_load(path.encode(), C.byref(out)))
        return cls(out)

    def save(self, path):
        check(lib().vbm25_segment_save(self.h, path.encode()))

    def __del__(self):
        try:
            lib().vbm25_segment_free(self.h)
        except Exception:
            pass

    @property
    def n_docs(self):
        return self.desc.n_docs

    @property
    def n_terms(self):
        return self.desc.n_terms

    @property
    def n_blocks(self):
        return self.desc.n_blocks

    def arrays(self):
        """numpy views (no copy) of the flattened arrays; valid while self is alive."""
        d = self.desc
        sizes = {"term_key": 16 * d.n_terms, "term_df": d.n_terms, "term_wand_fn": d.n_terms,
                 "term_wand_tf": d.n_terms, "term_first_block": d.n_terms + 1,
                 "blk_min_doc": d.n_blocks, "blk_max_doc": d.n_blocks, "blk_n": d.n_blocks,
                 "blk_wand_fn": d.n_blocks, "blk_wand_tf": d.n_blocks, "blk_meta_doc": d.n_blocks,
                 "blk_meta_tf": d.n_blocks, "blk_off8": d.n_blocks + 1, "blob": d.blob_bytes,
                 "doc_fieldnorm": d.n_docs, "doc_payload": 3 * d.n_docs}
        out = {}
        for name, dt in _DESC_ARRAYS:
            n = sizes[name]
            ptr = getattr(d, name)
            if n == 0 or not ptr:
                out[name] = np.zeros(0, dtype=dt)
                continue
            buf = (C.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(ptr)
            out[name] = np.frombuffer(buf, dtype=dt)
        out["term_key"] = out["term_key"].reshape(-1, 16)
        out["doc_payload"] = out["doc_payload"].reshape(-1, 3)
        return out

    def meta(self):
        d = self.desc
        return dict(n_docs=d.n_docs, n_terms=d.n_terms, n_blocks=d.n_blocks, sum_len=d.sum_len,
                    k1=d.k1, b=d.b)

    def token_terms(self, tokens):
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        out = np.zeros(len(tokens), dtype=np.uint32)
        check(lib().vbm25_segment_synth_token_terms(self.h, _p(tokens), len(tokens), _p(out)))
        return out

    def query_bytes(self, term_ids, k):
        term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
        return int(lib().vbm25_query_bytes(C.byref(self.desc), _p(term_ids), len(term_ids), k))


def _deleted_words(sealed_deleted, n_docs):
    """vbm25_index_maintain's / vbm25_filter_remap's sealed_deleted: None, a bool array of n_docs (True = deleted) or the packed
    uint64 words -> None or the words"""
    if sealed_deleted is None:
        return None
    a = np.asarray(sealed_deleted)
    if a.dtype == np.bool_:
        if len(a) != n_docs:
            raise ValueError(f"{len(a)} deleted flags for {n_docs} documents")
        words = np.zeros((n_docs + 63) // 64, dtype=np.uint64)
        idx = np.flatnonzero(a)
        np.bitwise_or.at(words, idx >> 6, np.left_shift(np.uint64(1), (idx & 63).astype(np.uint64)))
        return words
    words = np.ascontiguousarray(a, dtype=np.uint64)
    if len(words) != (n_docs + 63) // 64:
        raise ValueError(f"{len(words)} words for {n_docs} documents")
    return words


class DeviceSegment:
    """A sealed segment that lives in HBM (vbm25_device_segment): built or generated on the device, never downloaded unless
    asked (download() -> Segment).  GpuIndex(device_segment) makes the index of it without a round trip through the host."""

    def __init__(self, handle):
        self.h = handle
        nd, nt, nb, npost = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(lib().vbm25_device_segment_info(self.h, C.byref(nd), C.byref(nt), C.byref(nb), C.byref(npost)))
        self.n_docs, self.n_terms, self.n_blocks, self.n_postings = nd.value, nt.value, nb.value, npost.value

    @classmethod
    def synth(cls, n_docs, vocab, mean_len=100, len_mode=1, zipf_s=0.0, k1=1.2, b=0.75, seed=20260925, device=0):
        p = SynthParams(n_docs, vocab, mean_len, len_mode, zipf_s, k1, b, seed, 0, 0)
        out = C.c_void_p()
        check(lib().vbm25_device_segment_synth(C.byref(p), device, C.byref(out)))
        return cls(out)

    @classmethod
    def build(cls, k1, b, doc_len, doc_payload, term_key, term_start, post_doc, post_tf, device=0):
        doc_len = np.ascontiguousarray(doc_len, dtype=np.uint32)
        doc_payload = np.ascontiguousarray(doc_payload, dtype=np.uint16)
        term_key = np.ascontiguousarray(term_key, dtype=np.uint8)
        term_start = np.ascontiguousarray(term_start, dtype=np.uint64)
        post_doc = np.ascontiguousarray(post_doc, dtype=np.uint32)
        post_tf = np.ascontiguousarray(post_tf, dtype=np.uint32)
        out = C.c_void_p()
        check(lib().vbm25_device_segment_build(device, k1, b, len(doc_len), _p(doc_len), _p(doc_payload), len(term_start) - 1,
                                               _p(term_key), _p(term_start), _p(post_doc), _p(post_tf), C.byref(out)))
        return cls(out)

    @classmethod
    def from_documents(cls, documents, k1, b):
        """vbm25_device_segment_build_documents: the index ambuild makes of cast Documents (document i = doc id i, the vocabulary =
        their distinct keys), sorted, ranked and encoded on the documents' device; download() is byte for byte Segment.build of
        the same vocabulary and mappings."""
        out = C.c_void_p()
        check(lib().vbm25_device_segment_build_documents(documents.h, k1, b, C.byref(out)))
        return cls(out)

    @classmethod
    def from_pages(cls, pages, device=0):
        """vbm25_device_segment_from_pages: the sealed segment of a bm25 index relation in the reference's on-disk format, read into
        the HBM of `device` (the host follows the page chains, kernels parse, validate and flatten the tuples).  `pages` as
        segment_from_pages takes it: a sequence of 8192-byte page images or a callable page_id -> address.  download() of the
        result is byte for byte segment_from_pages(pages)."""
        cb, keep = _page_reader(pages)
        out = C.c_void_p()
        check(lib().vbm25_device_segment_from_pages(C.cast(cb, C.c_void_p), None, device, C.byref(out)))
        return cls(out)

    @classmethod
    def maintain(cls, index, sealed_deleted=None, growing=None, return_relabel=False):
        """vbm25_index_maintain: VACUUM's compaction of `index` (a GpuIndex) on its device.  sealed_deleted: None, a bool array of
        n_docs (True = deleted) or the packed uint64 words; growing: None or a dict of growing_data.make_growing's form (g_start,
        g_key, g_tf, g_payload, g_deleted; g_fieldnorm is not read).  Returns the new DeviceSegment, and with return_relabel the
        uint32 array old sealed ids + growing indexes -> new id (0xFFFFFFFF: dropped)."""
        n_docs = index.n_docs
        words = _deleted_words(sealed_deleted, n_docs)
        d, keep, n_grow = None, [], 0
        if growing is not None:
            g_start = np.ascontiguousarray(growing["g_start"], dtype=np.uint64)
            g_key = np.ascontiguousarray(growing["g_key"], dtype=np.uint8).reshape(-1)
            g_tf = np.ascontiguousarray(growing["g_tf"], dtype=np.uint32)
            g_payload = np.ascontiguousarray(growing["g_payload"], dtype=np.uint16).reshape(-1)
            g_del = growing.get("g_deleted")
            g_del = None if g_del is None else np.ascontiguousarray(g_del, dtype=np.uint8)
            if len(g_key) != 16 * len(g_tf):
                raise ValueError(f"{len(g_key)} key bytes for {len(g_tf)} elements")
            keep = [g_start, g_key, g_tf, g_payload, g_del]
            n_grow = len(g_start) - 1
            d = GrowingDesc()
            d.n_docs, d.n_elements = n_grow, len(g_tf)
            d.start, d.key, d.tf = _p(g_start), _p(g_key), _p(g_tf)
            d.fieldnorm, d.payload, d.deleted = None, _p(g_payload), _p(g_del)
        relabel = np.zeros(n_docs + n_grow, dtype=np.uint32) if return_relabel else None
        out = C.c_void_p()
        check(lib().vbm25_index_maintain(index.h, _p(words), C.byref(d) if d is not None else None,
                                         relabel.ctypes.data_as(C.c_void_p) if relabel is not None else None, C.byref(out)))
        seg = cls(out)
        return (seg, relabel) if return_relabel else seg

    @classmethod
    def maintain_device(cls, index, vacuum, return_relabel=False):
        """vbm25_index_maintain_device: maintain(index, words, csr) with the deletion words and the growing CSR taken from a
        DeviceVacuum's planes in HBM -- the same segment and relabel byte for byte, nothing of the inputs but the index's term keys
        crossing the host link.  The handle is only read: it serves remap_device and further compactions afterwards."""
        relabel = np.zeros(index.n_docs + vacuum.n_grow, dtype=np.uint32) if return_relabel else None
        out = C.c_void_p()
        check(lib().vbm25_index_maintain_device(index.h, vacuum.h, relabel.ctypes.data_as(C.c_void_p) if relabel is not None else None,
                                                C.byref(out)))
        seg = cls(out)
        return (seg, relabel) if return_relabel else seg

    def download(self):
        out = C.c_void_p()
        check(lib().vbm25_device_segment_download(self.h, C.byref(out)))
        return Segment(out)

    def page_count(self):
        """vbm25_device_segment_page_count: the pages a flush of this segment allocates (four tapes and both address tapes)."""
        n = C.c_uint32()
        check(lib().vbm25_device_segment_page_count(self.h, C.byref(n)))
        return n.value

    def write_pages(self, page_ids=None, first_page=0, write_page=None):
        """vbm25_device_segment_write_pages: the segment as the reference's page images, laid out and filled on the device.  The
        i-th page allocation of flush.rs gets page_ids[i] (None: first_page + i).  Returns (dict page id -> np.uint8[8192], dict of
        vbm25_flushed's fields: what goes into the Jump tuple).  write_page(page_id, address): called instead of collecting the
        pages (the image is valid during the call only; a non-zero return stops the write); the dict then stays empty."""
        pages = {}
        if write_page is None:
            def cb(ctx, page_id, image):
                pages[page_id] = np.frombuffer(C.string_at(image, 8192), dtype=np.uint8).copy()
                return 0
        else:
            def cb(ctx, page_id, image):
                return int(write_page(page_id, image) or 0)
        fn = WRITE_PAGE_FN(cb)
        ids, n_ids = None, 0
        if page_ids is not None:
            ids = np.ascontiguousarray(page_ids, dtype=np.uint32)
            n_ids = len(ids)
        f = Flushed()
        check(lib().vbm25_device_segment_write_pages(self.h, _p(ids), n_ids, first_page, C.cast(fn, C.c_void_p), None, C.byref(f)))
        return pages, {name: getattr(f, name) for name, _ in Flushed._fields_ if name != "_pad"}

    def to_relation(self, seed=None):
        """vbm25_device_segment_write_relation: a whole fresh relation of this segment as build.rs:22-71 writes it (Meta page 0 with
        the segment's k1 and b and `seed` -- 32 bytes, None: zeros --, the flush, the empty vectors tape, Jump, lock): the list of
        its page images, indexable by page id, as segment_from_pages and DeviceSegment.from_pages take it."""
        if seed is not None and len(seed) != 32:
            raise ValueError("the seed is 32 bytes")
        pages = {}

        def cb(ctx, page_id, image):
            pages[page_id] = np.frombuffer(C.string_at(image, 8192), dtype=np.uint8).copy()
            return 0
        fn = WRITE_PAGE_FN(cb)
        seed_buf = (C.c_uint8 * 32).from_buffer_copy(bytes(seed)) if seed is not None else None
        n = C.c_uint32()
        check(lib().vbm25_device_segment_write_relation(self.h, seed_buf, C.cast(fn, C.c_void_p), None, C.byref(n)))
        if sorted(pages) != list(range(n.value)):
            raise Vbm25Error(-1, f"{len(pages)} distinct pages delivered for a relation of {n.value}")
        return [pages[i] for i in range(n.value)]

    def token_terms(self, tokens):
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        out = np.zeros(len(tokens), dtype=np.uint32)
        check(lib().vbm25_device_segment_token_terms(self.h, _p(tokens), len(tokens), _p(out)))
        return out

    def query_bytes(self, term_ids, k):
        term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
        return int(lib().vbm25_device_segment_query_bytes(self.h, _p(term_ids), len(term_ids), k))

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_device_segment_free(self.h)
        except Exception:
            pass


def desc_from_arrays(meta, arrays):
    """IndexDesc over caller-owned numpy arrays (returns (desc, keepalive))."""
    keep = {}
    d = IndexDesc()
    d.n_docs, d.n_terms, d.n_blocks = meta["n_docs"], meta["n_terms"], meta["n_blocks"]
    d.sum_len, d.k1, d.b = meta["sum_len"], meta["k1"], meta["b"]
    for name, dt in _DESC_ARRAYS:
        a = np.ascontiguousarray(arrays[name], dtype=dt)
        keep[name] = a
        setattr(d, name, a.ctypes.data if a.size else None)
    d.blob_bytes = keep["blob"].size
    return d, keep


class GpuIndex:
    """HBM-resident sealed segment (vbm25_index)."""

    def __init__(self, segment_or_desc, device=0, keepalive=None):
        self.h = C.c_void_p()
        if isinstance(segment_or_desc, DeviceSegment):  # already in HBM: vbm25_index_create_from_device (on the segment's device)
            self.n_terms, self.n_docs = segment_or_desc.n_terms, segment_or_desc.n_docs
            check(lib().vbm25_index_create_from_device(segment_or_desc.h, C.byref(self.h)))
            return
        desc = segment_or_desc.desc if isinstance(segment_or_desc, Segment) else segment_or_desc
        self.n_terms = desc.n_terms
        self.n_docs = desc.n_docs
        check(lib().vbm25_index_create(C.byref(desc), device, C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_index_destroy(self.h)
        except Exception:
            pass

    @property
    def device_bytes(self):
        return int(lib().vbm25_index_device_bytes(self.h))

    def bind(self):
        """vbm25_index_bind: the forward index of the index's own sealed documents, made on the device from the index's arrays in HBM
        -> DocTerms of n_docs documents in the index's order (document d is sealed document d).  What Documents.bind gives for the
        documents the index was built from; valid for this index only (bind again after a compaction)."""
        out = C.c_void_p()
        check(lib().vbm25_index_bind(self.h, C.byref(out)))
        return DocTerms(out, index=self)

    def lookup_terms(self, keys):
        """address_tokens::read for a list of 16-byte keys -> term ids (0xffffffff = absent)."""
        buf = np.frombuffer(b"".join(keys), dtype=np.uint8) if keys else np.zeros(0, np.uint8)
        out = np.zeros(len(keys), dtype=np.uint32)
        check(lib().vbm25_lookup_terms(self.h, _p(buf), len(keys), _p(out)))
        return out


class Batch:
    """Device-resident query batch (vbm25_batch)."""

    def __init__(self, index, max_queries, max_total_terms, k):
        self.index, self.k, self.nq, self.max_queries = index, k, 0, max_queries
        self.doc_filter = None
        self.growing = None
        self.h = C.c_void_p()
        check(lib().vbm25_batch_create(index.h, max_queries, max(1, max_total_terms), k,
                                       C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_batch_destroy(self.h)
        except Exception:
            pass

    def set_queries(self, term_ids, q_off):
        term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
        try:
            check(lib().vbm25_batch_set_queries(self.h, _p(term_ids), q_off.ctypes.data_as(C.c_void_p),
                                                len(q_off) - 1))
        except Vbm25Error:
            self.nq = 0  # (a refused query set leaves the batch with none: include/vbm25.h)
            raise
        self.nq = len(q_off) - 1

    def run(self, stream=None):
        check(lib().vbm25_batch_run(self.h, C.c_void_p(stream) if stream else None))

    def fetch(self):
        hits = np.zeros((self.nq, self.k), dtype=HIT_DTYPE)
        n_hits = np.zeros(self.nq, dtype=np.uint32)
        check(lib().vbm25_batch_fetch(self.h, _p(hits) if self.nq else None,
                                      _p(n_hits) if self.nq else None))
        return hits, n_hits

    def set_timing(self, enabled=True):
        check(lib().vbm25_batch_set_timing(self.h, int(enabled)))

    def set_filter(self, doc_filter, q_filter=None):
        """vbm25_batch_set_filter: query q of this and every later query set takes bitmap q_filter[q] of `doc_filter`
        (NO_FILTER, or entries beyond the array: none).  doc_filter=None: no filter."""
        if doc_filter is None:
            check(lib().vbm25_batch_set_filter(self.h, None, None))
            self.doc_filter = None
            return
        sel = np.full(self.max_queries, NO_FILTER, dtype=np.uint32)
        if q_filter is not None:
            q_filter = np.asarray(q_filter, dtype=np.uint32).reshape(-1)
            if len(q_filter) > self.max_queries:
                raise ValueError(f"{len(q_filter)} selectors for a batch of {self.max_queries} queries")
            sel[:len(q_filter)] = q_filter
        check(lib().vbm25_batch_set_filter(self.h, doc_filter.h, _p(sel)))
        self.doc_filter = doc_filter  # (the batch refers to it: kept alive with the batch)

    def set_growing(self, growing):
        """vbm25_batch_set_growing: every later run merges the growing segment (a GrowingSegment of this batch's index) into the
        records; None detaches it."""
        check(lib().vbm25_batch_set_growing(self.h, growing.h if growing is not None else None))
        self.growing = growing  # (the batch refers to it: kept alive with the batch)

    def device_results(self):
        """vbm25_batch_device_results: device addresses of the records and counts (every later run leaves them complete there)."""
        hits, n_hits = C.c_void_p(), C.c_void_p()
        check(lib().vbm25_batch_device_results(self.h, C.byref(hits), C.byref(n_hits)))
        return hits.value, n_hits.value

    def kernel_ms(self):
        ms, n = C.c_double(), C.c_uint32()
        check(lib().vbm25_batch_kernel_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def debug_counts(self):
        """tuning / test aid (not in include/vbm25.h): (work items of the last run, items the first-choice
        kernel handed to scan_many_kernel; (0, 0) on the exhaustive route, which makes no work items)"""
        f = lib().vbm25_batch_debug_counts
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        ni, nf = C.c_uint32(), C.c_uint32()
        check(f(self.h, C.byref(ni), C.byref(nf)))
        return ni.value, nf.value

    def debug_route(self):
        """test aid: 0 general route (plan_kernel), 1 one launch, 2 plan-free scan_range_kernel, 3 scan_win_kernel, 4 exhaustive"""
        f = lib().vbm25_batch_debug_route
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def debug_routes(self):
        """bench / test aid: (queries classed sparse, dense, many-term by the host; work items of the last run on the general route
        that went to the sparse, the dense and the many-term kernel)"""
        f = lib().vbm25_batch_debug_routes
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_uint32 * 6)()
        check(f(self.h, out))
        return tuple(int(x) for x in out)

    def debug_win_launches(self):
        """test aid: 1 = the last run's scan_win_kernel merged in the kernel (one launch), 3 = scan_win_kernel + scan_many_kernel +
        merge_kernel (also the re-run after a one-launch run that gave an item up), 0 = another route"""
        f = lib().vbm25_batch_debug_win_launches
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def debug_win_handover(self):
        """test aid: how the last run's scan_win_kernel handed a query's lists to the merging wave -- 2 = through the LDS (every query
        but the last nq mod 4), 1 = through memory, 0 = it did not merge (three launches, or another route)"""
        f = lib().vbm25_batch_debug_win_handover
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def debug_theta(self, nq):
        """test aid: the thresholds (as float64 scores) the last run ended with; None if the library lacks the entry"""
        f = getattr(lib(), "vbm25_batch_debug_theta", None)
        if f is None:
            return None
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(nq, dtype=np.uint64)
        check(f(self.h, out.ctypes.data))
        return out.view(np.float64)

    def debug_lists(self, q):
        """test aid (not in include/vbm25.h), after a run on the general route: per list of query q's work items, in merge_kernel's
        order, (the entries merge_kernel loads, those of them at or above the query's threshold -- the survivors it ranks)"""
        f = lib().vbm25_batch_debug_lists
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        n = C.c_uint32()
        cap = 1 << 16
        cnt, surv = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        check(f(self.h, int(q), cnt.ctypes.data, surv.ctypes.data, cap, C.byref(n)))
        assert n.value <= cap
        return cnt[:n.value].copy(), surv[:n.value].copy()

    def debug_check(self):
        """-DVBM25_CHECK builds (tools/dense_stress.py): (code, value, item, thread) of the first violated device
        assertion since the last call; code 0 = none.  A library without the entry point reports None."""
        f = getattr(lib(), "vbm25_batch_debug_check", None)
        if f is None:
            return None
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_uint32 * 16)()
        check(f(self.h, out))
        return tuple(int(x) for x in out)


class Stream:
    """The pipelined host-buffer boundary (vbm25_stream_*): up to `depth` batches in flight, first in first out."""

    def __init__(self, index, depth, max_queries, max_total_terms, k):
        self.index, self.k = index, k
        self.h = C.c_void_p()
        L = lib()
        check(L.vbm25_stream_create(index.h, depth, max_queries, max(1, max_total_terms), k, C.byref(self.h)))
        self._nq = []
        self.growing = None     # what the next submit takes (set_growing / set_filter)
        self.doc_filter = None
        self._held = []         # per batch in flight: the (segment, filter) it was submitted with, kept alive until its collect

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_stream_destroy(self.h)
        except Exception:
            pass

    def set_growing(self, growing):
        """vbm25_stream_set_growing: batches submitted from now on merge the growing segment in (None detaches); batches in flight
        keep what they were submitted with.  Waits for nothing."""
        check(lib().vbm25_stream_set_growing(self.h, growing.h if growing is not None else None))
        self.growing = growing

    def set_filter(self, doc_filter):
        """vbm25_stream_set_filter: the filter of later submit(..., q_filter=...) calls (None detaches)."""
        check(lib().vbm25_stream_set_filter(self.h, doc_filter.h if doc_filter is not None else None))
        self.doc_filter = doc_filter

    def submit(self, term_ids, q_off, q_filter=None):
        """vbm25_stream_submit, or with q_filter (one selector per query, NO_FILTER: none) vbm25_stream_submit_filtered."""
        term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
        nq = len(q_off) - 1
        if q_filter is None:
            check(lib().vbm25_stream_submit(self.h, term_ids.ctypes.data if len(term_ids) else None, q_off.ctypes.data, nq))
        else:
            q_filter = np.ascontiguousarray(q_filter, dtype=np.uint32).reshape(-1)
            if len(q_filter) != nq:
                raise ValueError(f"{len(q_filter)} selectors for {nq} queries")
            check(lib().vbm25_stream_submit_filtered(self.h, q_filter.ctypes.data if nq else None,
                                                     term_ids.ctypes.data if len(term_ids) else None, q_off.ctypes.data, nq))
        self._nq.append(nq)  # (only a batch the library accepted is in the ring)
        self._held.append((self.growing, self.doc_filter))

    def collect_raw(self):
        """collect without this object's bookkeeping (tests: the library's own error on an empty ring)"""
        got = C.c_uint32()
        check(lib().vbm25_stream_collect(self.h, None, None, C.byref(got)))

    def collect(self, out=None):
        """The oldest batch in flight: (hits [nq, k], n_hits [nq]).  `out` = (hits, n_hits) arrays to write into."""
        if not self._nq:
            self.collect_raw()  # (the library's own error for an empty ring)
        nq = self._nq[0]
        hits, n_hits = out if out is not None else (np.zeros((nq, self.k), dtype=HIT_DTYPE), np.zeros(nq, dtype=np.uint32))
        if hits.size < nq * self.k or n_hits.size < nq:
            raise ValueError(f"collect: the output arrays hold {hits.size} records / {n_hits.size} counts, the batch needs {nq * self.k} / {nq}")
        got = C.c_uint32()
        check(lib().vbm25_stream_collect(self.h, hits.ctypes.data, n_hits.ctypes.data, C.byref(got)))
        self._nq.pop(0)  # (popped only after the library handed the batch over: an error leaves the bookkeeping in step with the ring)
        if self._held:
            self._held.pop(0)
        assert got.value == nq
        return hits, n_hits

    @property
    def in_flight(self):
        return int(lib().vbm25_stream_in_flight(self.h))


NO_FILTER = 0xFFFFFFFF  # the selector of a query that takes no bitmap


class DocFilter:
    """vbm25_filter: F bitmaps over the index's documents in HBM -- bit d of bitmap i set: document d may be returned.
    `keep` is a bool array [F, n_docs] (or [n_docs] for one bitmap), or a list of F arrays of document ids."""

    def __init__(self, index, keep):
        self.index = index
        self.growing = None  # the GrowingSegment of the growing bitmaps (set_growing)
        self.grow_n = 0      # ... and the number of its documents they cover (set_growing, extend_growing)
        words = self.pack(keep, index.n_docs)
        self.n_bitmaps, self.words = words.shape
        self.h = C.c_void_p()
        check(lib().vbm25_filter_create(index.h, self.n_bitmaps, _p(words), C.byref(self.h)))

    @staticmethod
    def pack(keep, n_docs):
        """-> uint64 words [F, ceil(n_docs / 64)]: bit d % 64 of word d / 64 (least significant first) = keep[d]."""
        if isinstance(keep, np.ndarray) and keep.dtype == np.bool_:
            bits = keep.reshape(1, -1) if keep.ndim == 1 else keep
            if bits.ndim != 2 or bits.shape[1] != n_docs:
                raise ValueError(f"keep has shape {keep.shape}; expected [F, {n_docs}]")
        else:
            bits = np.zeros((len(keep), n_docs), dtype=bool)
            for i, ids in enumerate(keep):
                ids = np.asarray(ids, dtype=np.int64).reshape(-1)
                if ids.size and (ids.min() < 0 or ids.max() >= n_docs):
                    raise ValueError(f"bitmap {i}: document ids outside 0 .. {n_docs - 1}")
                bits[i, ids] = True
        n_words = (n_docs + 63) // 64
        padded = np.zeros((bits.shape[0], 64 * n_words), dtype=bool)
        padded[:, :n_docs] = bits
        return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little").view("<u8"))

    def update(self, i, keep_i):
        """vbm25_filter_update: replace bitmap i (bool array [n_docs] or document ids); takes effect at the next run."""
        words = self.pack(keep_i if isinstance(keep_i, np.ndarray) and keep_i.dtype == np.bool_ else [keep_i], self.index.n_docs)
        check(lib().vbm25_filter_update(self.h, i, _p(words)))

    def device_words(self, i):
        """vbm25_filter_device_words: the device address of bitmap i (ceil(n_docs / 64) uint64 words)."""
        dev = C.c_void_p()
        check(lib().vbm25_filter_device_words(self.h, i, C.byref(dev)))
        return dev.value

    def set_growing(self, growing, keep=None):
        """vbm25_filter_set_growing: F growing bitmaps over the documents of `growing` (a GrowingSegment of this filter's index):
        bit g of growing bitmap i set = growing document g may be returned; query q's selector names sealed and growing bitmap
        alike.  `keep` as in the constructor over growing.n_docs documents (None: all bits zero).  growing=None removes them."""
        if growing is None:
            check(lib().vbm25_filter_set_growing(self.h, None, None))
            self.growing = None
            self.grow_n = 0
            return
        words = None
        if keep is not None:
            words = self.pack(keep, growing.n_docs)
            if words.shape[0] != self.n_bitmaps:
                raise ValueError(f"{words.shape[0]} growing bitmaps for a filter of {self.n_bitmaps}")
        check(lib().vbm25_filter_set_growing(self.h, growing.h, _p(words)))
        self.growing = growing
        self.grow_n = growing.n_docs

    def extend_growing(self, growing, keep_new=None):
        """vbm25_filter_extend_growing: after growing.append(...), extend the F growing bitmaps to the segment's document count in
        place on the device.  `keep_new` as in the constructor over the d = growing.n_docs - (documents covered so far) NEW
        documents (bit j: growing document old count + j); None: all bits zero.  Only the delta crosses the host link."""
        d = growing.n_docs - self.grow_n
        words = None
        if keep_new is not None and d > 0:
            words = self.pack(keep_new, d)
            if words.shape[0] != self.n_bitmaps:
                raise ValueError(f"{words.shape[0]} delta bitmaps for a filter of {self.n_bitmaps}")
        check(lib().vbm25_filter_extend_growing(self.h, growing.h, _p(words)))
        self.growing = growing
        self.grow_n = growing.n_docs

    def update_growing(self, i, keep_i):
        """vbm25_filter_update_growing: replace growing bitmap i (bool array [n_grow] or growing document ids)."""
        if self.growing is None:
            raise ValueError("the filter has no growing bitmaps")
        n = self.growing.n_docs
        words = self.pack(keep_i if isinstance(keep_i, np.ndarray) and keep_i.dtype == np.bool_ else [keep_i], n)
        check(lib().vbm25_filter_update_growing(self.h, i, _p(words)))

    def set_tids(self, i, tid_set, invert=False, growing=None):
        """vbm25_filter_set_tids: sealed bitmap i becomes "the document's payload is in `tid_set`" (invert: "is not"), computed on
        the device from the index's payloads; with `growing` (the GrowingSegment of this filter's growing bitmaps, at its current
        document count) growing bitmap i likewise.  No bitmap crosses the host link."""
        check(lib().vbm25_filter_set_tids(self.h, i, tid_set.h, 1 if invert else 0, growing.h if growing is not None else None))

    def growing_device_words(self, i):
        """vbm25_filter_growing_device_words: the device address of growing bitmap i (ceil(n_grow / 64) uint64 words)."""
        dev = C.c_void_p()
        check(lib().vbm25_filter_growing_device_words(self.h, i, C.byref(dev)))
        return dev.value

    def read(self, i, growing=False):
        """vbm25_filter_read: bitmap i back on the host as uint64 words -- the sealed one (ceil(n_docs / 64) words) or, with
        growing=True, the growing one (ceil(grow_n / 64) words; Vbm25Error when the filter has none)."""
        n = self.grow_n if growing else self.index.n_docs
        words = np.zeros(max(1, (n + 63) // 64), dtype=np.uint64)  # (never a NULL pointer, also for zero words)
        check(lib().vbm25_filter_read(self.h, i, 1 if growing else 0, words.ctypes.data_as(C.c_void_p)))
        return words[:(n + 63) // 64]

    def remap(self, new_index, sealed_deleted=None, growing_deleted=None):
        """vbm25_filter_remap: this filter carried across DeviceSegment.maintain(index, sealed_deleted, growing) on the device.
        `new_index`: the GpuIndex of the compacted segment (or a replica of MultiIndex.from_device); sealed_deleted: what maintain
        got (None, a bool array or the packed words); growing_deleted: the growing segment's g_deleted flags (None: none deleted) --
        without them the growing documents are those this filter's growing bitmaps cover (none: no growing segment was compacted
        in).  Returns the new DocFilter (no growing bitmaps yet); this one is only read and stays valid."""
        words = _deleted_words(sealed_deleted, self.index.n_docs)
        n_grow = self.grow_n
        g_del = None
        if growing_deleted is not None:  # (one flag per growing document of the compaction: the library compares the counts)
            g_del = np.ascontiguousarray(growing_deleted, dtype=np.uint8).reshape(-1)
            n_grow = len(g_del)
        h = C.c_void_p()
        check(lib().vbm25_filter_remap(self.h, _p(words), n_grow, _p(g_del), new_index.h, C.byref(h)))
        f = DocFilter.__new__(DocFilter)
        f.index, f.growing, f.grow_n = new_index, None, 0
        f.n_bitmaps, f.words, f.h = self.n_bitmaps, (new_index.n_docs + 63) // 64, h
        return f

    def remap_device(self, new_index, vacuum):
        """vbm25_filter_remap_device: remap(new_index, words, growing_deleted) with the deletion inputs taken from the DeviceVacuum
        that DeviceSegment.maintain_device compacted: the same words, no array crossing the host link."""
        h = C.c_void_p()
        check(lib().vbm25_filter_remap_device(self.h, vacuum.h, new_index.h, C.byref(h)))
        f = DocFilter.__new__(DocFilter)
        f.index, f.growing, f.grow_n = new_index, None, 0
        f.n_bitmaps, f.words, f.h = self.n_bitmaps, (new_index.n_docs + 63) // 64, h
        return f

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_filter_destroy(self.h)
        except Exception:
            pass


def search_batch_masked(index, term_ids, q_off, k, doc_filter, q_filter):
    """vbm25_search_batch_filtered: search_batch where query q returns only documents of bitmap q_filter[q] of `doc_filter`
    (NO_FILTER: every document) -- the exact filtered top-k, no depth limit."""
    term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
    nq = len(q_off) - 1
    q_filter = np.ascontiguousarray(q_filter, dtype=np.uint32).reshape(-1)
    if len(q_filter) != nq:
        raise ValueError(f"{len(q_filter)} selectors for {nq} queries")
    hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
    n_hits = np.zeros(nq, dtype=np.uint32)
    check(lib().vbm25_search_batch_filtered(index.h, doc_filter.h if doc_filter is not None else None, _p(q_filter), _p(term_ids),
                                            q_off.ctypes.data_as(C.c_void_p), nq, k, hits.ctypes.data_as(C.c_void_p),
                                            n_hits.ctypes.data_as(C.c_void_p)))
    return hits, n_hits


class GrowingSegment:
    """vbm25_device_growing: the growing (unsealed) documents of one index, uploaded to HBM (vbm25_growing_upload).  Built from the
    CSR arrays growing_search takes (g_start, g_key, g_tf, g_fieldnorm, g_payload, g_deleted) or from growing_from_pages' dict."""

    def __init__(self, index, g_start, g_key, g_tf, g_fieldnorm, g_payload, g_deleted=None):
        self.index = index
        g_start = np.ascontiguousarray(g_start, dtype=np.uint64)
        g_key = np.ascontiguousarray(g_key, dtype=np.uint8).reshape(-1)
        g_tf = np.ascontiguousarray(g_tf, dtype=np.uint32)
        g_fieldnorm = np.ascontiguousarray(g_fieldnorm, dtype=np.uint8)
        g_payload = np.ascontiguousarray(g_payload, dtype=np.uint16).reshape(-1)
        g_deleted = None if g_deleted is None else np.ascontiguousarray(g_deleted, dtype=np.uint8)
        self.n_docs = len(g_start) - 1
        if len(g_key) != 16 * len(g_tf):
            raise ValueError(f"{len(g_key)} key bytes for {len(g_tf)} elements")
        d = GrowingDesc()
        d.n_docs, d.n_elements = self.n_docs, len(g_tf)
        d.start, d.key, d.tf = _p(g_start), _p(g_key), _p(g_tf)
        d.fieldnorm, d.payload, d.deleted = _p(g_fieldnorm), _p(g_payload), _p(g_deleted)
        self.h = C.c_void_p()
        check(lib().vbm25_growing_upload(index.h, C.byref(d), C.byref(self.h)))

    @classmethod
    def from_dict(cls, index, grow):
        """from growing_from_pages(pages)"""
        return cls(index, grow["g_start"], grow["g_key"], grow["g_tf"], grow["g_fieldnorm"], grow["g_payload"], grow.get("g_deleted"))

    @classmethod
    def from_pages(cls, index, pages, return_csr=False):
        """vbm25_device_growing_from_pages: the growing segment of a bm25 index relation in the reference's on-disk format, read on
        the device of `index` (the host follows the vectors tape's page chain, kernels parse, validate and flatten the tuples) --
        the segment from_dict(index, growing_from_pages(pages)) makes, without the host touching a tuple.  `pages` as
        DeviceSegment.from_pages takes it.  With return_csr the CSR comes back from the device as well: (segment, the dict of
        growing_from_pages)."""
        cb, keep = _page_reader(pages)
        self = cls.__new__(cls)
        self.index = index
        self.h = C.c_void_p()
        csr = C.c_void_p()
        check(lib().vbm25_device_growing_from_pages(index.h, C.cast(cb, C.c_void_p), None, C.byref(self.h),
                                                    C.byref(csr) if return_csr else None))
        self.n_docs = int(lib().vbm25_device_growing_docs(self.h))
        if not return_csr:
            return self
        try:
            return self, _growing_dict(csr)
        finally:
            lib().vbm25_growing_free(csr)

    def append(self, g_start, g_key, g_tf, g_fieldnorm, g_payload, g_deleted=None):
        """vbm25_device_growing_append: the CSR of the new documents only (the constructor's form); document i becomes growing
        document n_docs + i.  Only these arrays cross the host link; a batch that holds the segment sees them at its next run."""
        g_start = np.ascontiguousarray(g_start, dtype=np.uint64)
        g_key = np.ascontiguousarray(g_key, dtype=np.uint8).reshape(-1)
        g_tf = np.ascontiguousarray(g_tf, dtype=np.uint32)
        g_fieldnorm = np.ascontiguousarray(g_fieldnorm, dtype=np.uint8)
        g_payload = np.ascontiguousarray(g_payload, dtype=np.uint16).reshape(-1)
        g_deleted = None if g_deleted is None else np.ascontiguousarray(g_deleted, dtype=np.uint8)
        if len(g_key) != 16 * len(g_tf):
            raise ValueError(f"{len(g_key)} key bytes for {len(g_tf)} elements")
        d = GrowingDesc()
        d.n_docs, d.n_elements = max(len(g_start) - 1, 0), len(g_tf)
        d.start, d.key, d.tf = _p(g_start), _p(g_key), _p(g_tf)
        d.fieldnorm, d.payload, d.deleted = _p(g_fieldnorm), _p(g_payload), _p(g_deleted)
        try:
            check(lib().vbm25_device_growing_append(self.h, C.byref(d)))
        finally:
            self.n_docs = int(lib().vbm25_device_growing_docs(self.h))

    def append_documents(self, documents):
        """vbm25_device_growing_append_documents: append() with the delta taken from cast Documents in HBM on the segment's device;
        nothing of it crosses the host link."""
        try:
            check(lib().vbm25_device_growing_append_documents(self.h, documents.h))
        finally:
            self.n_docs = int(lib().vbm25_device_growing_docs(self.h))

    def delete(self, indices):
        """vbm25_device_growing_delete: growing documents (indices below n_docs, any order) score nothing from now on."""
        g = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        check(lib().vbm25_device_growing_delete(self.h, _p(g), len(g)))

    def delete_tids(self, tid_set):
        """vbm25_device_growing_delete_tids: delete() of every growing document whose payload is in `tid_set`, found on the device.
        Returns the documents matched (those already deleted included)."""
        n = C.c_uint32()
        check(lib().vbm25_device_growing_delete_tids(self.h, tid_set.h, C.byref(n)))
        return n.value

    @property
    def device_bytes(self):
        return int(lib().vbm25_device_growing_bytes(self.h))

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_device_growing_free(self.h)
        except Exception:
            pass


class DeviceVacuum:
    """vbm25_device_vacuum: a relation's compaction inputs in HBM on the index's device -- the sealed documents' deleted flags as
    words and the growing segment's CSR, read from the page images by kernels (from_pages).  DeviceSegment.maintain_device and
    DocFilter.remap_device consume it in place.  n_sealed / n_sealed_deleted / n_grow / n_grow_deleted / n_elements: the counts."""

    def __init__(self, index, handle):
        self.index, self.h = index, handle
        ns, nsd, ng, ngd, ne = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(lib().vbm25_device_vacuum_info(self.h, C.byref(ns), C.byref(nsd), C.byref(ng), C.byref(ngd), C.byref(ne)))
        self.n_sealed, self.n_sealed_deleted, self.n_grow, self.n_grow_deleted = ns.value, nsd.value, ng.value, ngd.value
        self.n_elements = ne.value

    @classmethod
    def from_pages(cls, index, pages):
        """vbm25_device_vacuum_from_pages: `index` is the GpuIndex of the relation's sealed segment, `pages` as
        DeviceSegment.from_pages takes it.  The host follows the documents tape and the vectors tape; no tuple is touched on it."""
        cb, keep = _page_reader(pages)
        h = C.c_void_p()
        check(lib().vbm25_device_vacuum_from_pages(index.h, C.cast(cb, C.c_void_p), None, C.byref(h)))
        return cls(index, h)

    def read(self):
        """vbm25_device_vacuum_read: (the sealed deleted words, uint64 x ceil(n_sealed / 64); the growing deleted flags, uint8 x n_grow)"""
        n_words = (self.n_sealed + 63) // 64
        words = np.zeros(max(1, n_words), dtype=np.uint64)   # (never a NULL pointer, also for zero words)
        g_del = np.zeros(max(1, self.n_grow), dtype=np.uint8)
        check(lib().vbm25_device_vacuum_read(self.h, words.ctypes.data_as(C.c_void_p), g_del.ctypes.data_as(C.c_void_p)))
        return words[:n_words], g_del[:self.n_grow]

    def bulkdelete(self, index, tid_set):
        """vbm25_device_vacuum_bulkdelete: bulkdelete.rs on the handle -- every sealed document of `index` (the GpuIndex the handle
        was read for) and every growing document whose payload is in `tid_set` is flagged deleted.  Returns (sealed, growing): the
        documents that were live before and are deleted now; the counts of this object follow."""
        ns, ng = C.c_uint32(), C.c_uint32()
        check(lib().vbm25_device_vacuum_bulkdelete(self.h, index.h, tid_set.h, C.byref(ns), C.byref(ng)))
        nsd, ngd = C.c_uint32(), C.c_uint32()
        check(lib().vbm25_device_vacuum_info(self.h, None, C.byref(nsd), None, C.byref(ngd), None))
        self.n_sealed_deleted, self.n_grow_deleted = nsd.value, ngd.value
        return ns.value, ng.value

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_device_vacuum_free(self.h)
        except Exception:
            pass


class TidSet:
    """vbm25_tid_set: a set of ctids in the HBM of one device -- VACUUM's dead TIDs, the TID bitmap of a heap scan.  `tids`: [n, 3]
    uint16 payloads ([bi_hi, bi_lo, ip_posid]) in any order, repeats allowed; n_unique: the distinct ones.  match() / match_growing()
    answer, for every document, whether its payload is in the set, as the words DocFilter.pack makes; DocFilter.set_tids,
    GrowingSegment.delete_tids and DeviceVacuum.bulkdelete consume the set on the device.  Only ever read after it is made.  Also a
    context manager."""

    def __init__(self, tids, device=0):
        tids = np.ascontiguousarray(tids, dtype=np.uint16).reshape(-1, 3)
        self.h = C.c_void_p()
        check(lib().vbm25_tid_set_create(device, _p(tids) if len(tids) else None, len(tids), C.byref(self.h)))
        n, dev = C.c_uint64(), C.c_int()
        check(lib().vbm25_tid_set_info(self.h, C.byref(n), C.byref(dev)))
        self.n_unique, self.device = n.value, dev.value

    @staticmethod
    def keys(tids):
        """the packed 48-bit keys of payloads [n, 3]: ascending keys are ascending ctids"""
        t = np.asarray(tids, dtype=np.uint16).reshape(-1, 3).astype(np.uint64)
        return t[:, 0] << np.uint64(32) | t[:, 1] << np.uint64(16) | t[:, 2]

    def _match(self, fn, handle, n):
        n_words = (n + 63) // 64
        words = np.zeros(max(1, n_words), dtype=np.uint64)  # (never a NULL pointer, also for zero words)
        n_match = C.c_uint32()
        check(fn(self.h, handle, words.ctypes.data_as(C.c_void_p), C.byref(n_match)))
        return words[:n_words], n_match.value

    def match(self, index):
        """vbm25_tid_set_match_index -> (uint64 words [ceil(n_docs / 64)], the documents matched): bit d = sealed document d's payload
        is in the set"""
        return self._match(lib().vbm25_tid_set_match_index, index.h, index.n_docs)

    def match_growing(self, growing):
        """vbm25_tid_set_match_growing: the same over a GrowingSegment's documents, deleted ones included"""
        return self._match(lib().vbm25_tid_set_match_growing, growing.h, growing.n_docs)

    def read(self):
        """vbm25_tid_set_read: the distinct TIDs, [n_unique, 3] uint16, ascending"""
        out = np.zeros((max(1, self.n_unique), 3), dtype=np.uint16)
        check(lib().vbm25_tid_set_read(self.h, out.ctypes.data_as(C.c_void_p)))
        return out[:self.n_unique]

    def device_bytes(self):
        return int(lib().vbm25_tid_set_device_bytes(self.h))

    def close(self):
        if self.h:
            lib().vbm25_tid_set_free(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def search_batch_growing(index, growing, term_ids, q_off, k):
    """vbm25_search_batch_growing: search_batch with the growing segment's documents merged in (sealed first on equal scores)."""
    term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
    nq = len(q_off) - 1
    hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
    n_hits = np.zeros(nq, dtype=np.uint32)
    check(lib().vbm25_search_batch_growing(index.h, growing.h if growing is not None else None, _p(term_ids),
                                           q_off.ctypes.data_as(C.c_void_p), nq, k, hits.ctypes.data_as(C.c_void_p),
                                           n_hits.ctypes.data_as(C.c_void_p)))
    return hits, n_hits


def search_batch_growing_masked(index, growing, term_ids, q_off, k, doc_filter, q_filter):
    """vbm25_search_batch_growing_filtered: search_batch_growing where query q takes bitmap q_filter[q] of `doc_filter` on both
    segments (its sealed bitmap and its growing bitmap of `growing`, DocFilter.set_growing; NO_FILTER: every document)."""
    term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
    nq = len(q_off) - 1
    q_filter = np.ascontiguousarray(q_filter, dtype=np.uint32).reshape(-1)
    if len(q_filter) != nq:
        raise ValueError(f"{len(q_filter)} selectors for {nq} queries")
    hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
    n_hits = np.zeros(nq, dtype=np.uint32)
    check(lib().vbm25_search_batch_growing_filtered(index.h, growing.h if growing is not None else None,
                                                    doc_filter.h if doc_filter is not None else None, _p(q_filter), _p(term_ids),
                                                    q_off.ctypes.data_as(C.c_void_p), nq, k, hits.ctypes.data_as(C.c_void_p),
                                                    n_hits.ctypes.data_as(C.c_void_p)))
    return hits, n_hits


def search_batch_filtered(index, term_ids, q_off, k, keep, overfetch=2, return_truncated=False):
    """`prefilter = on` (default.rs:120-128, fetcher.rs:180-216: a candidate enters Results only if filter(payload) holds -- a heap
    visibility check the GPU cannot make) as the shim runs it: OVER-FETCH and filter on the host.  The GPU returns overfetch * k
    hits per query; the host keeps those `keep(hits) -> bool array` accepts; a query left with fewer than k accepted hits although
    the GPU delivered a full list is asked again, four times deeper, until k survive or its matches are exhausted (bm25.limit's
    maximum, 65535, bounds the depth as it bounds the reference's k).  Exact: the accepted hits are the first k accepted of the
    unfiltered ranking, which is what the reference's filtered search returns (ties aside).  Returns (hits[nq, k], n_hits[nq],
    rounds); with `return_truncated=True` a fourth value: per query, True when the depth reached bm25.limit's maximum with fewer than
    k accepted hits although the GPU's list was full -- the answer may then miss accepted documents beyond rank 65535 (the
    reference's k is bounded the same way)."""
    term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
    nq = len(q_off) - 1
    out = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
    n_out = np.zeros(nq, dtype=np.uint32)
    truncated = np.zeros(nq, dtype=bool)
    todo = np.arange(nq)
    depth = min(65535, max(k, int(k * overfetch)))
    rounds = 0
    while len(todo):
        rounds += 1
        sub_terms = np.concatenate([term_ids[q_off[q]:q_off[q + 1]] for q in todo]) if len(todo) else term_ids[:0]
        sub_off = np.concatenate([[0], np.cumsum([q_off[q + 1] - q_off[q] for q in todo])]).astype(np.uint32)
        hits, n_hits = search_batch(index, sub_terms, sub_off, depth)
        again = []
        for i, q in enumerate(todo):
            h = hits[i, :n_hits[i]]
            ok = h[np.asarray(keep(h), dtype=bool)]
            if len(ok) >= k or n_hits[i] < depth or depth == 65535:  # enough, or the query has no more matches to offer
                n_out[q] = min(k, len(ok))
                out[q, :n_out[q]] = ok[:k]
                truncated[q] = len(ok) < k and n_hits[i] == depth and depth == 65535
            else:
                again.append(q)
        todo = np.array(again, dtype=np.int64)
        depth = min(65535, depth * 4)
    if return_truncated:
        return out, n_out, rounds, truncated
    return out, n_out, rounds


class MultiIndex:
    """vbm25_multi_create: the sealed segment on several GPUs of one node -- uploaded once, replicated GPU to GPU.
    `devices` may list a device more than once (two replicas on device 0: the single-GPU test of the N-GPU path)."""

    def __init__(self, segment, devices):
        self.segment = segment
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        self.h = C.c_void_p()
        check(lib().vbm25_multi_create(C.byref(segment.desc), devs, len(devices), C.byref(self.h)))
        self.n_devices = lib().vbm25_multi_device_count(self.h)

    @classmethod
    def from_device(cls, device_segment, devices):
        """vbm25_multi_create_from_device: the replicas of a DeviceSegment (a compacted one) -- the first made on the segment's
        device, which devices[0] must name, the others copied GPU to GPU; the segment is left as it was."""
        m = cls.__new__(cls)
        m.segment = device_segment  # (n_terms / n_docs for index(); not needed alive by the library)
        m.h = C.c_void_p()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(lib().vbm25_multi_create_from_device(device_segment.h, devs, len(devices), C.byref(m.h)))
        m.n_devices = lib().vbm25_multi_device_count(m.h)
        return m

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_multi_destroy(self.h)
        except Exception:
            pass

    def index(self, i):
        """vbm25_multi_index: replica i as a GpuIndex that does not own its handle (for lookup_terms, and to build that replica's
        DocFilter and GrowingSegment on); it keeps this MultiIndex alive."""
        ix = _ReplicaIndex.__new__(_ReplicaIndex)
        ix.h = C.c_void_p()
        check(lib().vbm25_multi_index(self.h, int(i), C.byref(ix.h)))
        ix.n_terms, ix.n_docs = self.segment.n_terms, self.segment.n_docs
        ix.multi = self
        return ix

    def search_batch(self, term_ids, q_off, k):
        """vbm25_multi_search_batch: as search_batch(), the batch cut into contiguous shards over the replicas."""
        term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
        nq = len(q_off) - 1
        hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
        n_hits = np.zeros(nq, dtype=np.uint32)
        check(lib().vbm25_multi_search_batch(self.h, _p(term_ids), q_off.ctypes.data_as(C.c_void_p), nq, k,
                                             hits.ctypes.data_as(C.c_void_p), n_hits.ctypes.data_as(C.c_void_p)))
        return hits, n_hits


class _ReplicaIndex(GpuIndex):
    """A replica of a MultiIndex (MultiIndex.index): a GpuIndex whose handle belongs to the vbm25_multi."""

    def __del__(self):  # (the handle is borrowed: nothing to destroy)
        pass


class MultiBatch:
    """vbm25_multi_batch_*: the shards resident on their devices; run() is asynchronous on every device's stream
    (scan + download of the records), fetch() waits for all of them."""

    def __init__(self, multi, max_queries, max_total_terms, k):
        self.multi, self.k, self.nq, self.max_queries = multi, k, 0, max_queries
        self.growing = None      # per replica (set_growing / set_filter): kept alive with the batch
        self.doc_filters = None
        self.h = C.c_void_p()
        check(lib().vbm25_multi_batch_create(multi.h, max_queries, max(1, max_total_terms), k, C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_multi_batch_destroy(self.h)
        except Exception:
            pass

    def set_queries(self, term_ids, q_off):
        term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
        try:
            check(lib().vbm25_multi_batch_set_queries(self.h, _p(term_ids), q_off.ctypes.data_as(C.c_void_p), len(q_off) - 1))
        except Vbm25Error:
            self.nq = 0  # (every shard is left with no queries: include/vbm25.h)
            raise
        self.nq = len(q_off) - 1

    def set_growing(self, growing):
        """vbm25_multi_batch_set_growing: one GrowingSegment per replica (built on multi.index(i)), or None to detach."""
        if growing is None:
            check(lib().vbm25_multi_batch_set_growing(self.h, None))
            self.growing = None
            return
        growing = list(growing)
        if len(growing) != self.multi.n_devices:
            raise ValueError(f"{len(growing)} growing segments for {self.multi.n_devices} replicas")
        arr = (C.c_void_p * len(growing))(*[g.h.value if g is not None else None for g in growing])
        check(lib().vbm25_multi_batch_set_growing(self.h, arr))
        self.growing = growing

    def set_filter(self, doc_filters, q_filter=None):
        """vbm25_multi_batch_set_filter: one DocFilter per replica (built on multi.index(i)) and the batch's selectors (query q of
        every later query set takes q_filter[q]; entries beyond the array: NO_FILTER).  None removes the filter."""
        if doc_filters is None:
            check(lib().vbm25_multi_batch_set_filter(self.h, None, None))
            self.doc_filters = None
            return
        doc_filters = list(doc_filters)
        if len(doc_filters) != self.multi.n_devices:
            raise ValueError(f"{len(doc_filters)} filters for {self.multi.n_devices} replicas")
        sel = np.full(self.max_queries, NO_FILTER, dtype=np.uint32)
        if q_filter is not None:
            q_filter = np.asarray(q_filter, dtype=np.uint32).reshape(-1)
            if len(q_filter) > self.max_queries:
                raise ValueError(f"{len(q_filter)} selectors for a batch of {self.max_queries} queries")
            sel[:len(q_filter)] = q_filter
        arr = (C.c_void_p * len(doc_filters))(*[f.h.value for f in doc_filters])
        check(lib().vbm25_multi_batch_set_filter(self.h, arr, _p(sel)))
        self.doc_filters = doc_filters

    def run(self):
        check(lib().vbm25_multi_batch_run(self.h))

    def fetch(self):
        hits = np.zeros((self.nq, self.k), dtype=HIT_DTYPE)
        n_hits = np.zeros(self.nq, dtype=np.uint32)
        check(lib().vbm25_multi_batch_fetch(self.h, _p(hits) if self.nq else None, _p(n_hits) if self.nq else None))
        return hits, n_hits


def set_tuning(name, value):
    """test / tuning aid (vbm25_tuning_set, not in include/vbm25.h): process-wide switch read when a Batch / GpuIndex
    scratch batch is created.  Names: dense_x1000, dense, ne, fused, ne_ratio, dense_items, range_items,
    range_min_chunk, range_grid, dense_grid, fused_items, arith, win, win_force, win_items, win_grid, win_skew, win_guided,
    id16_max_blocks (an index without post_id16: the most 256-byte blocks of a batch's terms that scan_win_kernel's scratch plane
    takes; a larger batch takes scan_range_kernel), win_planes, rel16_plane and id16_plane (read at index creation), cast_wave_max
    and cast_group_max (the class bounds of Documents.cast and Caster.submit, read at the start of each; 0 turns the class off),
    cast_pack (a Caster's wave class: 0 one document a wave, 1 several a wave, 2 several a wave interning in the lanes where the batch
    allows) and cast_grid (the most workgroups of a Caster's kernels, 0 .. 2048, 0 = no cap; both read at each submit), eval_grid (the
    most workgroups of the kernels of Documents.bind, DocTerms.evaluate and a Scorer, 1 .. 2048, read at the start of each call),
    fwd_grid (the most workgroups of GpuIndex.bind's kernels, 0 .. 2048, 0 = no cap), fwd_wave_max and fwd_group_max (the class bounds
    of its per-document sort, up to 64 and 2048, 0 turns the class off; all three read at the start of each bind),
    rerank_part (the candidates one workgroup of Scorer.topk selects from, 64 .. 2^20 in 64s) and rerank_buf (its selection buffer
    as a multiple of k, 2 .. 8; both read at the start of each Scorer call), tid_grid (the most workgroups of the TID match kernel,
    1 .. 2048, read at each launch) and tid_dir (log2 of a TidSet's directory entries, 0 .. 12, read when a TidSet is made).  A
    Reranker reads eval_grid, rerank_part and rerank_buf at each submit, and rerank_part (the size of its part-list scratch) and tid_dir
    (its payload directory) when it is made; Reranker.sync() reads tid_dir again (the directory's new shape) and live_sort_max (the most
    rows of a delta that it sorts in one workgroup's LDS, 0 .. 4096, 0 = always the radix sort).  No switch of
    the product library changes results (`dbg`, the timing experiments of scan_win_kernel, exists only in the development build
    libvbm25_dev.so)."""
    f = lib().vbm25_tuning_set
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_longlong]
    check(f(name.encode(), int(value)))


def reset_tuning():
    f = lib().vbm25_tuning_reset
    f.restype = None
    f.argtypes = []
    f()


def search_batch(index, term_ids, q_off, k):
    """vbm25_search_batch: nq queries (CSR of ascending term ids) -> (hits[nq,k], n_hits[nq])."""
    term_ids = np.ascontiguousarray(term_ids, dtype=np.uint32)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
    nq = len(q_off) - 1
    hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
    n_hits = np.zeros(nq, dtype=np.uint32)
    check(lib().vbm25_search_batch(index.h, _p(term_ids), q_off.ctypes.data_as(C.c_void_p), nq, k,
                                   hits.ctypes.data_as(C.c_void_p),
                                   n_hits.ctypes.data_as(C.c_void_p)))
    return hits, n_hits


def pack_lexemes(queries):
    """A list of queries, each a list of `bytes` lexemes -> the prepacked form (bytes uint8, lex_off uint64, q_lex uint32) that
    Resolver.submit and search_batch_lexemes also take: the lexemes back to back, lexeme i = bytes[lex_off[i]:lex_off[i+1]], query q =
    lexemes q_lex[q] .. q_lex[q+1]."""
    flat = [bytes(t) for q in queries for t in q]
    lex_off = np.zeros(len(flat) + 1, dtype=np.uint64)
    if flat:
        np.cumsum([len(t) for t in flat], out=lex_off[1:])
    q_lex = np.zeros(len(queries) + 1, dtype=np.uint32)
    if len(queries):
        np.cumsum([len(q) for q in queries], out=q_lex[1:])
    return np.frombuffer(b"".join(flat), dtype=np.uint8), lex_off, q_lex


def _packed(queries):
    if isinstance(queries, tuple) and len(queries) == 3:
        data, lex_off, q_lex = queries
        return (np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(lex_off, dtype=np.uint64),
                np.ascontiguousarray(q_lex, dtype=np.uint32))
    return pack_lexemes(queries)


def _seed_arg(seed):
    if seed is not None and len(seed) != 32:
        raise ValueError("the seed is 32 bytes")
    return bytes(seed) if seed is not None else None


def intern_batch(lexemes, seed=None, device=0):
    """vbm25_intern_batch_device: intern (vector.rs:19-35) of a list of `bytes` lexemes on the device -> uint8 [n, 16], byte for byte
    what `intern` gives for each.  `lexemes` may also be the prepacked (bytes, lex_off)."""
    if isinstance(lexemes, tuple):
        data, lex_off = np.ascontiguousarray(lexemes[0], dtype=np.uint8), np.ascontiguousarray(lexemes[1], dtype=np.uint64)
    else:
        data, lex_off, _ = pack_lexemes([lexemes])
    n = len(lex_off) - 1
    keys = np.zeros((n, WIDTH), dtype=np.uint8)
    check(lib().vbm25_intern_batch_device(device, _seed_arg(seed), _p(data), lex_off.ctypes.data, n, _p(keys)))
    return keys


def pack_documents(docs):
    """A list of documents, each a list of (lexeme `bytes`, count) -> the prepacked form (bytes uint8, lex_off uint64, lex_count uint32,
    doc_lex uint32) that Documents.cast also takes: pack_lexemes' packing plus the lexemes' position counts."""
    data, lex_off, doc_lex = pack_lexemes([[t for t, _ in d] for d in docs])
    lex_count = np.array([c for d in docs for _, c in d], dtype=np.uint32)
    return data, lex_off, lex_count, doc_lex


class Documents:
    """vbm25_documents: cast_tsvector_to_document for a batch of tsvectors on the device, the result kept in HBM -- per document the
    distinct keys ascending with their saturating tf sums, the length and its fieldnorm code.  DeviceSegment.from_documents makes an
    index of it, GrowingSegment.append_documents appends it; download() brings the arrays back."""

    def __init__(self, handle, caster=None):
        self._h = handle
        self.caster = caster  # (a collected handle is its caster's: kept alive, never freed from here)
        self._refresh()

    @property
    def h(self):
        """the library's handle; a Documents collected from a Caster loses it when that caster is closed"""
        if self._h is None:
            raise Vbm25Error(-1, "this Documents belonged to a Caster that has been closed: its arrays are freed")
        return self._h

    def _refresh(self):
        nd, ne, dev = C.c_uint32(), C.c_uint64(), C.c_int()
        check(lib().vbm25_documents_info(self.h, C.byref(nd), C.byref(ne), C.byref(dev)))
        self.n_docs, self.n_elements, self.device = nd.value, ne.value, dev.value

    @staticmethod
    def _input(docs_or_packed, payload):
        """-> (bytes, lex_off, lex_count, doc_lex, n_docs, payload) as contiguous arrays of the library's types"""
        if isinstance(docs_or_packed, tuple) and len(docs_or_packed) == 4:
            data, lex_off, lex_count, doc_lex = docs_or_packed
            data, lex_off = np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(lex_off, dtype=np.uint64)
            lex_count, doc_lex = np.ascontiguousarray(lex_count, dtype=np.uint32), np.ascontiguousarray(doc_lex, dtype=np.uint32)
        else:
            data, lex_off, lex_count, doc_lex = pack_documents(docs_or_packed)
        n_docs = len(doc_lex) - 1
        if payload is not None:
            payload = np.ascontiguousarray(payload, dtype=np.uint16).reshape(-1)
            if len(payload) != 3 * n_docs:
                raise ValueError(f"{len(payload)} payload words for {n_docs} documents")
            if not n_docs:
                payload = np.zeros(3, dtype=np.uint16)  # (a non-NULL pointer: the handle is one with payloads)
        return data, lex_off, lex_count, doc_lex, n_docs, payload

    @classmethod
    def cast(cls, docs_or_packed, payload=None, seed=None, device=0):
        """`docs_or_packed`: a list of lists of (lexeme, count), or pack_documents' tuple.  payload: None or uint16 [n_docs, 3]."""
        data, lex_off, lex_count, doc_lex, n_docs, payload = cls._input(docs_or_packed, payload)
        out = C.c_void_p()
        check(lib().vbm25_documents_cast(device, _seed_arg(seed), _p(data), lex_off.ctypes.data, lex_count.ctypes.data, doc_lex.ctypes.data,
                                         n_docs, _p(payload), C.byref(out)))
        return cls(out)

    @classmethod
    def empty(cls, device=0, payload=False):
        """An owned handle of 0 documents, with or without payloads: what extend() grows"""
        return cls.cast([], payload=np.zeros((0, 3), dtype=np.uint16) if payload else None, device=device)

    def extend(self, other):
        """vbm25_documents_extend: `other`'s documents behind this handle's, on the device.  This handle is an owned one (cast,
        empty), `other` any Documents of the same device and payload kind; the result equals one cast of the concatenated input."""
        check(lib().vbm25_documents_extend(self.h, other.h))
        self._refresh()
        return self

    def device_bytes(self):
        return int(lib().vbm25_documents_device_bytes(self.h))

    def download(self, with_length=True):
        """dict: g_start, g_key, g_tf, g_fieldnorm, g_payload (None when the cast had none), g_deleted (all 0) and length"""
        csr = C.c_void_p()
        length = np.zeros(self.n_docs, dtype=np.uint32) if with_length else None
        check(lib().vbm25_documents_download(self.h, C.byref(csr), _p(length)))
        try:
            d = GrowingDesc()
            check(lib().vbm25_growing_get_desc(csr, C.byref(d)))
            out = _growing_dict(csr)
            if not d.payload:
                out["g_payload"] = None
        finally:
            lib().vbm25_growing_free(csr)
        out["length"] = length
        return out

    def bind(self, resolver):
        """vbm25_documents_bind: the documents' keys looked up in the vocabulary `resolver` holds in HBM -> DocTerms, what
        DocTerms.evaluate scores.  Valid for the resolver's index only."""
        out = C.c_void_p()
        check(lib().vbm25_documents_bind(self.h, resolver.h, C.byref(out)))
        return DocTerms(out, resolver.index)

    def __del__(self):
        try:
            if self._h and self.caster is None:
                lib().vbm25_documents_free(self._h)
        except Exception:
            pass


class Caster:
    """vbm25_caster: the Document step as a ring of `depth` slots (1 .. 16) that keep their stream, events, pinned staging, device
    scratch and result arrays between casts: submit() copies a batch in and enqueues it, collect() waits for the oldest batch and
    returns its Documents -- valid until the submit that takes its slot again, `depth` submits after its own.  Capacities a batch:
    max_docs documents, max_lexemes lexemes, max_bytes lexeme bytes, max_long_lexemes lexemes in documents of more than 2048.  One
    thread drives a caster.  Also a context manager."""

    def __init__(self, device, depth, max_docs, max_lexemes, max_bytes, max_long_lexemes=0, seed=None):
        self.h = C.c_void_p()
        check(lib().vbm25_caster_create(device, _seed_arg(seed), depth, max_docs, max_lexemes, max_bytes, max_long_lexemes, C.byref(self.h)))
        self.device, self.depth = device, depth
        self._collected = weakref.WeakSet()  # (the Documents handed out and still alive: close() takes their handles away)

    def submit(self, docs_or_packed, payload=None):
        """vbm25_caster_submit: Documents.cast's input"""
        data, lex_off, lex_count, doc_lex, n_docs, payload = Documents._input(docs_or_packed, payload)
        check(lib().vbm25_caster_submit(self.h, _p(data), lex_off.ctypes.data, lex_count.ctypes.data, doc_lex.ctypes.data, n_docs, _p(payload)))

    def collect(self):
        """The oldest batch in flight as a Documents that keeps this caster alive and never frees the handle"""
        out = C.c_void_p()
        check(lib().vbm25_caster_collect(self.h, C.byref(out)))
        docs = Documents(out, caster=self)
        self._collected.add(docs)
        return docs

    def in_flight(self):
        return int(lib().vbm25_caster_in_flight(self.h))

    def device_bytes(self):
        return int(lib().vbm25_caster_device_bytes(self.h))

    def allocations(self):
        """every allocation and creation the handle has made: it does not move after the constructor"""
        n = C.c_uint64()
        check(lib().vbm25_caster_info(self.h, None, None, C.byref(n)))
        return n.value

    def close(self):
        """vbm25_caster_free.  Every Documents this caster handed out is invalid from here on: using one raises instead of reading
        freed memory."""
        if self.h:
            for docs in list(self._collected):
                docs._h = None
            self._collected.clear()
            lib().vbm25_caster_free(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _at_least_one(a, dtype):
    """contiguous, and never zero-sized: the library refuses NULL pointers, numpy gives an empty array's data no address to rely on"""
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    return a if a.size else np.zeros(1, dtype=dtype)


class DocTerms:
    """vbm25_doc_terms: cast documents bound to one index's vocabulary -- per document the ascending term ids of its known elements
    with their tfs, and its fieldnorm code, in HBM.  evaluate() is the `<&>` operator (bm25::evaluate, evaluate.rs:22-74) for a batch
    of queries, each against its own candidate documents; the SQL operator returns the negation of these values."""

    def __init__(self, handle, index=None):
        self.h = handle
        self.index = index  # (kept alive: the handle refers to it)
        self._refresh()

    def _refresh(self):
        nd, nk, dev = C.c_uint32(), C.c_uint64(), C.c_int()
        check(lib().vbm25_doc_terms_info(self.h, C.byref(nd), C.byref(nk), C.byref(dev)))
        self.n_docs, self.n_known, self.device = nd.value, nk.value, dev.value

    @property
    def base_docs(self):
        """vbm25_doc_terms_base_docs: the documents the handle was bound with (from GpuIndex.bind: the sealed ones)"""
        return int(lib().vbm25_doc_terms_base_docs(self.h))

    def append_documents(self, documents, resolver):
        """vbm25_doc_terms_append_documents: the bind of cast `documents` written behind this handle's, on the device -- document i
        of the delta becomes document n_docs + i; on a handle from GpuIndex.bind, document base_docs + g is growing document g when
        the GrowingSegment is fed the same deltas.  Synchronous; a scorer or a reranker on the handle takes the new documents as
        indices at its next call, a reranker's ctids after Reranker.sync().  Nobody else is inside a call on the handle meanwhile."""
        try:
            check(lib().vbm25_doc_terms_append_documents(self.h, documents.h, resolver.h))
        finally:
            self._refresh()
        return self

    def append(self, g_start, g_key, g_tf, g_fieldnorm, g_payload, resolver, g_deleted=None):
        """vbm25_doc_terms_append: append_documents from the host CSR GrowingSegment.append takes (g_payload None: a delta without
        payloads); a document whose g_deleted is set gets an empty run and keeps its place in the numbering."""
        g_start = np.ascontiguousarray(g_start, dtype=np.uint64)
        g_key = np.ascontiguousarray(g_key, dtype=np.uint8).reshape(-1)
        g_tf = np.ascontiguousarray(g_tf, dtype=np.uint32)
        g_fieldnorm = np.ascontiguousarray(g_fieldnorm, dtype=np.uint8)
        g_payload = None if g_payload is None else _at_least_one(g_payload, np.uint16)
        g_deleted = None if g_deleted is None else np.ascontiguousarray(g_deleted, dtype=np.uint8)
        if len(g_key) != 16 * len(g_tf):
            raise ValueError(f"{len(g_key)} key bytes for {len(g_tf)} elements")
        d = GrowingDesc()
        d.n_docs, d.n_elements = max(len(g_start) - 1, 0), len(g_tf)
        d.start, d.key, d.tf = _p(g_start), _p(g_key), _p(g_tf)
        d.fieldnorm, d.payload, d.deleted = _p(g_fieldnorm), _p(g_payload), _p(g_deleted)
        try:
            check(lib().vbm25_doc_terms_append(self.h, C.byref(d), resolver.h))
        finally:
            self._refresh()
        return self

    def delete(self, docs):
        """vbm25_doc_terms_delete: the documents `docs` (indices into this handle; on a handle from GpuIndex.bind sealed document d
        is d, growing document g is base_docs + g; repeats and dead ones allowed) are dead: Scorer.topk and a Reranker leave them
        out, and a ctid names the lowest live document that carries it.  evaluate() and download() are unchanged.  Synchronous, with
        the append's contract.  -> the documents that were live before the call."""
        docs = np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)
        n_new = C.c_uint32()
        check(lib().vbm25_doc_terms_delete(self.h, _p(docs) if len(docs) else None, len(docs), C.byref(n_new)))
        return n_new.value

    def delete_tids(self, tid_set, documents=None):
        """vbm25_doc_terms_delete_tids: every document whose ctid is in the TidSet is dead.  `documents`: the Documents whose payloads
        name the documents the handle was bound with (what Reranker takes); None on a handle from GpuIndex.bind, whose ctids are the
        index's own.  -> the documents that were live before the call."""
        n_new = C.c_uint32()
        check(lib().vbm25_doc_terms_delete_tids(self.h, tid_set.h, None if documents is None else documents.h, C.byref(n_new)))
        return n_new.value

    @property
    def dead_docs(self):
        """vbm25_doc_terms_dead_docs: the dead documents now"""
        return int(lib().vbm25_doc_terms_dead_docs(self.h))

    def read_dead(self):
        """vbm25_doc_terms_read_dead: the deletion bitmap, uint64 [ceil(n_docs / 64)] -- document d at bit d & 63 of word d >> 6; all
        zero on a handle nobody deleted from"""
        n_words = (self.n_docs + 63) // 64
        words = np.zeros(max(1, n_words), dtype=np.uint64)
        check(lib().vbm25_doc_terms_read_dead(self.h, words.ctypes.data))
        return words[:n_words]

    def device_bytes(self):
        return int(lib().vbm25_doc_terms_device_bytes(self.h))

    def download(self):
        """(start uint64 [n_docs + 1], term uint32 [n_known], tf uint32 [n_known])"""
        start = np.zeros(self.n_docs + 1, dtype=np.uint64)
        term, tf = np.zeros(max(self.n_known, 1), dtype=np.uint32), np.zeros(max(self.n_known, 1), dtype=np.uint32)
        check(lib().vbm25_doc_terms_download(self.h, start.ctypes.data, term.ctypes.data, tf.ctypes.data))
        return start, term[:self.n_known], tf[:self.n_known]

    def evaluate(self, term_ids, q_off, q_cand=None, cand_doc=None):
        """vbm25_evaluate_documents: queries as the CSR (term_ids, q_off) Resolver.collect returns.  Query q scores the documents
        cand_doc[q_cand[q]:q_cand[q+1]] (indices into this handle) -> float64 aligned with cand_doc; without q_cand every query
        scores every document -> float64 [nq, n_docs]."""
        q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
        nq = len(q_off) - 1
        term_ids = _at_least_one(term_ids, np.uint32)
        if q_cand is None:
            if cand_doc is not None:
                raise ValueError("cand_doc without q_cand")
            scores = np.zeros((nq, self.n_docs), dtype=np.float64)
            qc = dc = None
        else:
            q_cand = np.ascontiguousarray(q_cand, dtype=np.uint64)
            if len(q_cand) != nq + 1:
                raise ValueError(f"{len(q_cand)} candidate offsets for {nq} queries")
            scores = np.zeros(int(q_cand[nq]), dtype=np.float64)
            qc = q_cand.ctypes.data
            dc = None if cand_doc is None else _at_least_one(cand_doc, np.uint32)
        out = scores if scores.size else np.zeros(1, dtype=np.float64)
        check(lib().vbm25_evaluate_documents(self.h, term_ids.ctypes.data, q_off.ctypes.data, nq, qc, None if dc is None else dc.ctypes.data,
                                             out.ctypes.data))
        return scores

    def scorer(self):
        """vbm25_scorer_create: a Scorer on this handle -- the rerank step with everything kept between calls"""
        return Scorer(self)

    def reranker(self, resolver, depth, max_queries, max_lexemes, max_bytes, max_candidates, max_k, documents=None, from_index=False):
        """vbm25_reranker_create: a Reranker on this handle -- the rerank step as a pipelined ring, from lexemes and ctids.
        from_index=True (vbm25_reranker_create_from_index, a handle from GpuIndex.bind only): the ctids are the index's own payloads"""
        return Reranker(self, resolver, depth, max_queries, max_lexemes, max_bytes, max_candidates, max_k, documents, from_index)

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_doc_terms_free(self.h)
        except Exception:
            pass


class Scorer:
    """vbm25_scorer: the rerank step on a DocTerms.  It keeps its stream, events, pinned staging and device buffers between calls
    (they grow when a call needs more and are freed by close() only).  evaluate() is DocTerms.evaluate through the handle; topk()
    returns each query's k best candidates, selected on the device.  One call at a time on a scorer (a mutex inside serialises
    them); several scorers on one DocTerms may run at once.  Also a context manager."""

    def __init__(self, doc_terms):
        self.doc_terms = doc_terms  # (kept alive: the handle refers to it)
        self.h = C.c_void_p()
        check(lib().vbm25_scorer_create(doc_terms.h, C.byref(self.h)))

    def device_bytes(self):
        return int(lib().vbm25_scorer_device_bytes(self.h))

    def _inputs(self, term_ids, q_off, q_cand, cand_doc):
        q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
        nq = len(q_off) - 1
        term_ids = _at_least_one(term_ids, np.uint32)
        if q_cand is None:
            if cand_doc is not None:
                raise ValueError("cand_doc without q_cand")
            return term_ids, q_off, nq, None, None
        q_cand = np.ascontiguousarray(q_cand, dtype=np.uint64)
        if len(q_cand) != nq + 1:
            raise ValueError(f"{len(q_cand)} candidate offsets for {nq} queries")
        return term_ids, q_off, nq, q_cand, None if cand_doc is None else _at_least_one(cand_doc, np.uint32)

    def evaluate(self, term_ids, q_off, q_cand=None, cand_doc=None):
        """vbm25_scorer_evaluate: DocTerms.evaluate's arguments, result, refusals and bits"""
        term_ids, q_off, nq, qc, dc = self._inputs(term_ids, q_off, q_cand, cand_doc)
        scores = np.zeros((nq, self.doc_terms.n_docs) if qc is None else int(qc[nq]), dtype=np.float64)
        out = scores if scores.size else np.zeros(1, dtype=np.float64)
        check(lib().vbm25_scorer_evaluate(self.h, term_ids.ctypes.data, q_off.ctypes.data, nq, None if qc is None else qc.ctypes.data,
                                          None if dc is None else dc.ctypes.data, out.ctypes.data))
        return scores

    def topk(self, term_ids, q_off, k, q_cand=None, cand_doc=None):
        """vbm25_scorer_topk -> (ranks [nq, k] of RANK_DTYPE, n_ranks uint32 [nq]).  Row q: the n_ranks[q] = min(k, candidates of q)
        best entries of q's list, score descending then pos (the index within q's list) ascending, zeros behind them -- a stable
        descending sort of evaluate()'s scores cut at k.  Zero scores and repeated documents are entries like any other."""
        term_ids, q_off, nq, qc, dc = self._inputs(term_ids, q_off, q_cand, cand_doc)
        ranks = np.zeros((nq, max(int(k), 0)), dtype=RANK_DTYPE)
        n_ranks = np.zeros(nq, dtype=np.uint32)
        r = ranks if ranks.size else np.zeros(1, dtype=RANK_DTYPE)
        n = n_ranks if nq else np.zeros(1, dtype=np.uint32)
        check(lib().vbm25_scorer_topk(self.h, term_ids.ctypes.data, q_off.ctypes.data, nq, None if qc is None else qc.ctypes.data,
                                      None if dc is None else dc.ctypes.data, int(k), r.ctypes.data, n.ctypes.data))
        return ranks, n_ranks

    def close(self):
        if self.h:
            lib().vbm25_scorer_free(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Reranker:
    """vbm25_reranker: the rerank step as a ring of `depth` slots (1 .. 16) on a DocTerms, with the vocabulary and the seed of
    `resolver`.  submit() takes lexeme queries and candidate lists -- document indices (cand_doc), ctids (cand_tid, uint16 [n, 3];
    needs `documents`, a Documents with payloads of the same documents, or from_index=True on a DocTerms from GpuIndex.bind, at
    construction) or none for the cross product -- and
    returns at once; collect() waits for the oldest batch and returns Scorer.topk's (ranks, n_ranks), byte for byte what
    Resolver.submit / collect followed by Scorer.topk give.  A ctid no document carries is not eligible and keeps its pos; a ctid of
    several documents names the lowest index.  Nothing is allocated after the constructor, except by a sync() that outgrows its room
    to spare.  One thread drives a reranker.  Also a
    context manager."""

    def __init__(self, doc_terms, resolver, depth, max_queries, max_lexemes, max_bytes, max_candidates, max_k, documents=None,
                 from_index=False):
        self.doc_terms, self.resolver = doc_terms, resolver  # (kept alive: the handle refers to both)
        self.h = C.c_void_p()
        if from_index:
            if documents is not None:
                raise ValueError("from_index takes the index's own payloads: documents must be None")
            check(lib().vbm25_reranker_create_from_index(doc_terms.h, resolver.h, depth, max_queries, max_lexemes, max_bytes,
                                                         max_candidates, max_k, C.byref(self.h)))
        else:
            check(lib().vbm25_reranker_create(doc_terms.h, resolver.h, None if documents is None else documents.h, depth, max_queries,
                                              max_lexemes, max_bytes, max_candidates, max_k, C.byref(self.h)))
        self.depth = depth
        self._shapes = []  # per batch in flight: (queries, k)

    @staticmethod
    def _candidates(nq, q_cand, cand_doc, cand_tid):
        """-> the three arrays (None stays None) as contiguous arrays of the library's types; the library refuses the bad pairings"""
        if q_cand is not None:
            q_cand = np.ascontiguousarray(q_cand, dtype=np.uint64)
            if len(q_cand) != nq + 1:
                raise ValueError(f"{len(q_cand)} candidate offsets for {nq} queries")
        return (q_cand, None if cand_doc is None else _at_least_one(cand_doc, np.uint32),
                None if cand_tid is None else _at_least_one(np.ascontiguousarray(cand_tid, dtype=np.uint16).reshape(-1), np.uint16))

    def submit(self, queries_or_packed, k, q_cand=None, cand_doc=None, cand_tid=None):
        """vbm25_reranker_submit_lexemes: Resolver.submit's queries, then Scorer.topk's candidates or ctids"""
        data, lex_off, q_lex = _packed(queries_or_packed)
        nq = len(q_lex) - 1
        qc, dc, tc = self._candidates(nq, q_cand, cand_doc, cand_tid)
        check(lib().vbm25_reranker_submit_lexemes(self.h, _p(data), lex_off.ctypes.data, q_lex.ctypes.data, nq, _p(qc), _p(dc), _p(tc), int(k)))
        self._shapes.append((nq, int(k)))  # (only a batch the library accepted is in the ring)

    def submit_ids(self, term_ids, q_off, k, q_cand=None, cand_doc=None, cand_tid=None):
        """vbm25_reranker_submit_ids: the queries as the CSR (term_ids, q_off) Scorer.topk takes"""
        q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
        nq = len(q_off) - 1
        term_ids = _at_least_one(term_ids, np.uint32)
        qc, dc, tc = self._candidates(nq, q_cand, cand_doc, cand_tid)
        check(lib().vbm25_reranker_submit_ids(self.h, term_ids.ctypes.data, q_off.ctypes.data, nq, _p(qc), _p(dc), _p(tc), int(k)))
        self._shapes.append((nq, int(k)))

    def collect(self):
        """The oldest batch in flight: (ranks [nq, k] of RANK_DTYPE, n_ranks uint32 [nq])"""
        nq, k = self._shapes[0] if self._shapes else (0, 1)  # (an empty ring: the library's own error)
        ranks, n_ranks = np.zeros((nq, k), dtype=RANK_DTYPE), np.zeros(nq, dtype=np.uint32)
        r = ranks if ranks.size else np.zeros(1, dtype=RANK_DTYPE)
        n = n_ranks if nq else np.zeros(1, dtype=np.uint32)
        got_nq, got_k = C.c_uint32(), C.c_uint32()
        check(lib().vbm25_reranker_collect(self.h, r.ctypes.data, n.ctypes.data, C.byref(got_nq), C.byref(got_k)))
        self._shapes.pop(0)
        assert (got_nq.value, got_k.value) == (nq, k)
        return ranks, n_ranks

    def sync(self):
        """vbm25_reranker_sync: the ctid directory brought up to the DocTerms' n_docs after appends, by a merge on the device.
        Batches already submitted resolve their ctids against the old directory, later ones against the new one."""
        check(lib().vbm25_reranker_sync(self.h))

    @property
    def directory_docs(self):
        """vbm25_reranker_directory_docs: the documents the ctid directory covers (the DocTerms' n_docs as of create or the last sync)"""
        return int(lib().vbm25_reranker_directory_docs(self.h))

    def in_flight(self):
        return int(lib().vbm25_reranker_in_flight(self.h))

    def device_bytes(self):
        return int(lib().vbm25_reranker_device_bytes(self.h))

    def allocations(self):
        """every allocation and creation the handle has made: it does not move after the constructor"""
        n = C.c_uint64()
        check(lib().vbm25_reranker_info(self.h, None, None, None, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            lib().vbm25_reranker_free(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Resolver:
    """The Query step on the device (vbm25_resolver_*): lexemes or keys in, per query the ascending term ids out, as the CSR
    (term_ids, q_off) every search entry point takes.  A ring of `depth` slots, first in first out; valid for its index only."""

    def __init__(self, index, depth, max_queries, max_lexemes, max_bytes, seed=None):
        self.index = index
        self.h = C.c_void_p()
        check(lib().vbm25_resolver_create(index.h, _seed_arg(seed), depth, max_queries, max_lexemes, max_bytes, C.byref(self.h)))
        self._n = []  # per batch in flight: (queries, lexemes)

    def __del__(self):
        try:
            if self.h:
                lib().vbm25_resolver_destroy(self.h)
        except Exception:
            pass

    @property
    def device_bytes(self):
        return int(lib().vbm25_resolver_device_bytes(self.h))

    def submit(self, queries):
        """vbm25_resolver_submit_lexemes: `queries` is a list of lists of `bytes`, or the prepacked (bytes, lex_off, q_lex) of
        pack_lexemes for callers that care about the host's time."""
        data, lex_off, q_lex = _packed(queries)
        nq = len(q_lex) - 1
        check(lib().vbm25_resolver_submit_lexemes(self.h, _p(data), lex_off.ctypes.data, q_lex.ctypes.data, nq))
        self._n.append((nq, len(lex_off) - 1))  # (only a batch the library accepted is in the ring)

    def submit_keys(self, keys, q_key):
        """vbm25_resolver_submit_keys: keys = uint8 [n, 16] (or n x 16 bytes), query q = keys q_key[q] .. q_key[q+1]."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
        q_key = np.ascontiguousarray(q_key, dtype=np.uint32)
        nq = len(q_key) - 1
        check(lib().vbm25_resolver_submit_keys(self.h, _p(keys), q_key.ctypes.data, nq))
        self._n.append((nq, len(keys) // WIDTH))

    def collect(self):
        """The oldest batch in flight: (term_ids, q_off)."""
        nq, n_lex = self._n[0] if self._n else (0, 0)  # (an empty ring: the library's own error)
        term_ids, q_off = np.zeros(max(n_lex, 1), dtype=np.uint32), np.zeros(nq + 1, dtype=np.uint32)
        got = C.c_uint32()
        check(lib().vbm25_resolver_collect(self.h, term_ids.ctypes.data, q_off.ctypes.data, C.byref(got)))
        self._n.pop(0)
        assert got.value == nq
        return term_ids[:q_off[nq]], q_off

    @property
    def in_flight(self):
        return int(lib().vbm25_resolver_in_flight(self.h))


def search_batch_lexemes(index, queries, k, seed=None):
    """vbm25_search_batch_lexemes: bm25::search for nq tsvectors' lexemes (list of lists of `bytes`, or prepacked) in one call ->
    (hits[nq,k], n_hits[nq])."""
    data, lex_off, q_lex = _packed(queries)
    nq = len(q_lex) - 1
    hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
    n_hits = np.zeros(nq, dtype=np.uint32)
    check(lib().vbm25_search_batch_lexemes(index.h, _seed_arg(seed), _p(data), lex_off.ctypes.data, q_lex.ctypes.data, nq, k,
                                           hits.ctypes.data, n_hits.ctypes.data))
    return hits, n_hits


def search(index, k, query):
    """bm25::search(&index, k, &query, |_| true) (search.rs:28-36) for one Query:
    best-first list of (score, payload) with the doc id alongside."""
    ids = index.lookup_terms(query.keys)
    ids = np.sort(ids[ids != 0xffffffff])  # unknown tokens are ignored (search.rs:59-61)
    hits, n = search_batch(index, ids, np.array([0, len(ids)], dtype=np.uint32), k)
    return hits[0, :n[0]]


def growing_search(segment_or_desc, query, k, g_start, g_key, g_tf, g_fieldnorm, g_payload, g_deleted=None):
    """Host side of the shim for unsealed documents (search.rs:83-135): `query` is a Query, the
    documents are a CSR over their elements (16-byte keys + term frequencies)."""
    desc = segment_or_desc.desc if isinstance(segment_or_desc, Segment) else segment_or_desc
    keys = np.frombuffer(b"".join(query.keys), dtype=np.uint8) if query.keys else np.zeros(0, np.uint8)
    g_start = np.ascontiguousarray(g_start, dtype=np.uint64)
    g_key = np.ascontiguousarray(g_key, dtype=np.uint8)
    g_tf = np.ascontiguousarray(g_tf, dtype=np.uint32)
    g_fieldnorm = np.ascontiguousarray(g_fieldnorm, dtype=np.uint8)
    g_payload = np.ascontiguousarray(g_payload, dtype=np.uint16)
    g_deleted = None if g_deleted is None else np.ascontiguousarray(g_deleted, dtype=np.uint8)
    hits = np.zeros(max(k, 1), dtype=HIT_DTYPE)
    n = C.c_uint32()
    check(lib().vbm25_growing_search(C.byref(desc), _p(keys), len(query.keys), k, len(g_start) - 1,
                                     _p(g_start), _p(g_key), _p(g_tf), _p(g_fieldnorm), _p(g_payload),
                                     _p(g_deleted), _p(hits), C.byref(n)))
    return hits[:n.value]


def merge_hits(sealed, grow, k):
    """Top-k of the union of two best-first hit lists (the last step of the shim)."""
    sealed = np.ascontiguousarray(sealed, dtype=HIT_DTYPE)
    grow = np.ascontiguousarray(grow, dtype=HIT_DTYPE)
    out = np.zeros(max(k, 1), dtype=HIT_DTYPE)
    n = C.c_uint32()
    check(lib().vbm25_merge_hits(_p(sealed), len(sealed), _p(grow), len(grow), k, _p(out), C.byref(n)))
    return out[:n.value]


READ_PAGE_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_uint32)
WRITE_PAGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p)


class GrowingDesc(C.Structure):
    _fields_ = [("n_docs", C.c_uint32), ("_pad", C.c_uint32), ("n_elements", C.c_uint64),
                ("start", C.c_void_p), ("key", C.c_void_p), ("tf", C.c_void_p),
                ("fieldnorm", C.c_void_p), ("payload", C.c_void_p), ("deleted", C.c_void_p)]


def _page_reader(pages):
    """`pages`: a sequence of 8192-byte page images (bytes / numpy uint8), or a callable
    page_id -> address.  Returns (callback object, keepalive)."""
    if callable(pages):
        cb = READ_PAGE_FN(lambda ctx, i: pages(i))
        return cb, pages
    bufs = [np.frombuffer(bytes(p), dtype=np.uint8) if not isinstance(p, np.ndarray) else p for p in pages]
    for b in bufs:
        if b.size != 8192:
            raise ValueError("a page image is 8192 bytes")
    cb = READ_PAGE_FN(lambda ctx, i: bufs[i].ctypes.data if i < len(bufs) else None)
    return cb, bufs


def segment_from_pages(pages):
    """Flatten a bm25 index relation in the reference's on-disk format (vbm25_segment_from_pages)."""
    cb, keep = _page_reader(pages)
    out = C.c_void_p()
    check(lib().vbm25_segment_from_pages(C.cast(cb, C.c_void_p), None, C.byref(out)))
    return Segment(out)


def pages_fingerprint(pages) -> bytes:
    """vbm25_pages_fingerprint: cache key of the relation's sealed segment (changes on VACUUM / REINDEX)."""
    cb, keep = _page_reader(pages)
    out = (C.c_uint8 * 32)()
    check(lib().vbm25_pages_fingerprint(C.cast(cb, C.c_void_p), None, out))
    return bytes(out)


def pages_seed(pages) -> bytes:
    """MetaTuple.seed of the relation (the key of intern's hash)."""
    cb, keep = _page_reader(pages)
    out = (C.c_uint8 * 32)()
    check(lib().vbm25_pages_seed(C.cast(cb, C.c_void_p), None, out))
    return bytes(out)


def growing_from_pages(pages):
    """The unsealed documents of the relation as the arrays growing_search takes
    (dict: g_start, g_key, g_tf, g_fieldnorm, g_payload, g_deleted; copies)."""
    cb, keep = _page_reader(pages)
    h = C.c_void_p()
    check(lib().vbm25_growing_from_pages(C.cast(cb, C.c_void_p), None, C.byref(h)))
    try:
        return _growing_dict(h)
    finally:
        lib().vbm25_growing_free(h)


def _growing_dict(h):
    """copies of the six arrays of a vbm25_growing"""
    d = GrowingDesc()
    check(lib().vbm25_growing_get_desc(h, C.byref(d)))

    def arr(ptr, n, dt):
        if not n or not ptr:
            return np.zeros(0, dtype=dt)
        buf = (C.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dt).copy()
    return dict(g_start=arr(d.start, d.n_docs + 1, np.uint64), g_key=arr(d.key, 16 * d.n_elements, np.uint8),
                g_tf=arr(d.tf, d.n_elements, np.uint32), g_fieldnorm=arr(d.fieldnorm, d.n_docs, np.uint8),
                g_payload=arr(d.payload, 3 * d.n_docs, np.uint16).reshape(-1, 3),
                g_deleted=arr(d.deleted, d.n_docs, np.uint8))


def sealed_deleted_from_pages(pages):
    """vbm25_sealed_deleted_from_pages: DocumentTuple.deleted of every sealed document of the relation, a bool array of n_docs
    (True = deleted): what DeviceSegment.maintain and DocFilter.remap take as sealed_deleted."""
    cb, keep = _page_reader(pages)
    fn = C.cast(cb, C.c_void_p)
    n_docs = C.c_uint32()
    check(lib().vbm25_sealed_deleted_from_pages(fn, None, None, 0, C.byref(n_docs), None))
    words = np.zeros((n_docs.value + 63) // 64, dtype=np.uint64)
    check(lib().vbm25_sealed_deleted_from_pages(fn, None, _p(words), len(words), C.byref(n_docs), None))
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_docs.value].astype(bool)


def evaluate(segment_or_desc, doc_keys, doc_tfs, query):
    """bm25::evaluate (evaluate.rs:22-74): the `<&>` operator as a plain function; the SQL operator
    returns the negation of this value (operators.rs:54)."""
    desc = segment_or_desc.desc if isinstance(segment_or_desc, Segment) else segment_or_desc
    dk = np.frombuffer(b"".join(doc_keys), dtype=np.uint8) if len(doc_keys) else np.zeros(0, np.uint8)
    dt = np.ascontiguousarray(doc_tfs, dtype=np.uint32)
    qk = np.frombuffer(b"".join(query.keys), dtype=np.uint8) if query.keys else np.zeros(0, np.uint8)
    out = C.c_double()
    check(lib().vbm25_evaluate(C.byref(desc), _p(dk), _p(dt), len(dt), _p(qk), len(query.keys), C.byref(out)))
    return out.value


def evaluate_batch(index, q_terms, doc_start, doc_term, doc_tf):
    """vbm25_evaluate_batch: bm25::evaluate for many documents against one query on the device (term-id space)."""
    q_terms = np.ascontiguousarray(q_terms, dtype=np.uint32)
    doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
    doc_term = np.ascontiguousarray(doc_term, dtype=np.uint32)
    doc_tf = np.ascontiguousarray(doc_tf, dtype=np.uint32)
    out = np.zeros(len(doc_start) - 1, dtype=np.float64)
    check(lib().vbm25_evaluate_batch(index.h, _p(q_terms), len(q_terms), len(doc_start) - 1,
                                     doc_start.ctypes.data_as(C.c_void_p), _p(doc_term), _p(doc_tf), _p(out)))
    return out
