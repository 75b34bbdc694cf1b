"""Hand-made posting lists that reach every codec shape of compression.rs:65-136, shared by tests/test_gpu_codec.py (through every scan
route) and tests/test_gpu_maintain_edges.py / tests/test_maintain_model.py (through the compaction).  A list is (docs ascending, tfs);
build_args turns a set of lists into the arguments of vb.Segment.build after (k1, b)."""
import numpy as np

TAIL_DOCS = (1 << 25) + 5000
WIDTH_DOCS = (1 << 25) + 200_000


def list_keys(n):
    keys = np.zeros((n, 16), dtype=np.uint8)
    for i in range(n):
        s = b"t%03d" % i
        keys[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return keys


def build_args(n_docs, lists, seed=0, payload=False):
    """(doc_len, doc_payload, term_key, term_start, post_doc, post_tf).  The lengths are random, not the sums of the tfs (a flush takes
    whatever lengths it is given).  payload=True: a document's payload is its id (low half, high half, 0), so a relabelled
    document is recognised by its payload; otherwise zeros."""
    rng = np.random.default_rng(seed)
    term_start = np.cumsum([0] + [len(d) for d, _ in lists]).astype(np.uint64)
    post_doc = np.concatenate([np.asarray(d, dtype=np.uint32) for d, _ in lists])
    post_tf = np.concatenate([np.asarray(t, dtype=np.uint32) for _, t in lists])
    # (2^31 documents: drawn as 32-bit values, the 64-bit ones would be another 17 GB)
    doc_len = rng.integers(1, 3000, n_docs, dtype=np.uint32) if n_docs > (1 << 29) else rng.integers(1, 3000, n_docs).astype(np.uint32)
    doc_payload = np.zeros((n_docs, 3), dtype=np.uint16)
    if payload:
        doc_payload[:, :2] = np.arange(n_docs, dtype="<u4").view("<u2").reshape(n_docs, 2)
    return doc_len, doc_payload, list_keys(len(lists)), term_start, post_doc, post_tf


def tail_lists(n_docs=TAIL_DOCS):
    """Byte-packed tails: a: 40 postings with 3-byte deltas and 2-byte tfs; b: 3 postings, raw absolute 4-byte ids and 3-byte tfs; c: a
    full block and a tail of ONE posting; d: two full wide blocks and a 3-byte tail of 80; e: a list that meets all of them"""
    rng = np.random.default_rng(4)
    a_docs = 7 + np.cumsum(rng.integers(1 << 16, 1 << 17, 40))               # tail of 40: gaps >= 2^16 -> 3-byte deltas
    a_tf = rng.integers(1, 60000, 40)
    a_tf[3] = 65535                                                         # 2-byte term frequencies
    b_docs = np.array([5, 5 + (1 << 24) + 3, 5 + (1 << 25) + 9])             # a gap >= 2^24 -> width 4: raw absolute ids
    b_tf = np.array([3, 1 << 17, 70000])                                     # 3-byte term frequencies
    c_docs = np.r_[np.arange(128) * 3 + 1, (1 << 24) + 77]                   # a full block and a tail of ONE posting
    c_tf = np.r_[rng.integers(1, 4, 128), 2]
    d_docs = np.arange(0, n_docs - 1, 100_003)[:336]                         # two full wide blocks (no plane word) + a 3-byte tail of 80
    d_tf = rng.integers(1, 300, len(d_docs))
    e_docs = np.unique(np.r_[a_docs[::2], b_docs, c_docs[::7], d_docs[::5], rng.integers(0, n_docs, 300)])  # meets all of them
    e_tf = rng.integers(1, 5, len(e_docs))
    return [(a_docs, a_tf), (b_docs, b_tf), (c_docs, c_tf), (d_docs, d_tf), (e_docs, e_tf)]


def assert_tail_blocks(a):
    """the blocks tail_lists is there for, in the arrays of the segment built from it"""
    first = a["term_first_block"]
    md, mt, nblk = a["blk_meta_doc"], a["blk_meta_tf"], a["blk_n"]
    assert md[first[0]] == 0x83 and mt[first[0]] == 0x82 and nblk[first[0]] == 40
    assert md[first[1]] == 0x84 and mt[first[1]] == 0x83 and nblk[first[1]] == 3
    assert nblk[first[2] + 1] == 1 and md[first[2]] < 32
    assert md[first[3] + 2] == 0x83 and nblk[first[3] + 2] == 80 and a["blk_max_doc"][first[3]] - a["blk_min_doc"][first[3]] > 65535


def width_lists(seed, n_docs=WIDTH_DOCS):
    """Full blocks of document width w = 1 .. 25 with tf width 1 + (w - 1) % 17 (list w - 1), and a list that meets every one of them a
    few times"""
    rng = np.random.default_rng(seed)
    lists = []
    for w in range(1, 26):  # 128 postings: gaps below 2^w, ONE of them with bit w - 1 set
        gaps = rng.integers(1, min(1 << w, 400) + 1, 128) if w > 1 else np.ones(128, dtype=np.int64)
        gaps = np.minimum(gaps, (1 << w) - 1)
        gaps[0] = 0
        gaps[rng.integers(1, 128)] = rng.integers(1 << (w - 1), 1 << w)
        docs = rng.integers(0, 1000) + np.cumsum(gaps)
        wt = 1 + (w - 1) % 17  # tf field width
        tf = rng.integers(1, 1 << min(wt, 3), 128)
        tf[rng.integers(0, 128)] = rng.integers(1 << (wt - 1), 1 << wt)
        lists.append((docs, tf))
    # a term that meets every list a few times, and a dense one
    mix = np.unique(np.concatenate([d[::9] for d, _ in lists] + [rng.integers(0, n_docs, 500)]))
    lists.append((mix, rng.integers(1, 4, len(mix))))
    return lists


def assert_width_blocks(a, first_list=0):
    first = a["term_first_block"]
    for w in range(1, 26):
        j = first[first_list + w - 1]
        assert a["blk_meta_doc"][j] == w and a["blk_meta_tf"][j] == 1 + (w - 1) % 17, w


def wide_tf_lists(seed, n_docs=WIDTH_DOCS):
    """Full blocks of tf width 18 .. 31 (ONE tf with bit w - 1 set, the others below 8), document gaps below 400 from a random start"""
    rng = np.random.default_rng(seed)
    lists = []
    for w in range(18, 32):
        docs = rng.integers(0, n_docs - 60_000) + np.cumsum(rng.integers(1, 400, 128))
        tf = rng.integers(1, 8, 128)
        tf[rng.integers(0, 128)] = rng.integers(1 << (w - 1), 1 << w)
        lists.append((docs, tf))
    return lists


def wide_tf_tail(n_docs=TAIL_DOCS):
    """A byte-packed tail of 9 postings with 4-byte tfs (one tf >= 2^24) and 3-byte deltas"""
    docs = 1234 + np.arange(9) * 70_001
    tf = np.array([1, 2, (1 << 24) + 5, 7, 65536, 3, (1 << 31) + 1, 255, 256])
    return docs, tf


def low_lists():
    """Lists whose last posting has a low id: a growing posting (id >= the kept sealed documents) behind them makes a gap as wide as
    the index.  20 postings (with one more: a byte-packed tail), 100 postings (filled up to 128: a full block)"""
    return [(40 + np.arange(20) * 13, 1 + np.arange(20) % 4), (3 + np.arange(100) * 7, 1 + np.arange(100) % 3)]


def codec_growing(lists, deleted):
    """Growing documents over the two low lists (the last two keys): the list of 20 gets one posting more, with a 4-byte tf -- a tail
    whose last gap is the whole index (raw absolute ids) --, the list of 100 as many as fill it up to 128 postings -- a full block with
    that gap.  Then a deleted document, and one with a key the sealed segment lacks."""
    keys = list_keys(len(lists))
    ka, kb, k4 = keys[len(lists) - 2], keys[len(lists) - 1], keys[4]
    new = np.frombuffer(b"t0040".ljust(16, b"\0"), np.uint8)  # between t004 and t005
    kept = (lambda d: len(d)) if deleted is None else (lambda d: int((~deleted[d]).sum()))
    assert kept(lists[-2][0]) >= 1
    fill = 128 - kept(lists[-1][0])
    assert fill >= 28
    doc_keys = [[ka, kb]] + [[kb]] * (fill - 1) + [[ka]] + [[k4, new]]
    doc_tfs = [[(1 << 24) + 5, 1]] + [[2]] * (fill - 1) + [[9]] + [[2, 70000]]
    g_del = np.zeros(len(doc_keys), np.uint8)
    g_del[fill] = 1  # (the second document over the list of 20)
    start = np.cumsum([0] + [len(k) for k in doc_keys]).astype(np.uint64)
    rng = np.random.default_rng(2)
    return dict(g_start=start, g_key=np.concatenate([np.stack(k) for k in doc_keys]).reshape(-1),
                g_tf=np.concatenate(doc_tfs).astype(np.uint32), g_fieldnorm=np.zeros(len(doc_keys), np.uint8),
                g_payload=rng.integers(0, 65535, (len(doc_keys), 3)).astype(np.uint16), g_deleted=g_del)
