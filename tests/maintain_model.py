"""A numpy restatement of VACUUM's compaction (crates/bm25/src/maintain.rs:27-298 of the reference), independent of the device code:
the sealed blocks decoded (test_segment_builder.decode_all, through the oracle's codec), deleted documents dropped and the others
relabelled in id order, every kept posting one mapping that adds 1 to its document's length (maintain.rs:344-362), the live growing
documents appended with Document::length() (vector.rs:77-83), the mappings sorted by (key, document).  maintain() returns the
arguments of vb.Segment.build and the expected relabel array of vbm25_index_maintain."""
import numpy as np

from test_segment_builder import decode_all

NONE = 0xFFFFFFFF


def key_halves(keys):
    """16-byte keys -> (high, low) big-endian u64: memcmp order is the order of the pairs"""
    k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 16)
    return k[:, :8].copy().view(">u8").ravel().astype(np.uint64), k[:, 8:].copy().view(">u8").ravel().astype(np.uint64)


def _bitpacked(words, b):
    """The 128 b-bit fields of bit-packed bodies (crates/simd/src/bitpacking.rs:58-98: field i is in lane stream i % 4 at bit
    (i / 4) b; stream l's word w is 32-bit word 4 w + l).  words: [blocks, 4 b] uint32 -> [blocks, 128] int64"""
    if b == 0:
        return np.zeros((len(words), 128), np.int64)
    if b == 32:
        return words.astype(np.int64)
    i = np.arange(128)
    bit = (i >> 2) * b
    lo_at = 4 * (bit >> 5) + (i & 3)
    hi_at = np.minimum(lo_at + 4, 4 * b - 1)
    both = (words[:, hi_at].astype(np.uint64) << np.uint64(32)) | words[:, lo_at].astype(np.uint64)
    both = np.where((bit & 31) + b > 32, both, both & np.uint64(0xFFFFFFFF))
    return ((both >> (bit & 31).astype(np.uint64)) & np.uint64((1 << b) - 1)).astype(np.int64)


def decode_all_np(arrays, chunk=1 << 19):
    """decode_all without a Python loop over blocks: every block of a width decoded at once with numpy (the host route's CPU
    decode of tools/maintain_cost.py).  Returns (post_doc, post_tf, term_start) as decode_all."""
    n_blocks = len(arrays["blk_n"])
    blob = np.asarray(arrays["blob"], np.uint8)
    n = arrays["blk_n"].astype(np.int64)
    at = np.r_[0, np.cumsum(n)]
    docs, tfs = np.zeros(int(at[-1]), np.uint32), np.zeros(int(at[-1]), np.uint32)
    off = 8 * arrays["blk_off8"][:n_blocks].astype(np.int64)
    md, mt, mn = arrays["blk_meta_doc"].astype(np.int64), arrays["blk_meta_tf"].astype(np.int64), arrays["blk_min_doc"].astype(np.int64)
    full = md < 0x80
    for c0 in range(0, n_blocks, chunk):
        sl = np.arange(c0, min(n_blocks, c0 + chunk))
        f = sl[full[sl]]
        for b in np.unique(md[f]):  # full blocks: doc-id deltas (width 32: absolute), then the tfs at +16 b bytes
            j = f[md[f] == b]
            body = blob[off[j, None] + np.arange(16 * b)].view("<u4").reshape(len(j), 4 * b) if b else np.zeros((len(j), 0), np.uint32)
            v = _bitpacked(body, int(b))
            ids = v if b == 32 else mn[j, None] + np.cumsum(v, axis=1)
            docs[at[j, None] + np.arange(128)] = ids
        for b in np.unique(mt[f]):
            j = f[mt[f] == b]
            body = blob[off[j, None] + 16 * md[j, None] + np.arange(16 * b)].view("<u4").reshape(len(j), 4 * b) if b else np.zeros((len(j), 0), np.uint32)
            tfs[at[j, None] + np.arange(128)] = _bitpacked(body, int(b))
        t = sl[~full[sl]]  # byte-packed tails (compression.rs:53-62): width 4 = absolute ids
        for j in t:
            wd, wt, k = int(md[j] & 127), int(mt[j] & 127), int(n[j])
            raw = blob[off[j]:off[j] + wd * k].reshape(k, wd).astype(np.int64)
            v = (raw << (8 * np.arange(wd))).sum(1)
            docs[at[j]:at[j] + k] = v if wd == 4 else mn[j] + np.cumsum(v)
            o = off[j] + (wd * k + 7) // 8 * 8
            raw = blob[o:o + wt * k].reshape(k, wt).astype(np.int64)
            tfs[at[j]:at[j] + k] = (raw << (8 * np.arange(wt))).sum(1)
    term_start = np.r_[0, np.cumsum(arrays["term_df"].astype(np.int64))].astype(np.uint64)
    return docs, tfs, term_start


def deleted_flags(deleted, n_docs):
    """None, a bool array or packed uint64 words (bit d % 64 of word d / 64 = deleted) -> bool array of n_docs"""
    if deleted is None:
        return np.zeros(n_docs, bool)
    a = np.asarray(deleted)
    if a.dtype == np.bool_:
        return a.copy()
    bits = np.unpackbits(a.astype("<u8").view(np.uint8), bitorder="little").astype(bool)
    return bits[:n_docs]


def maintain(arrays, meta, deleted=None, growing=None):
    """(build_args, relabel): build_args = (k1, b, doc_len, doc_payload, term_key, term_start, post_doc, post_tf)"""
    n = int(meta["n_docs"])
    keys = np.asarray(arrays["term_key"], np.uint8).reshape(-1, 16)
    if len(keys):
        docs, tfs, ts = decode_all(arrays)
    else:
        docs, tfs, ts = np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64)
    kept = ~deleted_flags(deleted, n)
    n_kept = int(kept.sum())
    relabel_s = np.where(kept, np.cumsum(kept) - 1, NONE).astype(np.int64)
    term = np.repeat(np.arange(len(keys)), np.diff(ts.astype(np.int64)))
    live_post = kept[docs] if len(docs) else np.zeros(0, bool)
    s_term, s_doc, s_tf = term[live_post], relabel_s[docs[live_post]], tfs[live_post].astype(np.int64)
    # rule 2: the length of a kept sealed document is its number of postings (saturating_add(1) per posting)
    s_len = np.bincount(s_doc, minlength=n_kept).astype(np.int64)
    payload = np.asarray(arrays["doc_payload"], np.uint16).reshape(-1, 3)[kept]
    m_hi, m_lo = key_halves(keys[s_term]) if len(s_term) else (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    m_doc, m_tf = s_doc, s_tf
    relabel_g = np.zeros(0, np.int64)
    g_len = np.zeros(0, np.int64)
    g_payload = np.zeros((0, 3), np.uint16)
    if growing is not None:
        start = np.asarray(growing["g_start"], np.uint64).astype(np.int64)
        n_grow = len(start) - 1
        g_del = growing.get("g_deleted")
        live = np.ones(n_grow, bool) if g_del is None else ~np.asarray(g_del).astype(bool)
        relabel_g = np.where(live, n_kept + np.cumsum(live) - 1, NONE).astype(np.int64)
        counts = np.diff(start)
        e_doc = np.repeat(np.arange(n_grow), counts)
        e_key = np.asarray(growing["g_key"], np.uint8).reshape(-1, 16)[start[0]:start[-1]]
        e_tf = np.asarray(growing["g_tf"], np.uint32)[start[0]:start[-1]].astype(np.int64)
        e_live = live[e_doc]
        g_len = np.minimum(np.bincount(e_doc[e_live], weights=e_tf[e_live], minlength=n_grow).astype(np.int64), 2 ** 32 - 1)[live]
        g_payload = np.asarray(growing["g_payload"], np.uint16).reshape(-1, 3)[live]
        gh, gl = key_halves(e_key[e_live])
        m_hi, m_lo = np.r_[m_hi, gh], np.r_[m_lo, gl]
        m_doc = np.r_[m_doc, relabel_g[e_doc[e_live]]]
        m_tf = np.r_[m_tf, e_tf[e_live]]
    # rule 4: sort by (key, document); the tokens are the keys that still have a mapping
    order = np.lexsort((m_doc, m_lo, m_hi))
    m_hi, m_lo, m_doc, m_tf = m_hi[order], m_lo[order], m_doc[order], m_tf[order]
    first = np.r_[True, (m_hi[1:] != m_hi[:-1]) | (m_lo[1:] != m_lo[:-1])] if len(m_hi) else np.zeros(0, bool)
    at = np.flatnonzero(first)
    term_key = np.concatenate([m_hi[at].astype(">u8").view(np.uint8).reshape(-1, 8),
                               m_lo[at].astype(">u8").view(np.uint8).reshape(-1, 8)], axis=1) if len(at) else np.zeros((0, 16), np.uint8)
    term_start = np.r_[at, len(m_hi)].astype(np.uint64)
    doc_len = np.r_[s_len, g_len].astype(np.uint32)
    doc_payload = np.concatenate([payload, g_payload]).astype(np.uint16)
    relabel = np.r_[relabel_s, relabel_g].astype(np.uint32)
    return (meta["k1"], meta["b"], doc_len, doc_payload, term_key, term_start, m_doc.astype(np.uint32), m_tf.astype(np.uint32)), relabel


def make_growing_new_keys(term_key, n_grow, seed, mean_elems=8, deleted=0.1, n_each=6):
    """Growing documents over the sealed keys and over keys the sealed segment lacks that sort BEFORE every sealed key, BETWEEN two
    sealed keys and AFTER every sealed key (n_each of each kind).  Elements in ascending key order, tf 1..5; the form make_growing
    returns."""
    rng = np.random.default_rng(seed)
    term_key = np.asarray(term_key, np.uint8).reshape(-1, 16)
    before = np.zeros((n_each, 16), np.uint8)
    before[:, 0] = 0x01
    before[:, 1] = np.arange(n_each) + 1
    after = rng.integers(1, 256, (n_each, 16), dtype=np.uint8)
    after[:, 0] = 0xFE
    between = term_key[rng.choice(len(term_key), min(n_each, len(term_key)), replace=False)].copy()
    for r in between:  # key + one byte 0x01 in its first zero byte: above it, below every longer key it prefixes
        z = np.flatnonzero(r == 0)
        r[z[0] if len(z) else 15] = 0x01 if len(z) else (r[15] ^ 0x01)
    universe = np.concatenate([term_key, before, between, after])
    hi, lo = key_halves(universe)
    _, uniq = np.unique(np.stack([hi, lo], 1), axis=0, return_index=True)
    universe = universe[np.sort(uniq)]
    hi, lo = key_halves(universe)
    order = np.lexsort((lo, hi))
    rank = np.empty(len(universe), np.int64)
    rank[order] = np.arange(len(universe))
    n_new = len(universe) - len(term_key)
    lens = np.maximum(1, rng.poisson(mean_elems, n_grow))
    doc = np.repeat(np.arange(n_grow), lens)
    pick = rng.integers(0, len(universe), len(doc))
    # every new key at least once (in a live document: the first ones are never deleted below)
    pick[:min(n_new, len(pick))] = len(term_key) + np.arange(min(n_new, len(pick)))
    code = np.unique(doc.astype(np.int64) * len(universe) + rank[pick])
    d = code // len(universe)
    u = order[code % len(universe)]
    start = np.zeros(n_grow + 1, np.uint64)
    np.add.at(start, d + 1, 1)
    start = np.cumsum(start).astype(np.uint64)
    g_del = (rng.random(n_grow) < deleted).astype(np.uint8)
    g_del[:max(1, n_new)] = 0
    return dict(g_start=start, g_key=universe[u].reshape(-1), g_tf=rng.integers(1, 6, len(u)).astype(np.uint32),
                g_fieldnorm=rng.integers(0, 200, n_grow).astype(np.uint8),
                g_payload=rng.integers(0, 65535, (n_grow, 3)).astype(np.uint16), g_deleted=g_del)
