"""Relations and damage for the device reader's tests (tests/test_gpu_pages_device.py, tests/test_pages_device_host.py): the small
helpers of tests/test_pages.py (copied: that file stays as it is), the named one-field edits, the seeded random damage of
test_random_damage_never_crashes_the_reader and an empty relation.  No GPU use."""
import struct

import numpy as np

import orc
import vectorchord_bm25_amd as vb
from corpus import make_corpus

NONE = 0xFFFFFFFF


def relation(n_docs=3000, vocab=500, seed=3):
    c = make_corpus(n_docs, vocab, seed=seed, length="lognormal", mean_len=40)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    return c, seg, oix, orc.Pages(oix, seed=bytes(range(32)))


def relation_of(seg):
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    return oix, orc.Pages(oix, seed=bytes(range(32)))


def page_list(pages):
    return [pages.page(i) for i in range(len(pages))]


def slots(page):
    lower = struct.unpack_from("<H", page, 12)[0]
    out = []
    for i in range((lower - 24) // 4):
        iid = struct.unpack_from("<I", page, 24 + 4 * i)[0]
        out.append((iid & 0x7fff, iid >> 17))
    return out


def next_page(page):
    return struct.unpack_from("<I", page, 8192 - 8)[0]


def tapes(pl):
    """page ids of the documents, tokens, summaries and blocks tapes, in tape order; and (jump page, offset of the Jump tuple)"""
    off = slots(pl[0])[0][0]
    ptr_jump = struct.unpack_from("<I", bytes(pl[0]), off + 36)[0]
    joff = slots(pl[ptr_jump])[0][0]
    out = []
    for k in range(4):
        p, ids = struct.unpack_from("<I", bytes(pl[ptr_jump]), joff + 44 + 4 * k)[0], []
        while p != NONE:
            ids.append(p)
            p = next_page(pl[p])
        out.append(ids)
    return out, (ptr_jump, joff)


def terms_of_interest_segment():
    """terms with df exactly 128 (no tail), 129 (a one-posting tail), 1 (a single block of one) and 256 (two full blocks), among a few
    ordinary ones; 700 documents"""
    n_docs = 700
    rng = np.random.default_rng(11)
    dfs = [128, 129, 1, 256, 37, 300, 128, 1]
    post_doc, post_tf, term_start = [], [], [0]
    for df in dfs:
        post_doc.append(np.sort(rng.choice(n_docs, df, replace=False)).astype(np.uint32))
        post_tf.append(rng.integers(1, 6, df).astype(np.uint32))
        term_start.append(term_start[-1] + df)
    post_doc, post_tf = np.concatenate(post_doc), np.concatenate(post_tf)
    doc_len = np.maximum(np.bincount(post_doc, weights=post_tf, minlength=n_docs).astype(np.uint32), 1)
    payload = np.stack([np.arange(n_docs) >> 16, np.arange(n_docs) & 0xffff, np.arange(n_docs) % 64 + 1], axis=1).astype(np.uint16)
    keys = np.zeros((len(dfs), 16), np.uint8)
    for t in range(len(dfs)):
        keys[t, :5] = np.frombuffer(b"t%04d" % t, np.uint8)
    return vb.Segment.build(1.2, 0.75, doc_len, payload, keys, np.array(term_start, np.uint64), post_doc, post_tf)


def _page(tuples, nxt=NONE):
    """one 8 KiB page of the reference's layout holding `tuples` (bytes, 8-aligned sizes), as tests/golden/make_page_fixture.py
    lays pages out: header, line pointers up, tuples down from the special area, Opaque.next in the last 8 bytes"""
    pg = bytearray(8192)
    upper = 8184
    for i, t in enumerate(tuples):
        upper -= (len(t) + 7) & ~7
        pg[upper:upper + len(t)] = t
        struct.pack_into("<I", pg, 24 + 4 * i, upper | 1 << 15 | len(t) << 17)
    struct.pack_into("<HHH", pg, 12, 24 + 4 * len(tuples), upper, 8184)
    struct.pack_into("<I", pg, 8184, nxt)
    return np.frombuffer(bytes(pg), np.uint8).copy()


def empty_relation():
    """an index whose documents are all still in the growing segment: Meta, four empty tapes (one page without tuples each), Jump"""
    meta = b"vchordbm" + struct.pack("<QddII", 1, 1.2, 0.75, NONE, 5) + bytes(range(32))
    jump = struct.pack("<IIQHHIIIIIIIIII", NONE, 0, 0, 2036, 680, 0, NONE, NONE, 0, NONE, NONE, 1, 2, 3, 4) + bytes(4)
    assert len(meta) == 72 and len(jump) == 64
    return [_page([meta]), _page([]), _page([]), _page([]), _page([]), _page([jump])]


def named_damage(pl):
    """(name, edit) pairs: each edit changes one field of a copy of the page list (numpy uint8 pages) in place"""
    (docs, toks, sums, blks), (ptr_jump, joff) = tapes(pl)
    moff = slots(pl[0])[0][0]

    def put(fmt, page, at, value):
        def edit(cp):
            cp[page][at:at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), np.uint8)
        return edit

    def add(page, at, delta, fmt="<B"):
        def edit(cp):
            v = struct.unpack_from(fmt, bytes(cp[page]), at)[0] + delta
            cp[page][at:at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, v), np.uint8)
        return edit

    def set_lp(page, slot, off=None, flags=None, size=None):
        def edit(cp):
            iid = struct.unpack_from("<I", bytes(cp[page]), 24 + 4 * slot)[0]
            o, f, s = iid & 0x7fff, (iid >> 15) & 3, iid >> 17
            o, f, s = (o if off is None else off), (f if flags is None else flags), (s if size is None else size)
            cp[page][24 + 4 * slot:28 + 4 * slot] = np.frombuffer(struct.pack("<I", o | f << 15 | s << 17), np.uint8)
        return edit

    s0 = slots(pl[sums[0]])[0][0]          # first summary
    s_last_full = None
    n_docs = struct.unpack_from("<I", bytes(pl[ptr_jump]), joff + 4)[0]
    # a summary of a full block (n == 128) and the block it points at
    for sp in sums:
        for so, _ in slots(pl[sp]):
            if pl[sp][so + 14] == 128:
                s_last_full = (sp, so)
                break
        if s_last_full:
            break
    fsp, fso = s_last_full
    fb_page, fb_slot = struct.unpack_from("<IH", bytes(pl[fsp]), fso + 8)
    fb_off = slots(pl[fb_page])[fb_slot - 1][0]
    t0, t1 = slots(pl[toks[0]])[0][0], slots(pl[toks[0]])[1][0]
    b0 = slots(pl[blks[0]])[0][0]
    b_lp_off, b_lp_size = slots(pl[blks[0]])[0]
    last_lower = struct.unpack_from("<H", bytes(pl[docs[-1]]), 12)[0]
    return [
        ("bad magic", put("<8s", 0, moff, b"notmagic")),
        ("version 2", put("<Q", 0, moff + 8, 2)),
        ("next of a documents page -> 10^6", put("<I", docs[0], 8184, 10**6)),
        ("pd_lower = 9000", put("<H", docs[0], 12, 9000)),
        ("a page's next pointing at itself", put("<I", toks[0], 8184, toks[0])),
        ("special != 8184", put("<H", sums[0], 16, 8176)),
        ("a summary's block slot + 1", add(sums[0], s0 + 12, 1, "<H")),
        ("a token's summary slot + 1", add(toks[0], t0 + 22, 1, "<H")),
        ("a block-page line pointer with off + len > 8192", set_lp(blks[0], 0, off=8192 - b_lp_size + 8)),
        ("a line pointer with flags != 1", set_lp(docs[0], 3, flags=2)),
        ("a block header with doc_e + 8", add(blks[0], b0 + 4, 8, "<H")),
        ("the last documents page's pd_lower - 4", put("<H", docs[-1], 12, last_lower - 4)),
        ("a token with df = 0", put("<I", toks[0], t0 + 24, 0)),
        ("a summary with max_doc = n_docs", put("<I", sums[0], s0 + 4, n_docs)),
        ("a summary with n = 0", put("<B", sums[0], s0 + 14, 0)),
        ("a summary with n = 129", put("<B", sums[0], s0 + 14, 129)),
        ("a full block with doc metadata 33", put("<B", fb_page, fb_off, 33)),
        ("a token key equal to its predecessor", lambda cp: cp[toks[0]].__setitem__(slice(t1, t1 + 16), cp[toks[0]][t0:t0 + 16].copy())),
        ("Jump n_docs + 1", add(ptr_jump, joff + 4, 1, "<I")),
    ]


def random_damage(n_pages, n_cases, seed=0):
    """the byte flips of tests/test_pages.py::test_random_damage_never_crashes_the_reader (same generator, same draws in the same
    order): per case a list of (page, position, byte)"""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n_cases):
        edits = []
        for _ in range(int(rng.integers(1, 4))):
            pg = int(rng.integers(0, n_pages))
            if rng.random() < 0.5:   # header / line pointers / special area
                pos = int(rng.choice(np.r_[np.arange(12, 60), np.arange(8184, 8192)]))
            else:
                pos = int(rng.integers(0, 8192))
            edits.append((pg, pos, int(rng.integers(0, 256))))
        cases.append(edits)
    return cases


def damage_relation():
    """the relation test_random_damage_never_crashes_the_reader damages: 1500 documents, 120 terms, six inserted documents"""
    c, seg, oix, pages = relation(n_docs=1500, vocab=120, seed=5)
    a = seg.arrays()
    for i in range(6):
        pages.insert(np.array([i, 1, 2], np.uint16), [a["term_key"][r].tobytes() for r in (1, 5, 9)], [1, 2, 3])
    return [p.copy() for p in page_list(pages)]


def apply_edits(pl, edits):
    cp = [p.copy() for p in pl]
    for pg, pos, val in edits:
        cp[pg][pos] = val
    return cp


def host_outcome(pl):
    """(True, Segment) or (False, error code) of the host reader"""
    try:
        return True, vb.segment_from_pages(pl)
    except vb.Vbm25Error as e:
        return False, e.code
