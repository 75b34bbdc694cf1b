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


def put(fmt, page, at, value):
    """edit: the field of format `fmt` at byte `at` of page `page` becomes `value`"""
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


def copy_key(page, src, dst):
    """edit: the 16 key bytes of the token tuple at offset `src` of `page` over those of the tuple at `dst`"""
    def edit(cp):
        cp[page][dst:dst + 16] = cp[page][src:src + 16].copy()
    return edit


def named_damage(pl):
    """(name, edit) pairs: each edit changes one field of a copy of the page list (numpy uint8 pages) in place"""
    (docs, toks, sums, blks), (ptr_jump, joff) = tapes(pl)
    moff = slots(pl[0])[0][0]

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
        ("a token key equal to its predecessor", copy_key(toks[0], t0, t1)),
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


# ---- relations past one chunk of 1024 pages and one grid-stride pass (tests/test_gpu_pages_device_scale.py)

def single_posting_relation(n_terms):
    """2000 documents and n_terms terms of one posting each (tf 1..3), keys the big-endian term number: a relation that is long in
    tokens, summaries and blocks and short in everything else.  226 tokens, 291 summaries or 226 one-posting blocks fill a page, so
    540 000 terms give three tapes of more than 1024 pages (one chunk of the device reader) and more than 2048 x 256 tokens (one
    grid-stride pass of its per-token kernels); 1 860 000 terms put the tokens and blocks tapes past 2048 x 4 pages (one pass of its
    per-page kernels).  tests/test_pages_device_host.py asserts these lengths.  Returns (segment, page list)."""
    n_docs = 2000
    rng = np.random.default_rng(n_terms)
    post_doc = rng.integers(0, n_docs, n_terms).astype(np.uint32)
    post_tf = rng.integers(1, 4, n_terms).astype(np.uint32)
    doc_len = np.maximum(np.bincount(post_doc, weights=post_tf, minlength=n_docs).astype(np.uint32), 1)
    payload = np.stack([np.arange(n_docs) >> 16, np.arange(n_docs) & 0xffff, np.arange(n_docs) % 64 + 1], axis=1).astype(np.uint16)
    keys = np.zeros((n_terms, 16), np.uint8)
    keys[:, :8] = np.arange(n_terms, dtype=">u8").view(np.uint8).reshape(-1, 8)
    seg = vb.Segment.build(1.2, 0.75, doc_len, payload, keys, np.arange(n_terms + 1, dtype=np.uint64), post_doc, post_tf)
    oix, pages = relation_of(seg)
    return seg, page_list(pages)


WIDE_TAIL_N = (1, 7, 8, 9, 127)


def wide_relation():
    """Block bodies of every length the copy of the device reader meets, on 2^20 + 5000 documents (a documents tape of more than one
    chunk).  Terms, in key order:
      0..39   full blocks: for every document-id width w = 1..20, 128 postings drawn as tests/test_gpu_codec.py's
              test_every_bit_width_of_full_blocks draws them (gaps below 2^w, one with bit w - 1 set), stored twice: with term
              frequencies of width w (term 2 (w - 1)) and of width w + 11 (term 2 (w - 1) + 1), one drawn tf with the top bit set
      40      a term that meets every one of those lists
      41..100 byte-packed tails: n in WIDE_TAIL_N postings x document byte width 1, 2, 3 (a gap >= 2^8, >= 2^16) x tf byte width
              1..4, term 41 + (12 in + 4 (bd - 1) + (bt - 1)).  A tail of one posting has document width 1 whatever its document.
    Document widths above 20 and the document byte width 4 need a gap of 2^20 / 2^24 and so more than 2^24 documents -- 200 MB of
    document pages: out of reach at test size, tests/test_gpu_codec.py has them on built segments.
    Returns (segment, page list, expectations: [(term, doc metadata or None, tf metadata, postings)])."""
    n_docs = (1 << 20) + 5000
    rng = np.random.default_rng(20)
    lists, expect = [], []
    for w in range(1, 21):
        gaps = rng.integers(1, min(1 << w, 30) + 1, 128) if w > 1 else np.ones(128, dtype=np.int64)
        gaps = np.minimum(gaps, (1 << w) - 1)
        gaps[0] = 0
        gaps[rng.integers(1, 128)] = rng.integers(1 << (w - 1), 1 << w)
        docs = rng.integers(0, 1000) + np.cumsum(gaps)
        for wt in (w, w + 11):
            tf = rng.integers(1, 1 << min(wt, 3), 128)
            tf[rng.integers(0, 128)] = rng.integers(1 << (wt - 1), 1 << wt)
            expect.append((len(lists), w, wt, 128))
            lists.append((docs, tf))
    mix = np.unique(np.concatenate([d[::9] for d, _ in lists[::2]] + [rng.integers(0, n_docs, 500)]))
    lists.append((mix, rng.integers(1, 4, len(mix))))
    for n in WIDE_TAIL_N:
        for bd in (1, 2, 3):
            for bt in (1, 2, 3, 4):
                gaps = rng.integers(1, 200, n)
                if bd > 1:
                    gaps[n // 2] = rng.integers(1 << (8 * (bd - 1)), (1 << (8 * (bd - 1))) + 1000)
                docs = rng.integers(0, 1000) + np.cumsum(gaps)
                tf = rng.integers(1, 200, n)
                tf[rng.integers(0, n)] = rng.integers(1 << (8 * (bt - 1)), 1 << min(8 * bt, 31))
                expect.append((len(lists), None if n == 1 else 0x80 | bd, 0x80 | bt, n))
                lists.append((docs, tf))
    assert all(int(d[-1]) < n_docs for d, _ in lists)
    keys = np.zeros((len(lists), 16), np.uint8)
    for i in range(len(lists)):
        keys[i, :4] = np.frombuffer(b"t%03d" % i, np.uint8)
    term_start = np.cumsum([0] + [len(d) for d, _ in lists]).astype(np.uint64)
    post_doc = np.concatenate([np.asarray(d, np.uint32) for d, _ in lists])
    post_tf = np.concatenate([np.asarray(t, np.uint32) for _, t in lists])
    doc_len = np.random.default_rng(21).integers(1, 3000, n_docs).astype(np.uint32)
    payload = np.zeros((n_docs, 3), np.uint16)
    payload[:, 0], payload[:, 1] = np.arange(n_docs) >> 16, np.arange(n_docs) & 0xffff
    seg = vb.Segment.build(1.2, 0.75, doc_len, payload, keys, term_start, post_doc, post_tf)
    oix, pages = relation_of(seg)
    return seg, page_list(pages), expect


def check_wide_widths(host_seg, expect):
    """the codec metadata wide_relation() was made for, on the host reader's segment: document widths 1..20 and tf widths 1..31 of
    full blocks, document byte widths 1..3 and tf byte widths 1..4 of tails of 1, 7, 8, 9 and 127 postings"""
    a = host_seg.arrays()
    first = a["term_first_block"]
    for t, md, mt, n in expect:
        j = first[t]
        assert first[t + 1] == j + 1 and a["blk_n"][j] == n and a["blk_meta_tf"][j] == mt, (t, md, mt, n)
        assert a["blk_meta_doc"][j] == (0x81 if md is None else md), (t, md, mt, n)   # a tail of one posting: width 1 whatever the id
    full = a["blk_n"] == 128
    assert set(range(1, 21)) <= set(a["blk_meta_doc"][full].tolist()) and set(range(1, 32)) <= set(a["blk_meta_tf"][full].tolist())
    assert set(a["blk_meta_doc"][~full].tolist()) == {0x81, 0x82, 0x83} and set(a["blk_meta_tf"][~full].tolist()) >= {0x81, 0x82, 0x83, 0x84}
    # body lengths that are no multiple of 8 (the copy's partial reads) and bodies of more than 16 units of 8 bytes (its unit loop)
    units = np.diff(a["blk_off8"].astype(np.int64))
    assert units.max() > 16 and units.min() == 2


# ---- damage beyond chunk 0 and the first grid-stride pass, several errors at once, illegal parameters

CHUNK_PAGES, TOKENS_PER_PASS = 1024, 2048 * 256  # csrc/pages_parse.h: CHUNK_PAGES; csrc/pages_device.hip: MAX_GRID x WG_THREADS


def page_tuples(page):
    return (struct.unpack_from("<H", page, 12)[0] - 24) // 4


def tuples_before(pl, tape, index):
    """tuples on the pages of `tape` (page ids in tape order) in front of its page number `index`"""
    return sum(page_tuples(pl[p]) for p in tape[:index])


def damaged(pl, pages, *edits):
    """a page list that shares every page with `pl` but copies of `pages`, with the edits applied to those: a 54 MB relation is not
    copied for one changed field.  Every edit must stay on `pages` (asserted: `pl` is left as it was)."""
    cp = list(pl)
    before = {p: pl[p].copy() for p in pages}
    for p in pages:
        cp[p] = pl[p].copy()
    for edit in edits:
        edit(cp)
    assert all(np.array_equal(pl[p], before[p]) for p in pages) and all(cp[i] is pl[i] for i in range(len(pl)) if i not in before)
    return cp


def byte_edits(pl, cp, pages):
    """the (page, position, byte) list that turns `pl` into `cp` (the case-file form of tests/native/fuzz_pages_device.cpp)"""
    return [(p, int(i), int(cp[p][i])) for p in pages for i in np.flatnonzero(cp[p] != pl[p])]


def chunk_damage(pl):
    """Damage of single_posting_relation(540 000) on pages that lie in the second and third chunk of their tapes, and on tokens beyond
    the first 2048 x 256: (name, what the readers must agree on -- "message" or "code" --, pages edited, edit, (tape, page number in
    the tape, tuple number in the tape) of the damaged tuple)."""
    (docs, toks, sums, blks), _ = tapes(pl)

    def at(tape, index, slot):
        return tape[index], slots(pl[tape[index]])[slot][0], tuples_before(pl, tape, index) + slot

    cases = []
    cases.append(("a line pointer with flags != 1 on tokens page 1500", "message", [toks[1500]], set_lp(toks[1500], 100, flags=2),
                  ("tokens", 1500, tuples_before(pl, toks, 1500) + 100)))
    last = len(blks) - 1
    cases.append(("a line pointer with flags != 1 on the last blocks page", "message", [blks[last]], set_lp(blks[last], 3, flags=0),
                  ("blocks", last, tuples_before(pl, blks, last) + 3)))
    p, o, g = at(blks, 2100, 5)
    cases.append(("a block header with doc_e + 8 on blocks page 2100", "message", [p], add(p, o + 4, 8, "<H"), ("blocks", 2100, g)))
    p, o, g = at(sums, 1100, 7)
    cases.append(("a summary's block slot + 1 on summaries page 1100", "message", [p], add(p, o + 12, 1, "<H"), ("summaries", 1100, g)))
    p, o, g = at(toks, 2350, 10)
    cases.append(("df = 0 of a token beyond the first pass of the per-token kernels", "code", [p], put("<I", p, o + 24, 0), ("tokens", 2350, g)))
    p, o, g = at(toks, 2200, 5)
    o_prev = slots(pl[p])[4][0]
    cases.append(("a token key equal to its predecessor in chunk 2", "code", [p], copy_key(p, o_prev, o), ("tokens", 2200, g)))
    return cases


def paired_damage(pl):
    """Two errors at once on relation() (3000 documents: 5 / 3 / 4 / 23 pages): (name, pages edited, edits, text and page id of the
    one error both readers must report: the first one in walk order, the relation's structure ahead of the flattened arrays)"""
    (docs, toks, sums, blks), (ptr_jump, joff) = tapes(pl)
    n_docs = struct.unpack_from("<I", bytes(pl[ptr_jump]), joff + 4)[0]
    lp = "line pointer is not LP_NORMAL"
    late = lambda tape: page_tuples(pl[tape[0]]) - 2
    s0 = slots(pl[sums[0]])[0][0]
    b_last = slots(pl[blks[-1]])[1][0]
    return [
        ("line pointers late on the first and early on the last documents page", [docs[0], docs[-1]],
         [set_lp(docs[-1], 1, flags=2), set_lp(docs[0], late(docs), flags=2)], lp, docs[0]),
        ("line pointers early on the first and late on the last documents page", [docs[0], docs[-1]],
         [set_lp(docs[-1], page_tuples(pl[docs[-1]]) - 1, flags=3), set_lp(docs[0], 1, flags=0)], lp, docs[0]),
        ("line pointers late on the first and early on the last blocks page", [blks[0], blks[-1]],
         [set_lp(blks[-1], 0, flags=2), set_lp(blks[0], late(blks), flags=2)], lp, blks[0]),
        ("line pointers early on the first and late on the last blocks page", [blks[0], blks[-1]],
         [set_lp(blks[-1], page_tuples(pl[blks[-1]]) - 1, flags=0), set_lp(blks[0], 1, flags=3)], lp, blks[0]),
        ("a line pointer on the last documents page and one on the first blocks page", [docs[-1], blks[0]],
         [set_lp(blks[0], 0, flags=2), set_lp(docs[-1], 2, flags=2)], lp, docs[-1]),
        ("a block header on the last blocks page and max_doc = n_docs in the first summary", [blks[-1], sums[0]],
         [put("<I", sums[0], s0 + 4, n_docs), add(blks[-1], b_last + 4, 8, "<H")],
         "block tuple ranges do not match its codec metadata", blks[-1]),
    ]


def set_params(k1=None, b=None):
    """edit: MetaTuple.k1 / .b (page 0)"""
    def edit(cp):
        moff = slots(cp[0])[0][0]
        if k1 is not None:
            cp[0][moff + 16:moff + 24] = np.frombuffer(struct.pack("<d", k1), np.uint8)
        if b is not None:
            cp[0][moff + 24:moff + 32] = np.frombuffer(struct.pack("<d", b), np.uint8)
    return edit


# the named cases that leave the relation's structure whole: with an illegal k1 or b the readers answer VBM25_ERR_INVALID (the
# parameters are looked at before the flattened arrays), every other named case stays VBM25_ERR_CORRUPT
ARRAY_LEVEL_DAMAGE = ("a summary with max_doc = n_docs", "a summary with n = 0", "a summary with n = 129", "a token key equal to its predecessor")


def host_error(pl):
    """(code, message) of the host reader's refusal"""
    try:
        vb.segment_from_pages(pl)
    except vb.Vbm25Error as e:
        return e.code, str(e)
    raise AssertionError("the host reader accepts the relation")


def write_case_file(path, pl, cases):
    """tests/native/fuzz_pages_device.cpp's case file: the relation and per case its (page, position, byte) edits"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(pl)))
        for p in pl:
            f.write(p.tobytes())
        f.write(struct.pack("<I", len(cases)))
        for edits in cases:
            f.write(struct.pack("<I", len(edits)))
            for e in edits:
                f.write(struct.pack("<III", *e))
