"""Relations, hand-made vectors tapes and damage for the tests of the device reader of the growing segment
(tests/test_vectors_device_host.py, tests/test_gpu_vectors_device.py).  The relations come from orc.Pages(...).insert, which writes
_2 / _1 / _0 as insert.rs does; the hand-made tapes from pages_device_data._page.  No GPU use."""
import struct
import zlib

import numpy as np

import vectorchord_bm25_amd as vb
import pages_device_data as D

NONE = D.NONE
CHUNK_PAGES, PAGES_PER_PASS = 1024, 2048 * 4   # csrc/pages_parse.h: CHUNK_PAGES; csrc/pages_device.hip: MAX_GRID workgroups of 4 waves


# ---- tuples of the vectors tape (tuples.rs: VectorTuple)

def elements(keys, tfs):
    return b"".join(bytes(k) + struct.pack("<I", int(t)) for k, t in zip(keys, tfs))


def t2(fieldnorm):
    return struct.pack("<QB", 2, fieldnorm) + bytes(7)


def t1(el):
    return struct.pack("<QHH", 1, 16, 16 + len(el)) + bytes(4) + el


def t0(el, payload=(0, 0, 0), deleted=0):
    return struct.pack("<QBxHHHHH", 0, deleted, *payload, 24, 24 + len(el)) + bytes(4) + el


def key_of(i, prefix=b"u"):
    """a 16-byte key that orders by i"""
    return (prefix + b"%09d" % i).ljust(16, b"\0")


def vectors_tape(pl):
    """page ids of the vectors tape in tape order"""
    _, (ptr_jump, joff) = D.tapes(pl)
    p, ids = struct.unpack_from("<I", bytes(pl[ptr_jump]), joff)[0], []
    while p != NONE:
        ids.append(p)
        p = D.next_page(pl[p])
    return ids


def with_vectors_tape(pl, pages_of_tuples):
    """a copy of the page list `pl` whose Jump.ptr_vectors names a new tape appended behind it: one page per entry of
    `pages_of_tuples` (a list of tuples each)"""
    cp = [np.array(p, dtype=np.uint8) for p in pl]
    first = len(cp)
    for i, tuples in enumerate(pages_of_tuples):
        cp.append(D._page(tuples, first + i + 1 if i + 1 < len(pages_of_tuples) else NONE))
    _, (ptr_jump, joff) = D.tapes(cp)
    cp[ptr_jump][joff:joff + 4] = np.frombuffer(struct.pack("<I", first if pages_of_tuples else NONE), np.uint8)
    return cp


# ---- relations

def insert_documents(pages, seg, n, seed, lengths=None, unknown=0.15):
    """n inserted documents of lognormal length: keys of the sealed vocabulary and, with probability `unknown` per document, a few keys
    it lacks, in bytewise ascending order; returns the number inserted"""
    a = seg.arrays()
    n_terms = seg.n_terms
    rng = np.random.default_rng(seed)
    for i in range(n):
        ln = int(lengths[i]) if lengths is not None else int(min(max(rng.lognormal(3.0, 1.0), 0), n_terms))
        ranks = np.sort(rng.choice(n_terms, min(ln, n_terms), replace=False))
        keys = [a["term_key"][r].tobytes() for r in ranks]
        if rng.random() < unknown:
            keys += [key_of(int(x), b"zz") for x in rng.choice(1000, 3, replace=False)]
        keys.sort()
        pages.insert(rng.integers(0, 65535, 3).astype(np.uint16), keys, rng.integers(1, 9, len(keys)).astype(np.uint32))
    return n


_C = {}
TIE_DOCS = (10, 20, 30)   # sealed documents of interleaved_relation() that are inserted again, as growing documents 300, 301, 302


def interleaved_relation():
    """relation() (3000 sealed documents, 500 terms) with 300 inserted documents of lognormal length -- documents that span pages
    (_1 tuples), documents of 0 elements, keys the sealed vocabulary lacks --, copies of the sealed documents TIE_DOCS behind them,
    and a few of the 303 marked deleted.
    Returns (corpus, sealed segment, page list); cached."""
    if "inter" not in _C:
        c, seg, oix, pages = D.relation()
        rng = np.random.default_rng(17)
        lengths = np.minimum(rng.lognormal(3.0, 1.2, 300), 500).astype(int)
        lengths[[3, 50, 299]] = 0
        lengths[[10, 120]] = 480
        insert_documents(pages, seg, 300, seed=18, lengths=lengths)
        # copies of sealed documents: the same terms, tfs and length, hence score ties across the segments
        term, post_doc = np.repeat(np.arange(len(c["term_start"]) - 1), np.diff(c["term_start"].astype(np.int64))), c["post_doc"]
        for d in TIE_DOCS:
            at = np.flatnonzero(post_doc == d)
            pairs = sorted((np.asarray(c["term_key"]).reshape(-1, 16)[term[i]].tobytes(), int(c["post_tf"][i])) for i in at)
            pages.insert(np.array([9, 9, d], np.uint16), [k for k, _ in pairs], [t for _, t in pairs])
        for g in (0, 7, 50, 123, 299):
            pages.mark_deleted_growing(g)
        pl = [p.copy() for p in D.page_list(pages)]
        assert len(vectors_tape(pl)) > 3
        g = vb.growing_from_pages(pl)
        assert g["g_fieldnorm"][300:].tolist() == seg.arrays()["doc_fieldnorm"][list(TIE_DOCS)].tolist()
        _C["inter"] = (c, seg, pl)
    return _C["inter"]


def tie_queries(seg):
    """per document of TIE_DOCS the ids of its three rarest terms: few enough postings that both the document and its growing
    copy are among the first 1500 records (asserted)"""
    c, _, pl = interleaved_relation()
    a = seg.arrays()
    key = a["term_key"].reshape(-1, 16)
    rank = {key[t].tobytes(): t for t in range(len(key))}
    g = vb.growing_from_pages(pl)
    rows = []
    for i in range(len(TIE_DOCS)):
        s, e = int(g["g_start"][300 + i]), int(g["g_start"][301 + i])
        ids = np.array([rank[g["g_key"][16 * j:16 * j + 16].tobytes()] for j in range(s, e)], np.uint32)
        ids = np.sort(ids[np.argsort(a["term_df"][ids], kind="stable")[:3]])
        assert len(ids) == 3 and int(a["term_df"][ids].sum()) < 1200
        rows.append(ids)
    return rows


def big_document_tape():
    """a document of 1000 elements as _2, two _1 and a _0 across three pages (400 + 400 + 200 elements), between two small ones"""
    keys = [key_of(i) for i in range(1000)]
    tfs = [1 + i % 7 for i in range(1000)]
    small = elements([key_of(5), key_of(9)], [2, 3])
    return [[t2(3), t0(small, (1, 2, 3)), t2(40), t1(elements(keys[:380], tfs[:380]))],
            [t1(elements(keys[380:780], tfs[380:780]))],
            [t0(elements(keys[780:], tfs[780:]), (4, 5, 6)), t2(3), t0(small, (7, 8, 9), deleted=1)]]


def hand_tapes():
    """(name, pages of tuples, what the host reader says: "ok" or the refusal's text) on empty_relation()"""
    a, b = elements([key_of(1), key_of(2)], [1, 2]), elements([key_of(3)], [5])
    doc = [t2(7), t0(a, (1, 1, 1))]
    bad_range = struct.pack("<QHH", 1, 16, 26) + bytes(4) + bytes(16)   # _1 with (e - s) = 10
    return [
        ("a document of 1000 elements across three pages", big_document_tape(), "ok"),
        ("documents of 0 elements", [[t2(0), t0(b""), t2(0), t1(b""), t0(b"", (9, 9, 9)), t2(4), t0(a)]], "ok"),
        ("a _2 followed by a _2: a dropped attempt with _1 tuples in it", [doc + [t2(9), t1(a), t1(b)], [t2(8), t1(a), t0(b, (2, 2, 2))] + doc], "ok"),
        ("a trailing _2 without a _0", [doc + doc, [t2(5), t1(a)]], "ok"),
        ("only dropped attempts", [[t2(5), t1(a), t2(6)]], "ok"),
        ("a tape of pages without tuples", [[], [], []], "ok"),
        ("a damaged range inside a dropped attempt", [doc + [t2(9), bad_range, t2(8), t0(a)]], "vector tuple element range"),
        ("a _1 first on the tape", [[t1(a)] + doc], "vector continuation without a start"),
        ("a _0 after a _0", [doc + [t0(b)] + doc], "vector end without a start"),
        ("a _1 after a _0", [doc + [t1(b)] + doc], "vector continuation without a start"),
        ("a _0 of size 16", [[t2(1), struct.pack("<QQ", 0, 0)] + doc], "vector end without a start"),
    ]


def hand_relation(pages_of_tuples, base=None):
    return with_vectors_tape(D.empty_relation() if base is None else base, pages_of_tuples)


def find_tuple(pl, tag, min_elements=1, skip=0):
    """(page id, slot, offset, size) of a tuple of `tag` with at least min_elements elements on the vectors tape, the skip-th such"""
    for p in vectors_tape(pl):
        for i, (off, size) in enumerate(D.slots(pl[p])):
            if struct.unpack_from("<Q", bytes(pl[p]), off)[0] != tag:
                continue
            if tag != 2:
                s, e = struct.unpack_from("<HH", bytes(pl[p]), off + (8 if tag == 1 else 16))
                if (e - s) // 20 < min_elements:
                    continue
            if skip == 0:
                return p, i, off, size
            skip -= 1
    raise AssertionError(f"no tuple of tag {tag}")


def named_damage(pl, skip=0):
    """(name, edit, text of the host reader's refusal): one field of one vector tuple of a relation with inserts (interleaved_relation)
    changes; `skip` moves every case to later tuples"""
    p0, i0, o0, z0 = find_tuple(pl, 0, skip=3 + skip)
    p1, i1, o1, z1 = find_tuple(pl, 1, skip=skip)
    p2, i2, o2, z2 = find_tuple(pl, 2, skip=5 + skip)
    first = vectors_tape(pl)[0]
    f_off = D.slots(pl[first])[0][0]
    return [
        ("line pointer flags", D.set_lp(p0, i0, flags=2), "line pointer is not LP_NORMAL"),
        ("line pointer range", D.set_lp(p1, i1, off=8192 - z1 + 8), "line pointer out of range"),
        ("size 8", D.set_lp(p2, i2, size=8), "vector tuple too short"),
        ("tag 3", D.put("<Q", p0, o0, 3), "vector tuple tag"),
        ("tag 2^32", D.put("<Q", p1, o1, 1 << 32), "vector tuple tag"),
        ("the first _2 of the tape becomes a _1", D.put("<Q", first, f_off, 1), "vector continuation without a start"),
        ("a _2 becomes a _0 of size 16", D.put("<Q", p2, o2, 0), "vector end without a start"),
        ("s > e", D.put("<H", p0, o0 + 16, struct.unpack_from("<H", bytes(pl[p0]), o0 + 18)[0] + 20), "vector tuple element range"),
        ("e > size", D.put("<H", p1, o1 + 10, z1 + 20), "vector tuple element range"),
        ("(e - s) = 10", D.put("<H", p0, o0 + 18, 24 + 10), "vector tuple element range"),
    ]


def unordered_keys(pl, skip=0):
    """edit: two neighbouring keys of a _0 tuple with at least two elements become equal (the reader accepts, the upload refuses)"""
    p, i, off, size = find_tuple(pl, 0, min_elements=2, skip=skip)
    s = struct.unpack_from("<H", bytes(pl[p]), off + 16)[0]

    def edit(cp):
        cp[p][off + s + 20:off + s + 36] = cp[p][off + s:off + s + 16].copy()
    return p, edit


def long_tape(n_pages, seed=1):
    """a vectors tape of n_pages pages made with _page: documents that straddle the page boundaries (_2 and _1 at the end of a page,
    the _0 at the start of the next), every 97th page without tuples, every 50th attempt dropped; returns the pages of tuples"""
    rng = np.random.default_rng(seed)
    out, serial, open_doc = [], 0, False
    for p in range(n_pages):
        tuples = []
        if p % 97 != 96:
            if open_doc:
                n = int(rng.integers(0, 4))
                tuples.append(t0(elements([key_of(serial + j) for j in range(n)], [1 + j for j in range(n)]), (p >> 16, p & 0xffff, 1), deleted=int(p % 11 == 0)))
                serial += n
            n = int(rng.integers(1, 6))
            tuples += [t2(p % 200), t1(elements([key_of(serial + j) for j in range(n)], [2 + j for j in range(n)]))]
            serial += n
            open_doc = True
            if p % 50 == 49:   # the attempt is dropped: the next page starts a new one
                open_doc = False
        out.append(tuples)
    return out


def only_starts_tape():
    """a page of 400 _2 tuples (more than 64 slots for one wave; 399 dropped attempts) and the _0 of the last one behind it"""
    a = elements([key_of(1), key_of(2), key_of(3)], [1, 2, 3])
    return [[t2(i % 256) for i in range(400)], [t1(a[:40]), t0(a[40:], (1, 2, 3))]]


# ---- what the readers say

def host_growing(pl):
    """("ok", dict) | ("corrupt", message) of vbm25_growing_from_pages"""
    try:
        return "ok", vb.growing_from_pages(pl)
    except vb.Vbm25Error as e:
        assert e.code == -2, e
        return "corrupt", str(e)


def first_unordered_document(g):
    """the first document whose keys are not strictly ascending (vbm25_growing_upload's refusal), None: none"""
    key = np.ascontiguousarray(g["g_key"]).reshape(-1, 16)
    if len(key) < 2:
        return None
    a, b = key[:-1], key[1:]
    diff = a != b
    first = np.argmax(diff, axis=1)
    rows = np.arange(len(a))
    less = diff.any(axis=1) & (a[rows, first] < b[rows, first])
    start = g["g_start"].astype(np.int64)
    doc_of = np.searchsorted(start, np.arange(len(key)), side="right") - 1
    bad = np.flatnonzero(~less & (doc_of[1:] == doc_of[:-1]))
    return int(doc_of[bad[0] + 1]) if len(bad) else None


def crcs(g):
    return [zlib.crc32(np.ascontiguousarray(g[name]).tobytes()) for name in ("g_start", "g_key", "g_tf", "g_fieldnorm", "g_payload", "g_deleted")]


def assert_same_csr(got, want, what=""):
    for name in ("g_start", "g_key", "g_tf", "g_fieldnorm", "g_payload", "g_deleted"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: {name} differs"
