"""Relations, flag patterns and damage of the documents tape for the tests of the device reader of VACUUM's inputs
(tests/test_vacuum_device_host.py, tests/test_gpu_vacuum_device.py).  The relations come from pages_device_data and
vectors_device_data; the yardsticks are the host readers (vbm25_sealed_deleted_from_pages, vbm25_growing_from_pages).  No GPU use."""
import ctypes as C
import struct

import numpy as np

import vectorchord_bm25_amd as vb
import pages_device_data as D
import vectors_device_data as V

FLAG_BYTES = (1, 2, 0x80, 0xFF)          # every one of them is the reference's Bool `true`
SMALL_DOC_COUNTS = (1, 63, 64, 65, 680, 681)   # around a word and around a full documents page (680 tuples)
_C = {}


def doc_slots(pl):
    """(page id, offset of the tuple) of every document in id order, and the documents per page of the tape"""
    (docs, _, _, _), _ = D.tapes(pl)
    where = [(p, off) for p in docs for off, _ in D.slots(pl[p])]
    return where, [len(D.slots(pl[p])) for p in docs]


def flag_patterns(n, per_page, seed=1):
    """name -> uint8[n] of DocumentTuple.deleted bytes (0: kept; the deleted ones cycle through FLAG_BYTES)"""
    rng = np.random.default_rng(seed)
    sets = {"none": [], "all": range(n), "document 0 only": [0], "the last document only": [n - 1],
            "every 64th": range(0, n, 64), "every 63rd": range(0, n, 63), "every 65th": range(0, n, 65),
            "a random half": np.flatnonzero(rng.random(n) < 0.5)}
    around = []
    for b in np.cumsum(per_page)[:-1]:
        around += list(range(max(0, int(b) - 20), min(n, int(b) + 20)))
    sets["the 40 documents around each page boundary"] = sorted(set(around))
    out = {}
    for name, idx in sets.items():
        idx = np.asarray(list(idx), dtype=np.int64)
        flags = np.zeros(n, np.uint8)
        flags[idx] = np.resize(np.array(FLAG_BYTES, np.uint8), len(idx))
        out[name] = flags
    return out


def with_flags(pl, where, flags):
    """a page list that shares every page with `pl` but copies of the documents-tape pages, their deleted bytes set to `flags`"""
    cp = list(pl)
    for p in {p for p, _ in where}:
        cp[p] = pl[p].copy()
    for d in np.flatnonzero(flags):
        cp[where[d][0]][where[d][1]] = flags[d]
    return cp


def packed(flags):
    """the DELETED words of a flag byte array: np.packbits, the bits beyond its length zero"""
    n = len(flags)
    return np.packbits(np.r_[np.asarray(flags) != 0, np.zeros(-n % 64, bool)], bitorder="little").view(np.uint64)


def host_flags(pl):
    """(n_docs, n_deleted, words) of vbm25_sealed_deleted_from_pages through the C ABI, or (code, message) of its refusal"""
    cb, keep = vb.api._page_reader(pl)
    fn = C.cast(cb, C.c_void_p)
    nd, ndel = C.c_uint32(), C.c_uint32()
    rc = vb.lib().vbm25_sealed_deleted_from_pages(fn, None, None, 0, C.byref(nd), C.byref(ndel))
    if rc:
        return rc, f"vbm25 error {rc}: " + vb.lib().vbm25_last_error().decode()
    words = np.zeros(max(1, (nd.value + 63) // 64), np.uint64)
    assert vb.lib().vbm25_sealed_deleted_from_pages(fn, None, words.ctypes.data_as(C.c_void_p), len(words), C.byref(nd), C.byref(ndel)) == 0
    return nd.value, ndel.value, words[:(nd.value + 63) // 64]


def small_relation(n_docs):
    """relation() of n_docs documents over a vocabulary of 40 terms (page list only)"""
    if ("small", n_docs) not in _C:
        c, seg, oix, pages = D.relation(n_docs=n_docs, vocab=40, seed=n_docs)
        _C[("small", n_docs)] = (seg, [p.copy() for p in D.page_list(pages)])
    return _C[("small", n_docs)]


def open_insert_at_the_end(pl):
    """`pl` with one more vectors-tape page behind its last one: a _2 and a _1 of an insert that did not reach its _0"""
    cp = list(pl)
    last = V.vectors_tape(pl)[-1]
    cp[last] = pl[last].copy()
    cp[last][8184:8188] = np.frombuffer(struct.pack("<I", len(cp)), np.uint8)
    cp.append(D._page([V.t2(9), V.t1(V.elements([V.key_of(1), V.key_of(2)], [3, 4]))]))
    return cp


def vacuum_relation():
    """relation() (3000 sealed documents on five documents-tape pages, 500 terms) with 300 inserted documents, 15 % of them with keys
    the sealed vocabulary lacks, none of them deleted (with_growing_deleted), and an unfinished insert at the tape's end.
    Returns (corpus, sealed segment, page list); cached."""
    if "vacuum" not in _C:
        c, seg, oix, pages = D.relation()
        V.insert_documents(pages, seg, 300, seed=31, unknown=0.15)
        pl = open_insert_at_the_end([p.copy() for p in D.page_list(pages)])
        g = vb.growing_from_pages(pl)
        assert len(g["g_start"]) == 301 and g["g_deleted"].sum() == 0 and len(V.vectors_tape(pl)) > 3
        known = set(seg.arrays()["term_key"].reshape(-1, 16).view("S16").reshape(-1).tolist())
        unknown = [k for k in g["g_key"].reshape(-1, 16).view("S16").reshape(-1).tolist() if k not in known]
        assert 20 < len(unknown) < len(g["g_tf"]) // 4
        _C["vacuum"] = (c, seg, pl)
    return _C["vacuum"]


GROWING_DELETED = {"none": (), "some": (0, 5, 63, 64, 128, 299), "all": range(300)}


def with_growing_deleted(pl, which):
    """`pl` with the deleted byte of the _0 tuples of the growing documents `which` set (copies of the pages touched)"""
    which = set(int(g) for g in which)
    cp, g = list(pl), 0
    for p in V.vectors_tape(pl):
        for off, size in D.slots(pl[p]):
            if struct.unpack_from("<Q", bytes(pl[p]), off)[0] == 0:
                if g in which:
                    if cp[p] is pl[p]:
                        cp[p] = pl[p].copy()
                    cp[p][off + 8] = 1
                g += 1
    return cp


def docs_damage(pl):
    """(name, edit) of the documents tape: what vbm25_sealed_deleted_from_pages refuses.  The named cases of pages_device_data that
    touch the documents tape (and Meta / Jump), then line pointers, lengths, the tape's count and its links."""
    (docs, toks, sums, blks), (ptr_jump, joff) = D.tapes(pl)
    named = [(n, e) for n, e in D.named_damage(pl) if n in (
        "bad magic", "version 2", "next of a documents page -> 10^6", "pd_lower = 9000", "a line pointer with flags != 1",
        "the last documents page's pd_lower - 4", "Jump n_docs + 1")]
    assert len(named) == 7
    lp_off, lp_size = D.slots(pl[docs[1]])[7]
    last_lower = struct.unpack_from("<H", bytes(pl[docs[-1]]), 12)[0]
    return named + [
        ("a line pointer not LP_NORMAL on the second page", D.set_lp(docs[1], 7, flags=0)),
        ("a line pointer's offset out of range", D.set_lp(docs[1], 7, off=8192 - lp_size + 8)),
        ("a line pointer's offset inside the header", D.set_lp(docs[0], 0, off=16)),
        ("a tuple of length 7", D.set_lp(docs[2], 70, size=7)),
        ("a tuple of length 7 in the last round of a page", D.set_lp(docs[0], 679, size=7)),
        ("a tape one tuple short of Jump's count", D.put("<H", docs[-1], 12, last_lower - 4)),
        ("a tape one tuple long", D.add(ptr_jump, joff + 4, -1, "<I")),
        ("an unreadable page", D.put("<I", docs[1], 8184, 10**6)),
        ("a page linked twice", D.put("<I", docs[2], 8184, docs[1])),
        ("the special area of the third page", D.put("<H", docs[2], 16, 8176)),
    ]


def docs_damage_pairs(pl):
    """(name, edits): two damages at once; the host reader reports the first in tape order, a page's tuples ahead of its link"""
    (docs, _, _, _), _ = D.tapes(pl)
    return [
        ("line pointers late on the first and early on the last page", [D.set_lp(docs[-1], 1, flags=2), D.set_lp(docs[0], 600, flags=3)]),
        ("a short tuple on page 1 and an unreadable page behind page 2", [D.put("<I", docs[2], 8184, 10**6), D.set_lp(docs[1], 9, size=4)]),
        ("a bad line pointer on the page whose special area is damaged", [D.put("<H", docs[2], 16, 8176), D.set_lp(docs[2], 100, flags=2)]),
        ("a bad line pointer behind a page linked twice", [D.put("<I", docs[1], 8184, docs[0]), D.set_lp(docs[3], 5, flags=2)]),
    ]


def apply(pl, edits):
    cp = [p.copy() for p in pl]
    for e in edits:
        e(cp)
    return cp
