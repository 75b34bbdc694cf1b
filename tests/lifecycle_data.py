"""Corpora, query sets and the oracle's expected records for tests/test_gpu_batch_lifecycle.py: one batch object fed query set after
query set, with filters and growing segments attached and detached between them.  The expected records are the oracle's brute force
for the batch's state of the moment: plain, filtered (the full unfiltered ranking with the rejected documents removed) or with a growing
segment (the host composition vbm25_merge_hits(sealed, vbm25_growing_search(...), k))."""
import numpy as np

import orc
import vectorchord_bm25_amd as vb
from parity import assert_bit_exact

NONE = vb.NO_FILTER


def built(c):
    """a make_corpus() dict as a host Segment"""
    return vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])


def oracle(seg):
    return orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())


def bench_queries(seg, vocab, nq, nterms, seed, zipf_s=0.0):
    from bench import make_queries
    return make_queries(seg, vocab, nq, nterms, seed=seed, zipf_s=zipf_s)


def from_rows(rows):
    """(term ids, q_off) of a list of per-query id arrays"""
    terms = np.concatenate([np.asarray(r, np.uint32) for r in rows]) if rows else np.zeros(0, np.uint32)
    off = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.uint32)
    return terms.astype(np.uint32), off


def rows_of(terms, off):
    return [terms[off[q]:off[q + 1]] for q in range(len(off) - 1)]


def term_df(seg):
    return seg.arrays()["term_df"].astype(np.int64)


def id16_blocks(df, terms, off):
    """the 256-byte blocks a batch's terms take in the scratch plane of an index without post_id16 (block 0 and 1 reserved)"""
    t = terms[terms < len(df)]
    return 2 + int(((df[t] + 127) // 128).sum())


class Expect:
    """the oracle's records of one segment for the states a batch object goes through"""

    def __init__(self, seg, oix=None):
        self.seg = seg
        self.oix = oix if oix is not None else oracle(seg)
        self.n_terms = seg.n_terms
        self._key = None

    def plain(self, terms, off, k):
        return [self.oix.search_brute(t, k) for t in rows_of(terms, off)]

    def filtered(self, terms, off, k, keeps, sel):
        """query q takes bitmap sel[q] of `keeps` (NONE: no bitmap)"""
        out = []
        for q, t in enumerate(rows_of(terms, off)):
            s = int(sel[q]) if q < len(sel) else NONE
            if s == NONE:
                out.append(self.oix.search_brute(t, k))
                continue
            full = self.oix.search_brute(t, 65535)
            assert len(full) < 65535, "the reference ranking would be cut"
            out.append(full[keeps[s][full["doc_id"]]][:k])
        return out

    def growing(self, terms, off, k, G):
        if self._key is None:
            self._key = self.seg.arrays()["term_key"].reshape(-1, 16)
        out = []
        for t in rows_of(terms, off):
            sealed = self.oix.search_brute(t, k)
            t = t[t < self.n_terms]
            grow = vb.growing_search(self.seg, vb.Query([self._key[r].tobytes() for r in t]), k, **G)
            out.append(vb.merge_hits(sealed, grow, k))
        return out


def check(want, hits, nh, what):
    assert len(nh) == len(want), f"{what}: {len(nh)} queries, want {len(want)}"
    for q, w in enumerate(want):
        assert nh[q] == len(w), f"{what} q{q}: {nh[q]} records, want {len(w)}"
        assert_bit_exact(w, hits[q, :nh[q]], what=f"{what} q{q}")


def failing_sets(terms, off, max_q, max_t, n_terms):
    """(name, term ids, q_off, error code) of the query sets set_queries must refuse, made from a valid set (terms, off) of a batch
    of max_q queries and max_t terms over an index of n_terms terms"""
    INVALID, UNSUPPORTED = -1, -4
    nq = len(off) - 1
    assert nq >= 3 and off[-1] - off[-2] >= 2 and off[1] >= 1 and n_terms > 1024
    out = []
    o = off.copy()
    o[0] = 1
    out.append(("q_off[0] != 0", terms, o, INVALID))
    o = off.copy()
    o[2] = o[1] - 1  # (query 0 is valid, query 1 ends before it starts)
    out.append(("q_off not monotone", terms, o, INVALID))
    t = terms.copy()
    a = int(off[-2])
    t[a], t[a + 1] = t[a + 1], t[a]  # (the last query: every query before it was taken apart already)
    out.append(("unsorted ids in the last query", t, off, INVALID))
    extra = max_t - len(terms) + 1  # (unknown ids behind the last query's: valid but for their number)
    base = max(int(terms.max()) + 1, n_terms)
    t = np.r_[terms, base + np.arange(extra)].astype(np.uint32)
    o = off.copy()
    o[-1] += extra
    out.append(("more terms than max_total_terms", t, o, INVALID))
    out.append(("more queries than max_queries", np.zeros(max_q + 1, np.uint32), np.arange(max_q + 2, dtype=np.uint32), INVALID))
    t = np.r_[terms[:a], np.arange(1025)].astype(np.uint32)
    o = off.copy()
    o[-1] = a + 1025
    out.append(("a query of 1025 indexed terms", t, o, UNSUPPORTED))
    return out
