"""A model of one table's rows through INSERT, SELECT, DELETE and VACUUM (the reference's tests/fuzz transposed), for
tests/test_table_model.py and tests/test_gpu_table_fuzz.py.  It knows which rows the table holds and the reference's rules, and
nothing of the library: its only dependencies are numpy and the oracle (tests/orc.py), which flushes the rows (flush.rs), lays the
relation out (build.rs, insert.rs), ranks the sealed rows by brute force and evaluates one BM25 term.  No GPU use.

The rules:
  * a growing row's length is min(sum tf, 2^32 - 1) (vector.rs:77-83);
  * deleted sealed rows stay in the index and in its statistics until the next VACUUM (search.rs:226-229 only skips them);
  * a growing row is scored with the sealed segment's statistics over the query keys both it and the sealed vocabulary hold,
    summed in ascending key order from 0.0, and enters with a score > 0 as doc_id 0xFFFFFFFF - g (search.rs:83-135);
  * order: score descending; on equal scores sealed before growing, sealed by id, growing by g;
  * VACUUM keeps the live sealed rows in order, then the live growing rows in order; a kept sealed row's new length is its number
    of postings (maintain.rs:344-362), a growing row keeps its length; everything is flushed again from scratch;
  * a delete by ctid (bulkdelete.rs) kills every row of both segments that carries one of the ctids;
  * the rerank step scores a candidate with the `<&>` operator (evaluate.rs: idf * tf per shared key, ascending, from 0.0; the
    fieldnorm of the row's stored length), names a ctid's lowest row and knows nothing of deletion (Table.rerank);
  * on the rerank stack that follows the table (one index-bound handle that every insert is appended to, side "live") the rows
    are sealed + growing in that order, so a ctid of a sealed and a growing row names the sealed one, dead or not; the ctid
    directory covers the rows of its last sync (Table.rerank_op syncs when a rerank finds rows pending).
Table.ops_ctid draws the same life in lexemes and ctids for tests/test_gpu_table_ctid_fuzz.py and tests/test_gpu_table_live_fuzz.py."""
import struct

import numpy as np

import orc

NONE = 0xFFFFFFFF
MAX_K = 65535
KS = (1, 10, 100, 300, 1025)
NO_ROW_KEY = b"~no row".ljust(16, b"\0")
INSERT_KEYS = (1, 3, 30, 250)
INSERT_ROWS = (1, 4, 16)
# one row of a rerank result: the score, the position in the query's candidate list, the row index (the library's vbm25_rank)
RANK_DTYPE = np.dtype({"names": ["score", "pos", "doc"], "formats": ["<f8", "<u4", "<u4"], "offsets": [0, 8, 12], "itemsize": 16})
RERANK_KS = (1, 10, 64, 65, 1024)   # 1024: the scorer's maximum
NO_ROW_LEXEME = b"~no row"          # (shorter than 16 bytes: its key is NO_ROW_KEY, vector.rs:21-24)
HITS_K = 100                        # the records a search returns for the rerank of its hits (rerank_op's "hits")
CAST_DOCS = 4                       # the rows of one cast handle of the ctid lives: an INSERT of n rows is ceil(n / 4) appends


def new_key(i):
    """a key no initial row holds (corpus.token_keys are decimal digits)"""
    return (b"n%06d" % i).ljust(16, b"\0")


def random_rows(n_docs, vocab, seed, mean_len=40, keys=None):
    """n_docs rows of lognormal length (mean about mean_len) over `vocab` Zipf(1) tokens (tests/fuzz:168-205 of the reference: a row
    is its length in token draws, tf the multiplicity); token t's key is its decimal digits, zero padded (vector.rs:21-24), or
    keys[t] where `keys` is given (interned lexemes).  Returns (rows, the keys of all `vocab` tokens)."""
    rng = np.random.default_rng(seed)
    keys = [str(t).encode().ljust(16, b"\0") for t in range(vocab)] if keys is None else [bytes(key) for key in keys]
    assert len(keys) == vocab
    lens = np.clip(np.rint(rng.lognormal(np.log(mean_len * 0.8), 0.6, n_docs)), 8, 2000).astype(np.int64)
    p = 1.0 / np.arange(1, vocab + 1)
    rows = []
    for d in range(n_docs):
        tok, cnt = np.unique(rng.choice(vocab, int(lens[d]), p=p / p.sum()), return_counts=True)
        rows.append((((d // 64) >> 16, (d // 64) & 0xffff, d % 64 + 1), {keys[t]: int(c) for t, c in zip(tok, cnt)}, int(lens[d])))
    return rows, keys


def length_of(kt):
    return min(sum(kt.values()), 2 ** 32 - 1)


def _slots(page):
    lower = struct.unpack_from("<H", page, 12)[0]
    return [struct.unpack_from("<I", page, 24 + 4 * i)[0] & 0x7fff for i in range((lower - 24) // 4)]


class Table:
    def __init__(self, rows, k1, b, seed32):
        self.k1, self.b, self.seed = float(k1), float(b), bytes(seed32)
        self.vacuums = []   # per VACUUM: (sealed rows deleted, growing rows deleted, keys the sealed vocabulary lacked)
        self.stats = dict(selects=0, both=0, nothing=0, deleted_shown=0, mixed_ties=0)
        # what the ctid life counts (delete_tids with `what`, rerank_op); assert_coverage_ctid of tests/test_table_model.py reads it
        self.cstats = dict(bulk_full=0, delete_batches=0, reranks=0, rerank_both=0, ineligible_sealed=0, ineligible_growing=0,
                           rerank_short=0, rerank_cut=0)
        # what the live side counts (live_append, rerank_op); assert_coverage_live reads it
        self.cstats.update(live_both=0, live_shared=0, sync_multi=0, sync_one=0, ab_differ=0, unknown_handle=0, live_short=0, live_cut=0,
                           live_hits=0)
        self._n_batches = 0
        self._seal([(tuple(p), dict(kt), int(ln)) for p, kt, ln in rows])

    # ---- state

    def _seal(self, rows):
        """flush `rows` from scratch: the oracle's index and its relation; no growing rows, nothing deleted"""
        self.sealed = rows
        self.sealed_deleted = np.zeros(len(rows), bool)
        self.growing, self.growing_deleted = [], []
        self.growing_batch = []   # per growing row: the number of the insert (insert's `batch`) that appended it
        self._first = {}          # side -> (rows covered, {payload: lowest row index}), see first_rows
        # the live side (rerank_op): the rows its ctid directory covers, the growing rows appended to its handle and in how many
        # appends since the last sync, whether the epoch's search hits have been reranked
        self._live_covered, self._live_appended, self._live_pending, self._live_hits_done = len(rows), 0, 0, False
        self.ginv = {}     # key -> [(g, tf)] of the growing rows, g ascending
        vocab = sorted({key for _, kt, _ in rows for key in kt})
        self.vocab, self.rank = vocab, {key: t for t, key in enumerate(vocab)}
        t_of, d_of, tf_of = [], [], []
        for d, (_, kt, _) in enumerate(rows):
            for key, tf in kt.items():
                t_of.append(self.rank[key])
                d_of.append(d)
                tf_of.append(tf)
        t_of, d_of, tf_of = np.array(t_of, np.int64), np.array(d_of, np.int64), np.array(tf_of, np.uint32)
        order = np.lexsort((d_of, t_of))
        term_start = np.r_[0, np.cumsum(np.bincount(t_of, minlength=len(vocab)))].astype(np.uint64)
        term_key = np.frombuffer(b"".join(vocab), np.uint8).reshape(-1, 16) if vocab else np.zeros((0, 16), np.uint8)
        self.oix = orc.OracleIndex.build(self.k1, self.b, np.array([ln for _, _, ln in rows], np.uint32),
                                         np.array([p for p, _, _ in rows], np.uint16).reshape(-1, 3), term_key, term_start,
                                         d_of[order].astype(np.uint32), tf_of[order])
        assert self.oix.n_docs == len(rows) and self.oix.n_terms == len(vocab)
        self.pages = orc.Pages(self.oix, seed=self.seed)
        self._doc_slots = None
        self._eval = {}

    def doc_slots(self):
        """(page id, offset of the DocumentTuple) of every sealed row in id order: Meta -> Jump -> ptr_documents -> the chain"""
        if self._doc_slots is None:
            p0 = self.pages.page(0)
            ptr_jump = struct.unpack_from("<I", p0, _slots(p0)[0] + 36)[0]
            pj = self.pages.page(ptr_jump)
            p = struct.unpack_from("<I", pj, _slots(pj)[0] + 44)[0]
            where = []
            while p != NONE:
                pg = self.pages.page(p)
                where += [(p, off) for off in _slots(pg)]
                p = struct.unpack_from("<I", pg, 8184)[0]
            assert len(where) == len(self.sealed)
            self._doc_slots = where
        return self._doc_slots

    def page_list(self):
        return [self.pages.page(i) for i in range(len(self.pages))]

    # ---- mutations

    def new_batch(self):
        """a number for insert's `batch`: the rows of one INSERT statement share one"""
        self._n_batches += 1
        return self._n_batches

    def insert(self, payload, kt, batch=None):
        keys = sorted(kt)
        self.pages.insert(np.array(payload, np.uint16), keys, [kt[key] for key in keys])
        g = len(self.growing)
        self.growing.append((tuple(int(x) for x in payload), dict(kt), length_of(kt)))
        self.growing_deleted.append(False)
        self.growing_batch.append(self.new_batch() if batch is None else batch)
        for key in keys:
            self.ginv.setdefault(key, []).append((g, kt[key]))
        return g

    def delete_sealed(self, d):
        p, off = self.doc_slots()[d]
        self.pages.page(p, writable=True)[off] = 1   # DocumentTuple.deleted
        self.sealed_deleted[d] = True

    def delete_growing(self, g):
        self.pages.mark_deleted_growing(g)
        self.growing_deleted[g] = True

    def delete_tids(self, tids, what=None):
        """every sealed and growing row whose payload is among the ctids `tids` ([n, 3], repeats and ctids of no row allowed) is
        deleted (bulkdelete.rs).  Returns (sealed rows newly dead, growing rows newly dead, growing rows matched, the already dead
        ones included).  what: "bulkdelete" or "delete" counts the call for the ctid life's coverage conditions."""
        want = {tuple(int(x) for x in t) for t in tids}
        held = {p for p, _, _ in self.sealed} | {p for p, _, _ in self.growing}
        dead_named = any(p in want for d, (p, _, _) in enumerate(self.sealed) if self.sealed_deleted[d]) or \
            any(p in want for g, (p, _, _) in enumerate(self.growing) if self.growing_deleted[g])
        new_s = [d for d, (p, _, _) in enumerate(self.sealed) if p in want and not self.sealed_deleted[d]]
        hit_g = [g for g, (p, _, _) in enumerate(self.growing) if p in want]
        new_g = [g for g in hit_g if not self.growing_deleted[g]]
        for d in new_s:
            self.delete_sealed(d)
        for g in new_g:
            self.delete_growing(g)
        if what == "bulkdelete":
            self.cstats["bulk_full"] += bool(new_s and new_g and dead_named and want - held)
        elif what == "delete":
            self.cstats["delete_batches"] += len({self.growing_batch[g] for g in hit_g}) > 1
        return len(new_s), len(new_g), len(hit_g)

    # ---- what a filter built from the rows holds

    def alive(self):
        """keep predicate 0: (sealed, growing) bool arrays, not deleted"""
        return ~self.sealed_deleted, ~np.array(self.growing_deleted, bool)

    @staticmethod
    def tenant_bits(rows):
        return np.array([p[2] % 3 == 0 for p, _, _ in rows], bool)

    def tenant(self):
        """keep predicate 1: payload[2] % 3 == 0 and alive"""
        s, g = self.alive()
        return s & self.tenant_bits(self.sealed), g & self.tenant_bits(self.growing)

    def keep_of(self, selector):
        return None if selector == NONE else (self.alive(), self.tenant())[selector]

    def growing_csr(self, lo=0, hi=None):
        """the growing rows lo .. hi - 1 (default: all) as the arrays vbm25_growing_from_pages gives"""
        L = orc.lib()
        rows, deleted = self.growing[lo:hi], self.growing_deleted[lo:hi]
        counts = [len(kt) for _, kt, _ in rows]
        keys = b"".join(key for _, kt, _ in rows for key in sorted(kt))
        return dict(g_start=np.r_[0, np.cumsum(counts)].astype(np.uint64), g_key=np.frombuffer(keys, np.uint8).copy(),
                    g_tf=np.array([kt[key] for _, kt, _ in rows for key in sorted(kt)], np.uint32),
                    g_fieldnorm=np.array([L.orc_length_to_fieldnorm(ln) for _, _, ln in rows], np.uint8),
                    g_payload=np.array([p for p, _, _ in rows], np.uint16).reshape(-1, 3),
                    g_deleted=np.array(deleted, np.uint8))

    def counts(self):
        """(sealed rows, deleted ones, growing rows, deleted ones, growing elements): vbm25_device_vacuum_info's five"""
        return (len(self.sealed), int(self.sealed_deleted.sum()), len(self.growing), int(sum(self.growing_deleted)),
                sum(len(kt) for _, kt, _ in self.growing))

    # ---- SELECT

    def _evaluate(self, t, fieldnorm, tf):
        at = (t, fieldnorm, tf)
        if at not in self._eval:
            o = self.oix
            self._eval[at] = orc.lib().orc_cache_evaluate(o.n_docs, int(o.arrays["term_df"][t]), o.k1, o.b, o.sum_len / o.n_docs,
                                                          fieldnorm, tf)
        return self._eval[at]

    def select(self, query_keys, k, keep=None, count=True):
        """the first k records (orc.HIT_DTYPE) of the table's ranking for the query; keep: None (every sealed row, deleted ones
        included; every live growing row) or (sealed, growing) bool arrays"""
        out = np.zeros(0, orc.HIT_DTYPE)
        if self.oix.n_docs == 0:   # no statistics: nothing scores
            return self._counted(out, False, False, count)
        L = orc.lib()
        qkeys = [key for key in sorted(set(query_keys)) if key in self.rank]   # unknown keys are ignored (search.rs:59-61)
        sealed = self.oix.search_brute([self.rank[key] for key in qkeys], MAX_K)
        assert len(sealed) < MAX_K, "the brute-force ranking was cut"
        if keep is not None:
            sealed = sealed[keep[0][sealed["doc_id"]]]
        acc = {}
        for key in qkeys:   # ascending keys: each row's sum runs in key order
            for g, tf in self.ginv.get(key, ()):
                if self.growing_deleted[g] or (keep is not None and not keep[1][g]):
                    continue
                fn = L.orc_length_to_fieldnorm(self.growing[g][2])
                acc[g] = acc.get(g, 0.0) + self._evaluate(self.rank[key], fn, tf)
        grow = sorted((-s, g) for g, s in acc.items() if s > 0)
        merged, i, j = [], 0, 0
        while len(merged) < k and (i < len(sealed) or j < len(grow)):
            if j == len(grow) or (i < len(sealed) and sealed["score"][i] >= -grow[j][0]):   # sealed first on equal scores
                merged.append((float(sealed["score"][i]), int(sealed["doc_id"][i]), tuple(sealed["payload"][i])))
                i += 1
            else:
                g = grow[j][1]
                merged.append((-grow[j][0], NONE - g, self.growing[g][0]))
                j += 1
        out = np.zeros(len(merged), orc.HIT_DTYPE)
        for r, (s, d, p) in enumerate(merged):
            out[r] = (s, d, p)
        n_sealed = len(self.sealed)
        is_g = out["doc_id"] >= n_sealed
        tie = bool(np.any((out["score"][1:] == out["score"][:-1]) & (is_g[1:] != is_g[:-1])))
        shown = keep is None and bool(self.sealed_deleted[out["doc_id"][~is_g]].any())
        return self._counted(out, tie, shown, count, both=bool(is_g.any() and (~is_g).any()))

    def _counted(self, out, tie, shown, count, both=False):
        if count:
            s = self.stats
            s["selects"] += 1
            s["both"] += both
            s["nothing"] += len(out) == 0
            s["deleted_shown"] += shown
            s["mixed_ties"] += tie
        return out

    # ---- the forward index and the rerank step

    def forward(self):
        """the sealed rows as a forward index: (start uint64 [n + 1], term uint32, tf uint32, fieldnorm uint8 [n]) -- per row its
        term ranks ascending with their tf, and the fieldnorm code of its STORED length (after a VACUUM a kept sealed row's length
        is its number of postings, _seal's rows carry it)"""
        L = orc.lib()
        start, term, tf, fn = [0], [], [], []
        for _, kt, ln in self.sealed:
            for key in sorted(kt):
                term.append(self.rank[key])
                tf.append(kt[key])
            start.append(len(term))
            fn.append(L.orc_length_to_fieldnorm(ln))
        return np.array(start, np.uint64), np.array(term, np.uint32), np.array(tf, np.uint32), np.array(fn, np.uint8)

    def _operator(self, t, fieldnorm, tf):
        """one term of the `<&>` operator: idf * tf (evaluate.rs:22-74 with bm25.rs:285-295).  NOT _evaluate: the search multiplies
        tf into the cached idf * (k1 + 1) before it divides (Cache::evaluate, bm25.rs:355-358), the operator divides first, and the
        two differ in the last bit for some postings."""
        at = ("<&>", t, fieldnorm, tf)
        if at not in self._eval:
            o, L = self.oix, orc.lib()
            self._eval[at] = L.orc_idf(o.n_docs, int(o.arrays["term_df"][t])) * L.orc_tf(fieldnorm, tf, o.k1, o.b, o.sum_len / o.n_docs)
        return self._eval[at]

    def first_rows(self, side):
        """{payload: the lowest row index of `side` that carries it}"""
        rows = self.sealed if side == "sealed" else self.growing
        n, first = self._first.get(side, (0, {}))
        for i in range(n, len(rows)):   # (rows are only ever appended between two _seal)
            first.setdefault(rows[i][0], i)
        self._first[side] = (len(rows), first)
        return first

    def live_row(self, i):
        """row i of sealed + growing, the documents of an index-bound handle that every insert was appended to"""
        n_sealed = len(self.sealed)
        return self.sealed[i] if i < n_sealed else self.growing[i - n_sealed]

    def live_index(self, tid, covered=None):
        """the lowest index of sealed + growing (its first `covered` rows; default: all) that carries the ctid, or None.  A sealed
        row beats a growing one, dead or not: every growing index exceeds every sealed one (live_merge_kernel's stable merge on
        (key, doc))."""
        tid = tuple(int(x) for x in tid)
        i = self.first_rows("sealed").get(tid)
        if i is None:
            g = self.first_rows("growing").get(tid)
            i = None if g is None else len(self.sealed) + g
        return i if i is None or covered is None or i < covered else None

    def _row_score(self, row, qkeys):
        _, kt, ln = row
        fn, s = orc.lib().orc_length_to_fieldnorm(ln), 0.0
        for key in qkeys:
            if key in kt:
                s += self._operator(self.rank[key], fn, kt[key])
        return s

    @staticmethod
    def _top(entries, k):
        best = sorted(entries, key=lambda e: -e[0])[:k]   # (sorted is stable: equal scores stay in list order)
        ranks = np.zeros(k, RANK_DTYPE)
        for r, e in enumerate(best):
            ranks[r] = e
        return ranks, len(best), len(entries)

    def rerank(self, query_keys, cand_tids, k, side, covered=None):
        """the rerank step (`<&>` over a candidate list, top k) on the rows of one side, "sealed" or "growing" -> (ranks [k] of
        RANK_DTYPE, n_ranks, eligible candidates).  A ctid names the lowest row index of the side that carries it; one no row of the
        side carries is not eligible, and the others keep their positions in the list.  DELETION IS NOT CONSULTED: the reranker
        knows the documents it was bound to, not their deleted flags, so a dead row scores like a live one.  A row's score is the
        sum of _operator(rank, its fieldnorm, tf) from 0.0 in ascending key order over the distinct query keys that the sealed
        vocabulary and the row hold; growing rows take the sealed statistics and their own length (what binding cast documents to
        the index's vocabulary keeps).  The result is the stable descending sort of the eligible entries cut at k: (score, pos in
        the list, row index), zeros behind them.
        side "live": the rows are sealed + growing in that order, indexed 0 .. n_sealed + n_growing - 1 (live_index); `covered`
        (default: all) is the number of them that the ctid directory knows.  So a dead sealed row's ctid, inserted again before the
        VACUUM, still names the sealed row: DESIGN section 6, "Not in: deleting documents from a bound handle"."""
        assert side in ("sealed", "growing", "live") and (covered is None or side == "live")
        qkeys = [key for key in sorted(set(query_keys)) if key in self.rank]
        entries = []
        if side == "live":
            for pos, tid in enumerate(cand_tids):
                i = self.live_index(tid, covered)
                if i is not None:
                    entries.append((self._row_score(self.live_row(i), qkeys), pos, i))
            return self._top(entries, k)
        rows, first = (self.sealed if side == "sealed" else self.growing), self.first_rows(side)
        for pos, tid in enumerate(cand_tids):
            i = first.get(tuple(int(x) for x in tid))
            if i is not None:
                entries.append((self._row_score(rows[i], qkeys), pos, i))
        return self._top(entries, k)

    def rerank_docs(self, query_keys, doc_indices, k):
        """rerank's "live" side for a list of indices into sealed + growing (the cand_doc route): pos is the position in the list,
        and every index is eligible"""
        qkeys = [key for key in sorted(set(query_keys)) if key in self.rank]
        return self._top([(self._row_score(self.live_row(int(i)), qkeys), pos, int(i)) for pos, i in enumerate(doc_indices)], k)

    def forward_live(self, drop_deleted=False):
        """sealed + growing as a forward index: forward()'s four arrays, continued by the growing rows -- each the ranks of those of
        its keys that the sealed vocabulary holds, ascending, with their tf, and the fieldnorm code of its own stored length (keys
        outside the vocabulary counted).  drop_deleted: a growing row flagged deleted has an empty run and keeps its code, what
        vbm25_doc_terms_append documents for a CSR with `deleted` flags."""
        L = orc.lib()
        start, term, tf, fn = (list(a) for a in self.forward())
        for g, (_, kt, ln) in enumerate(self.growing):
            if not (drop_deleted and self.growing_deleted[g]):
                known = sorted((self.rank[key], kt[key]) for key in kt if key in self.rank)
                term += [t for t, _ in known]
                tf += [c for _, c in known]
            start.append(len(term))
            fn.append(L.orc_length_to_fieldnorm(ln))
        return np.array(start, np.uint64), np.array(term, np.uint32), np.array(tf, np.uint32), np.array(fn, np.uint8)

    def live_append(self, n_rows):
        """the driver appended one cast handle of the next n_rows growing rows to the live handle (rows the model already holds)"""
        lo = self._live_appended
        assert 0 < n_rows <= len(self.growing) - lo
        self._live_appended, self._live_pending = lo + n_rows, self._live_pending + 1
        self.cstats["unknown_handle"] += not any(key in self.rank for _, kt, _ in self.growing[lo:lo + n_rows] for key in kt)

    def growing_hits(self, queries, k):
        """per query the live indices of the first k records a search returns (deleted growing rows are skipped, a deleted sealed row is
        shown): a hit 0xFFFFFFFF - g is document n_sealed + g"""
        n_sealed = len(self.sealed)
        hits = [self.select(keys, k, None, count=False)["doc_id"].astype(np.int64) for keys in queries]
        return [np.where(h >= n_sealed, n_sealed + (NONE - h), h).astype(np.uint32) for h in hits]

    def rerank_op(self, queries, lists, k, count=True):
        """rerank of every (query keys, ctid list) pair on both sides -> {side: (ranks [nq, k], n_ranks uint32 [nq])}, and on the
        live side as a ring on ONE index-bound handle answers it, which is synced only here, when a rerank needs it:
          "live"           the result over all rows (after the sync)
          "live_before"    the result over the rows the directory covered before this rerank, "live_covered" of them; None where
                           nothing was pending (or the table has no sealed row: no ring exists)
          "live_docs"      per query the live indices of the eligible candidates, in list order; "live_by_doc": rerank_docs of them
          "hits"           once per epoch, at the first rerank that finds a deleted growing row: growing_hits(queries, HITS_K), with
                           "hits_by_doc" rerank_docs of them; else None"""
        out, seen = {}, {}
        stack = lambda got: (np.stack([g[0] for g in got]) if got else np.zeros((0, k), RANK_DTYPE), np.array([g[1] for g in got], np.uint32))
        n_sealed, n_rows = len(self.sealed), len(self.sealed) + len(self.growing)
        if self._live_appended < len(self.growing):   # (a driver without a live handle reports no appends: one delta)
            self._live_appended, self._live_pending = len(self.growing), self._live_pending + 1
        covered, pending = self._live_covered, self._live_pending
        out["live_before"], out["live_covered"] = None, covered
        if n_sealed and covered != n_rows:
            out["live_before"] = stack([self.rerank(keys, tids, k, "live", covered) for keys, tids in zip(queries, lists)])
            self._live_covered, self._live_pending = n_rows, 0
        got_live = [self.rerank(keys, tids, k, "live") for keys, tids in zip(queries, lists)]
        out["live"] = stack(got_live)
        out["live_docs"] = [np.array([i for i in (self.live_index(t) for t in tids) if i is not None], np.uint32) for tids in lists]
        out["live_by_doc"] = stack([self.rerank_docs(keys, docs, k) for keys, docs in zip(queries, out["live_docs"])])
        out["hits"] = None
        if n_sealed and not self._live_hits_done and any(self.growing_deleted):
            self._live_hits_done = True
            out["hits"] = self.growing_hits(queries, HITS_K)
            out["hits_by_doc"] = stack([self.rerank_docs(keys, docs, k) for keys, docs in zip(queries, out["hits"])])
        if count and n_sealed:
            c, (ranks, n_ranks) = self.cstats, out["live"]
            scored = [ranks["doc"][q, :n][ranks["score"][q, :n] != 0] for q, n in enumerate(n_ranks)]
            c["live_both"] += any((d < n_sealed).any() and (d >= n_sealed).any() for d in scored)
            first_s, first_g = self.first_rows("sealed"), self.first_rows("growing")
            c["live_shared"] += any(tuple(int(x) for x in t) in first_s and tuple(int(x) for x in t) in first_g for tids in lists for t in tids)
            c["live_short"] += any(g[1] < k for g in got_live)
            c["live_cut"] += any(g[1] == k < g[2] for g in got_live)
            if out["live_before"] is not None:
                c["sync_multi"] += pending >= 2
                c["sync_one"] += n_rows - covered == 1
                c["ab_differ"] += out["live_before"][0].tobytes() != ranks.tobytes()
            if out["hits"] is not None:
                c["live_hits"] += any((h >= n_sealed).any() for h in out["hits"])
        for side in ("sealed", "growing"):
            got = [self.rerank(keys, tids, k, side) for keys, tids in zip(queries, lists)]
            ranks = np.stack([g[0] for g in got]) if got else np.zeros((0, k), RANK_DTYPE)
            out[side] = (ranks, np.array([g[1] for g in got], np.uint32))
            first = self.first_rows(side)
            seen[side] = dict(nonzero=bool((ranks["score"] != 0).any()),
                              ineligible=any(tuple(int(x) for x in t) not in first for tids in lists for t in list(tids)[:k]),
                              short=any(g[1] < k for g in got), cut=any(g[1] == k < g[2] for g in got))
        if count:
            c = self.cstats
            c["reranks"] += 1
            c["rerank_both"] += seen["sealed"]["nonzero"] and seen["growing"]["nonzero"]
            c["ineligible_sealed"] += seen["sealed"]["ineligible"]
            c["ineligible_growing"] += seen["growing"]["ineligible"]
            c["rerank_short"] += seen["sealed"]["short"] or seen["growing"]["short"]
            c["rerank_cut"] += seen["sealed"]["cut"] or seen["growing"]["cut"]
        return out

    # ---- VACUUM

    def vacuum(self):
        """compacts the table; returns the relabel array: old sealed ids, then old growing indices -> new id or 0xFFFFFFFF"""
        rows, relabel = [], []
        for d, (p, kt, _) in enumerate(self.sealed):
            relabel.append(NONE if self.sealed_deleted[d] else len(rows))
            if not self.sealed_deleted[d]:
                rows.append((p, kt, len(kt)))   # maintain.rs:344-362: one per posting
        for g, row in enumerate(self.growing):
            relabel.append(NONE if self.growing_deleted[g] else len(rows))
            if not self.growing_deleted[g]:
                rows.append(row)
        new_keys = {key for g, (_, kt, _) in enumerate(self.growing) if not self.growing_deleted[g] for key in kt if key not in self.rank}
        self.vacuums.append((int(self.sealed_deleted.sum()), int(sum(self.growing_deleted)), len(new_keys)))
        self._seal(rows)
        return np.array(relabel, np.uint32)

    # ---- the operation sequence

    def epoch_k(self):
        """the k of the front ends that are created once per epoch (the time between two VACUUMs): every k of KS in turn"""
        return KS[len(self.vacuums) % len(KS)]

    def ops(self, seed, n, universe=None):
        """n operations drawn from the reference's mix (tests/fuzz: 2 INSERT : 4 SELECT : 3 DELETE : 1 VACUUM) against the table's
        state at the time each is drawn (the consumer applies an operation before it asks for the next), a ("reopen",) in front of
        every 10th:
          ("insert", [(payload, {key: tf})])      1, 4 or 16 rows, to be inserted one by one (with one row per INSERT the growing
                                                  segment of this mix holds two rows on average and few selects see it): each of
                                                  1, 3, 30 or 250 distinct keys of `universe` (default: the vocabulary now), tf 1..8;
                                                  with probability 0.2 one of them is a key no row has held
          ("delete", "sealed" | "growing", ids)   1, 3 or 40 rows of one segment, already deleted ones included
          ("select", queries, selectors, k, front end)   8 queries of 1 to 6 keys from the sealed vocabulary and the last inserts' keys,
                                                  a third of them with a key no row holds as well; selectors cycle NO_FILTER, 0, 1;
                                                  front ends 0, 1, 2 in rotation: 0 takes a k drawn from KS, the others epoch_k()
          ("vacuum",)"""
        rng = np.random.default_rng(seed)
        universe = list(self.vocab if universe is None else universe)
        recent, serial, n_selects = [], 0, 0
        for i in range(n):
            if i and i % 10 == 0:
                yield ("reopen",)
            kind = int(rng.choice(4, p=[0.2, 0.4, 0.3, 0.1]))
            if kind == 0:
                docs = []
                for _ in range(int(rng.choice(INSERT_ROWS))):
                    nk = int(rng.choice(INSERT_KEYS))
                    keys = [universe[j] for j in rng.choice(len(universe), min(nk, len(universe)), replace=False)]
                    if rng.random() < 0.2:
                        keys[0] = new_key(seed * 1000 + serial)
                        serial += 1
                    kt = {key: int(tf) for key, tf in zip(keys, rng.integers(1, 9, len(keys)))}
                    recent = (recent + [list(kt)])[-8:]
                    docs.append((tuple(int(x) for x in rng.integers(0, 65536, 3)), kt))
                yield ("insert", docs)
            elif kind == 1:
                queries = []
                for _ in range(8):
                    pool_r = [key for keys in recent for key in keys]
                    q = []
                    for _ in range(int(rng.integers(1, 7))):
                        pool = pool_r if pool_r and (rng.random() < 0.5 or not self.vocab) else self.vocab
                        if pool:
                            q.append(pool[int(rng.integers(len(pool)))])
                    if not q or rng.random() < 1 / 3:
                        q.append(NO_ROW_KEY)
                    queries.append(sorted(set(q)))
                selectors = [(NONE, 0, 1)[(q + n_selects) % 3] for q in range(8)]
                k, front = int(rng.choice(KS)), n_selects % 3
                yield ("select", queries, selectors, k if front == 0 else self.epoch_k(), front)
                n_selects += 1
            elif kind == 2:
                where = "growing" if self.growing and rng.random() < 0.4 else "sealed"
                n_rows = len(self.growing) if where == "growing" else len(self.sealed)
                many = int(rng.choice((1, 3, 40)))
                yield ("delete", where, [int(x) for x in rng.integers(0, n_rows, many)] if n_rows else [])
            else:
                yield ("vacuum",)

    # ---- the same life by lexeme and ctid

    def keys_of(self, lexemes):
        """a query's lexemes -> its sorted distinct keys (cast_tsvector_to_query)"""
        return sorted({self.key_of[t] for t in lexemes})

    def cast(self, lexrow):
        """a row [(lexeme, count)] -> {key: tf}: the counts of equal lexemes add up (cast_tsvector_to_document)"""
        kt = {}
        for t, c in lexrow:
            kt[self.key_of[t]] = min(kt.get(self.key_of[t], 0) + c, 2 ** 32 - 1)
        return kt

    def ops_ctid(self, seed, n, universe):
        """ops' mix and ("reopen",) cadence, in the terms a serving process is handed: lexemes and ctids.  `universe` is a list of
        (lexeme, key) with key = intern(lexeme) under the index's seed, every key of the table's rows among them; self.key_of maps
        every lexeme the sequence has named to its key (new lexemes and NO_ROW_LEXEME are shorter than 16 bytes: zero padded).
          ("insert", [(payload, [(lexeme, count)])])   ops' rows, each key's tf split over 1 to 3 entries of its lexeme, shuffled;
                                                  payloads have field 0 < 0xFFFF and field 2 >= 1 (so the ctids below that no row
                                                  carries are certain); one row in ten takes the ctid of a live row of the table
          ("delete_tids", tids)                   the ctids of 1, 3 or 40 rows of both segments, dead ones included, one more of a
                                                  dead row where there is one, one that no row carries, one of them twice; shuffled
          ("select", queries, selectors, k, front end)   ops' selects, the queries as lexemes, some lexeme twice
          ("rerank", queries, lists, k)           after every other select on average: its queries, each with a ctid list -- in
                                                  turn the payloads of the first 5, 30 or 100 rows the select returns now (sealed and
                                                  growing mixed), those of 1, 20 or 200 random rows of either segment, and an edge:
                                                  a ctid no row carries in front, behind or alone, a repeated ctid, the empty list;
                                                  k from RERANK_KS
          ("vacuum", tids)                        "the dead TIDs the heap reports": delete_tids' mix, empty one time in three"""
        rng = np.random.default_rng(seed)
        self.key_of = {lexeme: key for lexeme, key in universe}
        self.key_of[NO_ROW_LEXEME] = NO_ROW_KEY
        lexeme_of = {key: lexeme for lexeme, key in universe}
        ukeys = [key for _, key in universe]
        assert all(key in lexeme_of for key in self.vocab)
        recent, serial, n_selects, n_reranks = [], 0, 0, 0

        def absent():
            return (int(rng.integers(0, 65536)), int(rng.integers(0, 65536)), 0)

        def any_row():
            n_s, n_g = len(self.sealed), len(self.growing)
            if n_g and (not n_s or rng.random() < 0.4):
                return self.growing[int(rng.integers(n_g))][0]
            return self.sealed[int(rng.integers(n_s))][0] if n_s else absent()

        def ctid_mix():
            tids = [any_row() for _ in range(int(rng.choice((1, 3, 40))))]
            dead = [p for d, (p, _, _) in enumerate(self.sealed) if self.sealed_deleted[d]] + \
                   [p for g, (p, _, _) in enumerate(self.growing) if self.growing_deleted[g]]
            if dead:
                tids.append(dead[int(rng.integers(len(dead)))])
            tids.append(absent())
            tids.append(tids[int(rng.integers(len(tids)))])
            return [tids[i] for i in rng.permutation(len(tids))]

        def as_lexemes(keys):
            q = [lexeme_of[key] for key in keys]
            if rng.random() < 0.3:
                q.append(q[int(rng.integers(len(q)))])
            return [q[i] for i in rng.permutation(len(q))]

        for i in range(n):
            if i and i % 10 == 0:
                yield ("reopen",)
            kind = int(rng.choice(4, p=[0.2, 0.4, 0.3, 0.1]))
            if kind == 0:
                docs = []
                for _ in range(int(rng.choice(INSERT_ROWS))):
                    nk = int(rng.choice(INSERT_KEYS))
                    keys = [ukeys[j] for j in rng.choice(len(ukeys), min(nk, len(ukeys)), replace=False)]
                    if rng.random() < 0.2:
                        keys[0] = new_key(seed * 1000 + serial)
                        lexeme_of[keys[0]] = keys[0].rstrip(b"\0")
                        self.key_of[lexeme_of[keys[0]]] = keys[0]
                        serial += 1
                    row = []
                    for key, tf in zip(keys, rng.integers(1, 9, len(keys))):
                        cuts = sorted(int(c) for c in rng.integers(1, int(tf) + 1, int(rng.integers(0, 3))))
                        row += [(lexeme_of[key], b - a) for a, b in zip([0] + cuts, cuts + [int(tf)]) if b > a]
                    recent = (recent + [keys])[-8:]
                    payload = (int(rng.integers(0, 65535)), int(rng.integers(0, 65536)), int(rng.integers(1, 65536)))
                    if rng.random() < 0.1:   # (a live row's: a heap hands a dead row's ctid out again only after the VACUUM)
                        live = [p for d, (p, _, _) in enumerate(self.sealed) if not self.sealed_deleted[d]] + \
                               [p for g, (p, _, _) in enumerate(self.growing) if not self.growing_deleted[g]]
                        if live:
                            payload = live[int(rng.integers(len(live)))]
                    docs.append((payload, [row[j] for j in rng.permutation(len(row))]))
                yield ("insert", docs)
            elif kind == 1:
                queries = []
                for _ in range(8):
                    pool_r = [key for keys in recent for key in keys]
                    q = []
                    for _ in range(int(rng.integers(1, 7))):
                        pool = pool_r if pool_r and (rng.random() < 0.5 or not self.vocab) else self.vocab
                        if pool:
                            q.append(pool[int(rng.integers(len(pool)))])
                    if not q or rng.random() < 1 / 3:
                        q.append(NO_ROW_KEY)
                        lexeme_of[NO_ROW_KEY] = NO_ROW_LEXEME
                    queries.append(as_lexemes(sorted(set(q))))
                selectors = [(NONE, 0, 1)[(q + n_selects) % 3] for q in range(8)]
                k, front = int(rng.choice(KS)), n_selects % 3
                yield ("select", queries, selectors, k if front == 0 else self.epoch_k(), front)
                n_selects += 1
                if rng.random() < 0.5:
                    lists = []
                    for q, lexemes in enumerate(queries):
                        shown = [tuple(int(x) for x in p) for p in
                                 self.select(self.keys_of(lexemes), int(rng.choice((5, 30, 100))), None, count=False)["payload"]]
                        source = (q + n_reranks) % 3
                        if source == 0:
                            tids = shown
                        elif source == 1:
                            tids = [any_row() for _ in range(int(rng.choice((1, 20, 200))))]
                        else:
                            edge = int(rng.integers(5))
                            tids = ([absent()] + shown, shown + [absent()], [absent()],
                                    shown + shown[:1] + [any_row()] * 2, [])[edge]
                        lists.append(tids)
                    yield ("rerank", queries, lists, int(rng.choice(RERANK_KS)))
                    n_reranks += 1
            elif kind == 2:
                yield ("delete_tids", ctid_mix())
            else:
                yield ("vacuum", [] if rng.random() < 1 / 3 else ctid_mix())
