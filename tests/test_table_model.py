"""tests/table_model.py against the library's host side, along the operation sequences tests/test_gpu_table_fuzz.py runs on the
device: the host readers of the model's pages give the model's state, its SELECT is vbm25_merge_hits(the oracle's brute-force
ranking, vbm25_growing_search) bit for bit, and its VACUUM is tests/maintain_model.py put through the host builder.  Also the
coverage conditions of the chosen seeds, on the model alone.  No GPU use."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import maintain_model
import orc
import table_model as T
import vectors_device_data as V
from parity import assert_bit_exact
from test_segment_builder import assert_same_index

SEEDS = (1, 4, 8)   # chosen for the coverage conditions (assert_coverage)
N_OPS = 160
SEED32 = bytes(range(32))


def assert_readers_give_the_state(m, sealed=True):
    """the host readers of the model's pages: the deleted flags, the growing CSR and (sealed=True) the index arrays"""
    pl = m.page_list()
    assert np.array_equal(vb.sealed_deleted_from_pages(pl), m.sealed_deleted)
    V.assert_same_csr(vb.growing_from_pages(pl), m.growing_csr(), "growing rows")
    if sealed:
        assert_same_index(vb.segment_from_pages(pl), m.oix)
    return pl


def library_select(m, seg, csr, keys, k, keep):
    """the host composition: the oracle's brute-force ranking of the sealed rows, filtered, merged with vbm25_growing_search"""
    if m.oix.n_docs == 0:
        return np.zeros(0, vb.HIT_DTYPE)
    ranks = [m.rank[key] for key in keys if key in m.rank]
    sealed = m.oix.search_brute(ranks, T.MAX_K)
    g_del = csr["g_deleted"]
    if keep is not None:
        sealed = sealed[keep[0][sealed["doc_id"]]]
        g_del = ((g_del != 0) | ~keep[1]).astype(np.uint8)
    grow = vb.growing_search(seg, vb.Query(keys), k, csr["g_start"], csr["g_key"], csr["g_tf"], csr["g_fieldnorm"], csr["g_payload"], g_del)
    return vb.merge_hits(sealed[:k], grow, k)


def check_vacuum(m):
    """the model's VACUUM against maintain_model.maintain + vb.Segment.build on what the host readers give"""
    pl = assert_readers_give_the_state(m)
    seg = vb.segment_from_pages(pl)
    args, want = maintain_model.maintain(seg.arrays(), seg.meta(), vb.sealed_deleted_from_pages(pl), vb.growing_from_pages(pl))
    relabel = m.vacuum()
    assert np.array_equal(relabel, want)
    if m.oix.n_docs:   # (vb.Segment.build refuses a segment without documents)
        assert_same_index(vb.Segment.build(*args), m.oix)
    else:
        assert len(args[2]) == 0
    assert_readers_give_the_state(m)


def apply(m, op):
    """an INSERT or a DELETE on the model alone"""
    if op[0] == "insert":
        for payload, kt in op[1]:
            m.insert(payload, kt)
    elif op[1] == "sealed":
        for d in op[2]:
            m.delete_sealed(d)
    else:
        for g in op[2]:
            m.delete_growing(g)


def assert_coverage(m, what):
    """the conditions a random seed has to meet (asserted by the device test as well)"""
    s, v = m.stats, m.vacuums
    print(f"{what}: {len(v)} vacuums {v}; {s}")
    assert len(v) >= 3, what
    assert any(sd and gd and nk for sd, gd, nk in v), f"{what}: no vacuum with sealed deletes, growing deletes and new keys"
    assert 4 * s["both"] >= s["selects"], f"{what}: {s['both']} of {s['selects']} selects returned both segments"
    assert 10 * s["nothing"] <= s["selects"], f"{what}: {s['nothing']} of {s['selects']} selects returned nothing"
    assert s["deleted_shown"] >= 1, f"{what}: no deleted sealed row among an unfiltered select's records"
    assert s["mixed_ties"] >= 1, f"{what}: no tie group with a sealed and a growing record"


def new_table(seed):
    rows, universe = T.random_rows(3000, 300, seed)
    return T.Table(rows, 1.2, 0.75, SEED32), universe


@pytest.mark.parametrize("seed", SEEDS)
def test_model_along_a_random_life(seed):
    m, universe = new_table(seed)
    assert_readers_give_the_state(m)
    seg = csr = None
    for op in m.ops(seed, N_OPS, universe):
        if op[0] in ("insert", "delete"):
            apply(m, op)
            assert_readers_give_the_state(m, sealed=False)
            seg = None
        elif op[0] == "reopen":
            assert_readers_give_the_state(m)
        elif op[0] == "vacuum":
            check_vacuum(m)
            seg = None
        else:
            _, queries, selectors, k, _ = op
            if seg is None:
                pl = m.page_list()
                seg, csr = vb.segment_from_pages(pl), vb.growing_from_pages(pl)
            for keys, sel in zip(queries, selectors):
                keep = m.keep_of(sel)
                got = m.select(keys, k, keep)
                assert_bit_exact(library_select(m, seg, csr, keys, k, keep), got, f"seed {seed} k={k} selector {sel}")
                if sel == T.NONE and m.sealed_deleted[got["doc_id"][got["doc_id"] < len(m.sealed)]].any():
                    hidden = m.select(keys, k, m.keep_of(0), count=False)   # the same query under `alive`: the deleted row is gone
                    assert not m.sealed_deleted[hidden["doc_id"][hidden["doc_id"] < len(m.sealed)]].any()
    assert_coverage(m, f"seed {seed}")


# ---- the same life by lexeme and ctid (Table.ops_ctid), as tests/test_gpu_table_ctid_fuzz.py runs it on the device

SEEDS_CTID = (1, 4)  # chosen for the coverage conditions (assert_coverage_ctid)


def lexeme_universe(vocab=300):
    """[(lexeme, key)] of the tokens 0 .. vocab - 1: decimal digits, every third one with a prefix that takes it past 15 bytes, so
    its key is the keyed hash (vector.rs:19-35; the host intern has its own test in tests/test_blake3.py)"""
    lexemes = [b"%d" % t if t % 3 else b"a lexeme of more than fifteen bytes %d" % t for t in range(vocab)]
    return [(t, vb.intern(t, SEED32)) for t in lexemes]


def new_table_ctid(seed):
    universe = lexeme_universe()
    rows, _ = T.random_rows(3000, 300, seed, keys=[key for _, key in universe])
    return T.Table(rows, 1.2, 0.75, SEED32), universe


def assert_coverage_ctid(m, what):
    """assert_coverage, and what the ctid life has to meet besides (asserted by the device test as well)"""
    assert_coverage(m, what)
    c = m.cstats
    print(f"{what}: {c}")
    assert c["bulk_full"] >= 1, f"{what}: no bulkdelete that newly kills rows of both segments and names a dead row and an absent ctid"
    assert c["delete_batches"] >= 1, f"{what}: no delete_tids that matches growing rows of different inserts"
    assert 4 * c["rerank_both"] >= c["reranks"] > 0, f"{what}: {c['rerank_both']} of {c['reranks']} reranks scored on both sides"
    assert c["ineligible_sealed"] >= 1 and c["ineligible_growing"] >= 1, f"{what}: no ineligible ctid within the first k on a side"
    assert c["rerank_short"] >= 1, f"{what}: no rerank with n_ranks < k"
    assert c["rerank_cut"] >= 1, f"{what}: no rerank with n_ranks = k and more eligible candidates"


def check_delete_tids(m, tids, what):
    """Table.delete_tids against np.isin over the packed ctids of what the host readers give, before and after"""
    pl = m.page_list()
    t_keys = vb.TidSet.keys(np.array(tids, np.uint16).reshape(-1, 3))
    seg = vb.segment_from_pages(pl)   # (kept: arrays() are views into it)
    s_hit = np.isin(vb.TidSet.keys(seg.arrays()["doc_payload"]), t_keys)
    s_dead, grow = vb.sealed_deleted_from_pages(pl), vb.growing_from_pages(pl)
    g_hit, g_dead = np.isin(vb.TidSet.keys(grow["g_payload"]), t_keys), grow["g_deleted"] != 0
    got = m.delete_tids(tids, what)
    assert got == (int((s_hit & ~s_dead).sum()), int((g_hit & ~g_dead).sum()), int(g_hit.sum())), what
    pl = assert_readers_give_the_state(m, sealed=False)
    assert np.array_equal(vb.sealed_deleted_from_pages(pl), s_dead | s_hit), what
    assert np.array_equal(vb.growing_from_pages(pl)["g_deleted"] != 0, g_dead | g_hit), what
    return got


def row_score(m, seg, side, i, keys):
    """one row's `<&>` score for the sorted distinct query `keys`, computed without Table.rerank.
    Growing rows: the oracle's evaluate on (ranks, tfs) -- keys the sealed vocabulary lacks get ranks past it, which the oracle skips
    but counts into the length, a growing row's length being its tf sum.
    Sealed rows whose stored length is their tf sum (the initial rows): vbm25_evaluate on the segment read from the pages.
    Sealed rows kept by a VACUUM: THE FIELDNORM COMES FROM THE STORED LENGTH, one per posting (maintain.rs:344-362), which no evaluate
    that sums the tfs reproduces; so the per-term sum alone, ascending, with the oracle index's own doc_fieldnorm of the row.  The
    term is the operator's idf * tf (orc_idf, orc_tf: evaluate.rs), not the search's orc_cache_evaluate, which rounds differently in
    the last bit for some postings -- the two evaluates above are the operator's."""
    L, o = orc.lib(), m.oix
    _, kt, ln = (m.sealed if side == "sealed" else m.growing)[i]
    if side == "growing":
        ranked = sorted((m.rank.get(key, o.n_terms + j), kt[key]) for j, key in enumerate(sorted(kt)))
        return L.orc_score_to_f64(o.evaluate([r for r, _ in ranked], [tf for _, tf in ranked], [m.rank[key] for key in keys if key in m.rank]))
    if ln == T.length_of(kt):
        doc_keys = sorted(kt)
        return vb.evaluate(seg, doc_keys, [kt[key] for key in doc_keys], vb.Query(keys))
    s = 0.0
    for key in keys:
        if key in kt:
            s += L.orc_idf(o.n_docs, int(o.arrays["term_df"][m.rank[key]])) * \
                L.orc_tf(int(o.arrays["doc_fieldnorm"][i]), kt[key], o.k1, o.b, o.sum_len / o.n_docs)
    return s


def check_rerank(m, seg, csr, queries, lists, k, what, covered=None):
    """Table.rerank_op against row_score, a lowest-row directory made from the payload arrays and numpy's stable sort.
    The live side is put together here from the two others, without Table.rerank(side="live"): a candidate is eligible if it is on the
    sealed or the growing side; its entry is the sealed side's where there is one, else the growing side's with doc + n_sealed; the
    result is the stable descending sort of that union cut at k.  `covered`: the rows the live directory has to cover before this
    rerank, as the caller counts them (default: not checked).  Table.rerank_docs goes through row_score as well, and on the indices
    the live side resolved it gives the scores and docs of the ctid route, pos counting the eligible candidates only."""
    n_sealed, n_rows = len(m.sealed), len(m.sealed) + len(m.growing)
    keys_of = [m.keys_of(q) for q in queries]
    got = m.rerank_op(keys_of, lists, k)
    scores = {}

    def score(side, i, q):
        if (side, i, q) not in scores:
            scores[side, i, q] = row_score(m, seg, side, i, keys_of[q])
        return scores[side, i, q]

    def top(pos, doc, score):
        order = np.argsort(-np.array(score, np.float64), kind="stable")[:k]
        want = np.zeros(k, T.RANK_DTYPE)
        want["score"][:len(order)] = np.array(score, np.float64)[order]
        want["pos"][:len(order)], want["doc"][:len(order)] = np.array(pos, np.uint32)[order], np.array(doc, np.uint32)[order]
        return want, len(order)

    def same(result, q, want, what_q):
        assert result[0].shape == (len(queries), k) and result[0].dtype == T.RANK_DTYPE
        assert result[1][q] == want[1], f"{what} {what_q} query {q}: {result[1][q]} ranks for {want[1]}"
        assert result[0][q].tobytes() == want[0].tobytes(), f"{what} {what_q} query {q}: {result[0][q][:4]} for {want[0][:4]}"

    lowest, c_keys, entry = {}, [vb.TidSet.keys(np.array(tids, np.uint16).reshape(-1, 3)).tolist() for tids in lists], {}
    for side, rows in (("sealed", m.sealed), ("growing", m.growing)):
        p_keys = vb.TidSet.keys(np.array([p for p, _, _ in rows], np.uint16).reshape(-1, 3)).tolist()
        lowest[side] = {key: i for i, key in reversed(list(enumerate(p_keys)))}
        for q in range(len(queries)):
            entry[side, q] = {j: (lowest[side][key], score(side, lowest[side][key], q)) for j, key in enumerate(c_keys[q]) if key in lowest[side]}
            pos = sorted(entry[side, q])
            same(got[side], q, top(pos, [entry[side, q][j][0] for j in pos], [entry[side, q][j][1] for j in pos]), side)

    def live_entries(q, limit):
        """{pos: (live doc, score)}: the sealed side's entry, else the growing side's over the first `limit` rows"""
        union = {j: (g + n_sealed, s) for j, (g, s) in entry["growing", q].items() if g + n_sealed < limit}
        union.update(entry["sealed", q])
        return union

    if n_sealed and covered is not None:
        assert got["live_covered"] == covered, f"{what}: the live directory covers {got['live_covered']} rows, the caller counts {covered}"
    assert (got["live_before"] is not None) == bool(n_sealed and got["live_covered"] != n_rows), what
    for q in range(len(queries)):
        for name, limit in (("live", n_rows),) + ((("live_before", got["live_covered"]),) if got["live_before"] is not None else ()):
            union = live_entries(q, limit)
            assert name != "live" or set(union) == set(entry["sealed", q]) | set(entry["growing", q]), what
            pos = sorted(union)
            same(got[name], q, top(pos, [union[j][0] for j in pos], [union[j][1] for j in pos]), name)
        # the cand_doc route: the same scores and docs, pos among the eligible candidates
        union = live_entries(q, n_rows)
        pos = sorted(union)
        assert got["live_docs"][q].dtype == np.uint32 and got["live_docs"][q].tolist() == [union[j][0] for j in pos], what
        by_doc, n = got["live_by_doc"][0][q], got["live_by_doc"][1][q]
        assert n == got["live"][1][q], what
        assert by_doc["score"].tobytes() == got["live"][0]["score"][q].tobytes() and by_doc["doc"].tobytes() == got["live"][0]["doc"][q].tobytes(), what
        assert np.array_equal(np.array(pos, np.uint32)[by_doc["pos"][:n]], got["live"][0]["pos"][q, :n]), what
        direct = m.rerank_docs(keys_of[q], got["live_docs"][q], k)
        assert direct[0].tobytes() == by_doc.tobytes() and direct[1] == n and direct[2] == len(pos), what
    if got["hits"] is not None:   # the search's records as document indices of the live handle, reranked by index
        for q, hits in enumerate(got["hits"]):
            shown = library_select(m, seg, csr, keys_of[q], T.HITS_K, None)["doc_id"].astype(np.int64)
            assert hits.dtype == np.uint32 and hits.tolist() == np.where(shown >= n_sealed, n_sealed + (T.NONE - shown), shown).tolist(), what
            assert not any(m.growing_deleted[int(i) - n_sealed] for i in hits if i >= n_sealed), what
            score_q = [score("sealed", int(i), q) if i < n_sealed else score("growing", int(i) - n_sealed, q) for i in hits]
            same(got["hits_by_doc"], q, top(range(len(hits)), hits, score_q), "search hits")
    return got


def check_forward_live(m, what):
    """Table.forward_live against forward() and the growing rows as the host reader of the pages gives them, bound by hand: the ranks
    of the keys that the sealed vocabulary holds, ascending (keys ascend in a row, and so do their ranks), the tape's own fieldnorm"""
    grow = vb.growing_from_pages(m.page_list())
    g_keys = [bytes(key) for key in np.asarray(grow["g_key"], np.uint8).reshape(-1, 16)]
    known = np.array([key in m.rank for key in g_keys], bool)
    for drop in (False, True):
        start, term, tf, fn = m.forward_live(drop_deleted=drop)
        s_start, s_term, s_tf, s_fn = m.forward()
        n_s, nk_s = len(m.sealed), len(s_term)
        for got, want, name in ((start[:n_s + 1], s_start, "start"), (term[:nk_s], s_term, "term"), (tf[:nk_s], s_tf, "tf"), (fn[:n_s], s_fn, "fieldnorm")):
            assert got.dtype == want.dtype and np.array_equal(got, want), f"{what}: forward_live's sealed {name}"
        keep = known & ~np.repeat(grow["g_deleted"] != 0, np.diff(grow["g_start"]).astype(np.int64)) if drop else known
        runs = [int(keep[int(a):int(b)].sum()) for a, b in zip(grow["g_start"][:-1], grow["g_start"][1:])]
        assert np.array_equal(start[n_s:], nk_s + np.r_[0, np.cumsum(runs)].astype(np.uint64)), f"{what}: forward_live's growing start"
        assert np.array_equal(term[nk_s:], np.array([m.rank[key] for key, kept in zip(g_keys, keep) if kept], np.uint32)), f"{what}: growing terms"
        assert np.array_equal(tf[nk_s:], np.asarray(grow["g_tf"], np.uint32)[keep]), f"{what}: forward_live's growing tf"
        assert np.array_equal(fn[n_s:], grow["g_fieldnorm"]) and all(a.dtype == b.dtype for a, b in zip((start, term, tf, fn), m.forward())), what
        assert all(np.all(np.diff(term[int(a):int(b)].astype(np.int64)) > 0) for a, b in zip(start[:-1], start[1:])), f"{what}: a run does not ascend"


def append_in_handles(m, n_rows):
    """one INSERT statement of n_rows rows, already in the model, reported as the ctid lives append it: handles of at most CAST_DOCS"""
    for lo in range(0, n_rows, T.CAST_DOCS):
        m.live_append(min(T.CAST_DOCS, n_rows - lo))


def assert_coverage_live(m, what):
    """what a life on the live rerank stack (tests/test_gpu_table_live_fuzz.py) has to meet, each at least once"""
    c = m.cstats
    print(f"{what}: {c}")
    assert c["live_both"] >= 1, f"{what}: no live result with a sealed and a growing document both scoring non-zero"
    assert c["live_shared"] >= 1, f"{what}: no ctid of a sealed and a growing row named on the live ring"
    assert c["sync_multi"] >= 1, f"{what}: no sync whose delta came from two appends or more"
    assert c["sync_one"] >= 1, f"{what}: no sync of exactly one row"
    assert c["ab_differ"] >= 1, f"{what}: no batch that the sync changed"
    assert c["unknown_handle"] >= 1, f"{what}: no appended handle in which every document had no known element"
    assert c["live_short"] >= 1 and c["live_cut"] >= 1, f"{what}: no live rerank with n_ranks < k, or none cut at k"
    assert c["live_hits"] >= 1, f"{what}: no rerank of search hits with a growing document among them while a growing row is deleted"


# chosen for assert_coverage_ctid and assert_coverage_live together: of the seeds 1 .. 32 these are 4, 6, 15, 26 and 29 (seed 1 appends no
# handle of only unknown lexemes); 6, 15 and 26 run 19 to 24 VACUUMs, these two 14 and 15 like SEEDS_CTID's
SEEDS_LIVE = (4, 29)


@pytest.mark.parametrize("seed", sorted(set(SEEDS_CTID + SEEDS_LIVE)))
def test_model_along_a_ctid_life(seed):
    m, universe = new_table_ctid(seed)
    assert_readers_give_the_state(m)
    seg = csr = None
    dead = set()   # the ctids the epoch's deletes have named
    covered = len(m.sealed)   # the rows the live ctid directory covers: those of the epoch's last rerank, or the sealed ones
    for n_op, op in enumerate(m.ops_ctid(seed, N_OPS, universe)):
        what = f"seed {seed} operation {n_op} {op[0]}"
        if op[0] in ("insert", "delete_tids"):   # (after the last one: a row is dead exactly when its ctid has been named)
            assert [p in dead for p, _, _ in m.sealed] == m.sealed_deleted.tolist(), what
            assert [p in dead for p, _, _ in m.growing] == m.growing_deleted, what
        if seg is None and op[0] in ("select", "rerank"):
            pl = m.page_list()
            seg, csr = vb.segment_from_pages(pl), vb.growing_from_pages(pl)
        if op[0] == "insert":
            batch = m.new_batch()
            for payload, lexrow in op[1]:
                kt = {}
                for lexeme, count in lexrow:   # the cast, with the host intern
                    kt[vb.intern(lexeme, SEED32)] = kt.get(vb.intern(lexeme, SEED32), 0) + count
                assert m.cast(lexrow) == kt, what
                m.insert(payload, kt, batch)
            append_in_handles(m, len(op[1]))
            assert_readers_give_the_state(m, sealed=False)
            seg = None
        elif op[0] == "delete_tids":
            check_delete_tids(m, op[1], "delete")
            dead |= {tuple(t) for t in op[1]}
            seg = None
        elif op[0] == "reopen":
            assert_readers_give_the_state(m)
            check_forward_live(m, what)
        elif op[0] == "vacuum":
            check_delete_tids(m, op[1], "bulkdelete")
            check_forward_live(m, what)
            check_vacuum(m)
            dead.clear()
            covered = len(m.sealed)
            seg = None
        elif op[0] == "select":
            _, queries, selectors, k, _ = op
            for lexemes, sel in zip(queries, selectors):
                keys = m.keys_of(lexemes)
                assert keys == sorted({vb.intern(t, SEED32) for t in lexemes}), what
                keep = m.keep_of(sel)
                assert_bit_exact(library_select(m, seg, csr, keys, k, keep), m.select(keys, k, keep), f"{what} k={k} selector {sel}")
        else:
            _, queries, lists, k = op
            check_rerank(m, seg, csr, queries, lists, k, f"{what} k={k}", covered)
            covered = len(m.sealed) + len(m.growing) if m.sealed else covered
    assert_coverage_ctid(m, f"seed {seed}")
    if seed in SEEDS_LIVE:
        assert_coverage_live(m, f"seed {seed}")


def test_model_through_the_empty_table():
    """everything deleted and vacuumed away, two inserts that cannot score, a vacuum that seals them"""
    rows, universe = T.random_rows(700, 60, 9)
    m = T.Table(rows, 1.2, 0.75, SEED32)
    for d in range(700):
        m.delete_sealed(d)
    check_vacuum(m)
    assert m.oix.n_docs == 0 and len(m.page_list()) == 10
    m.insert((1, 2, 3), {universe[1]: 2, universe[2]: 1})
    m.insert((4, 5, 6), {universe[2]: 5})
    append_in_handles(m, 2)
    assert_readers_give_the_state(m)
    assert len(m.select([universe[2]], 10)) == 0
    # the live side without a sealed row: two documents with empty runs (the vocabulary is empty) and their own codes; every score is
    # 0.0, no directory exists that a sync could bring up, and the handle of both rows held no known element
    check_forward_live(m, "the empty table")
    start, term, _, fn = m.forward_live()
    assert start.tolist() == [0, 0, 0] and len(term) == 0 and len(fn) == 2 and m.cstats["unknown_handle"] == 1
    got = m.rerank_op([[universe[2]]], [[(4, 5, 6), (9, 9, 9), (1, 2, 3)]], 10)
    assert got["live_before"] is None and got["hits"] is None and got["live"][1].tolist() == [2]
    assert got["live"][0][0, :2].tolist() == [(0.0, 0, 1), (0.0, 2, 0)] and got["live_docs"][0].tolist() == [1, 0]
    assert got["live_by_doc"][0][0, :2].tolist() == [(0.0, 0, 1), (0.0, 1, 0)]
    check_vacuum(m)
    check_forward_live(m, "the two rows sealed")
    got = m.rerank_op([[universe[2]]], [[(4, 5, 6), (9, 9, 9), (1, 2, 3)]], 10)
    assert got["live_before"] is None and got["live"][0]["doc"][0, :2].tolist() == got["sealed"][0]["doc"][0, :2].tolist()
    assert got["live"][0].tobytes() == got["sealed"][0].tobytes() and (got["live"][0]["score"][0, :2] > 0).all()
    got = m.select([universe[2]], 10)
    assert got["doc_id"].tolist() == [1, 0] or got["doc_id"].tolist() == [0, 1]
    assert len(got) == 2 and np.all(got["score"] > 0)
