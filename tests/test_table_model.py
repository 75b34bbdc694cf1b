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


def check_rerank(m, seg, queries, lists, k, what):
    """Table.rerank_op against row_score, a lowest-row directory made from the payload arrays and numpy's stable sort"""
    got = m.rerank_op([m.keys_of(q) for q in queries], lists, k)
    for side, rows in (("sealed", m.sealed), ("growing", m.growing)):
        p_keys = vb.TidSet.keys(np.array([p for p, _, _ in rows], np.uint16).reshape(-1, 3)).tolist()
        lowest = {key: i for i, key in reversed(list(enumerate(p_keys)))}
        ranks, n_ranks = got[side]
        assert ranks.shape == (len(queries), k) and ranks.dtype == T.RANK_DTYPE
        for q, (lexemes, tids) in enumerate(zip(queries, lists)):
            c_keys = vb.TidSet.keys(np.array(tids, np.uint16).reshape(-1, 3)).tolist()
            pos = np.array([j for j, key in enumerate(c_keys) if key in lowest], np.uint32)
            doc = np.array([lowest[c_keys[j]] for j in pos], np.uint32)
            score = np.array([row_score(m, seg, side, int(i), m.keys_of(lexemes)) for i in doc], np.float64)
            order = np.argsort(-score, kind="stable")[:k]
            want = np.zeros(k, T.RANK_DTYPE)
            want["score"][:len(order)], want["pos"][:len(order)], want["doc"][:len(order)] = score[order], pos[order], doc[order]
            assert n_ranks[q] == len(order), f"{what} {side} query {q}"
            assert ranks[q].tobytes() == want.tobytes(), f"{what} {side} query {q}: {ranks[q][:4]} for {want[:4]}"


@pytest.mark.parametrize("seed", SEEDS_CTID)
def test_model_along_a_ctid_life(seed):
    m, universe = new_table_ctid(seed)
    assert_readers_give_the_state(m)
    seg = csr = None
    dead = set()   # the ctids the epoch's deletes have named
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
            assert_readers_give_the_state(m, sealed=False)
            seg = None
        elif op[0] == "delete_tids":
            check_delete_tids(m, op[1], "delete")
            dead |= {tuple(t) for t in op[1]}
            seg = None
        elif op[0] == "reopen":
            assert_readers_give_the_state(m)
        elif op[0] == "vacuum":
            check_delete_tids(m, op[1], "bulkdelete")
            check_vacuum(m)
            dead.clear()
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
            check_rerank(m, seg, queries, lists, k, f"{what} k={k}")
    assert_coverage_ctid(m, f"seed {seed}")


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
    assert_readers_give_the_state(m)
    assert len(m.select([universe[2]], 10)) == 0
    check_vacuum(m)
    got = m.select([universe[2]], 10)
    assert got["doc_id"].tolist() == [1, 0] or got["doc_id"].tolist() == [0, 1]
    assert len(got) == 2 and np.all(got["score"] > 0)
