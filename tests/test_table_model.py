"""tests/table_model.py against the library's host side, along the operation sequences tests/test_gpu_table_fuzz.py runs on the
device: the host readers of the model's pages give the model's state, its SELECT is vbm25_merge_hits(the oracle's brute-force
ranking, vbm25_growing_search) bit for bit, and its VACUUM is tests/maintain_model.py put through the host builder.  Also the
coverage conditions of the chosen seeds, on the model alone.  No GPU use."""
import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import maintain_model
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
