"""The reference's tests/fuzz on the device lifecycle: one table's long-lived handles (index, growing segment, filter, resident
batch, ring) carried through random INSERT, SELECT, DELETE and VACUUM as INTEGRATION.md sections 2b to 2b'' string them together, every
answer compared with tests/table_model.py -- a model of the table's rows that shares no code with the library (checked against the
library's host side by tests/test_table_model.py).  Records are compared bit for bit: the model and the device rank ties by the same
documented rule.

The resident batch and the ring have their k fixed per epoch (the time between two VACUUMs): epoch e uses KS[e % 5]
(table_model.Table.epoch_k), so every k is served by every front end over a life; vbm25_search_batch_growing_filtered takes the k
each SELECT draws.

Measured on an MI355X: test_random_life 1.7 to 2.0 s per seed (160 operations, 11 to 16 VACUUMs, about 500 selects),
test_scripted_corners and test_bulk_insert_across_a_tile 0.8 s each."""
import time

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
import table_model as T
import vectors_device_data as V
from pages_write_data import assert_same_pages
from parity import assert_bit_exact
from test_segment_builder import assert_same_index as assert_same_arrays
from test_table_model import N_OPS, SEED32, SEEDS, assert_coverage, new_table

pytestmark = pytest.mark.gpu
NONE = T.NONE
GT = 8192   # growing documents per tile (csrc/growing.h)


def assert_same_index(seg, oix):
    """a downloaded segment against the oracle's index, array for array; the empty index by its counts (no array has an element but
    the two offset arrays' leading 0)"""
    if oix.n_docs or oix.n_terms:
        return assert_same_arrays(seg, oix)
    assert (seg.n_docs, seg.n_terms, seg.n_blocks, seg.desc.sum_len, seg.desc.blob_bytes) == (0, 0, 0, 0, 0)
    assert (seg.desc.k1, seg.desc.b) == (oix.k1, oix.b)


def packed(bits):
    return vb.DocFilter.pack(np.asarray(bits, bool), len(bits))[0]


class Life:
    """the model next to the device state a serving process holds for the same table"""

    def __init__(self, model):
        self.m = model
        self.epoch = 0
        pl = model.page_list()
        self.gix = vb.GpuIndex(vb.DeviceSegment.from_pages(pl))
        self.grow = vb.GrowingSegment.from_pages(self.gix, pl)
        self.filt = vb.DocFilter(self.gix, self.keeps(0))
        self.filt.set_growing(self.grow, self.keeps(1))
        self.attach()
        self.last = ([[key] for key in model.vocab[:8]], [(NONE, 0, 1)[q % 3] for q in range(8)])

    def keeps(self, half):
        """the two keep predicates over the sealed (half 0) or the growing (half 1) rows: bool [2, n]"""
        return np.stack([self.m.alive()[half], self.m.tenant()[half]])

    def attach(self):
        self.k = self.m.epoch_k()
        self.batch = vb.Batch(self.gix, 16, 256, self.k)
        self.batch.set_growing(self.grow)
        self.ring = vb.Stream(self.gix, 2, 16, 256, self.k)
        self.ring.set_growing(self.grow)
        self.ring.set_filter(self.filt)

    # ---- INSERT, DELETE

    def insert(self, payload, kt):
        self.insert_many([(payload, kt)])

    def insert_many(self, docs):
        """one append of all `docs`, the growing bitmaps extended in the same step"""
        lo = len(self.m.growing)
        for payload, kt in docs:
            self.m.insert(payload, kt)
        G = self.m.growing_csr(lo)
        self.grow.append(G["g_start"], G["g_key"], G["g_tf"], G["g_fieldnorm"], G["g_payload"])
        self.filt.extend_growing(self.grow, self.keeps(1)[:, lo:])
        assert self.grow.n_docs == len(self.m.growing)

    def delete(self, where, ids):
        if where == "sealed":
            for d in ids:
                self.m.delete_sealed(d)
            if ids:
                self.filt.update(0, self.keeps(0)[0])
                self.filt.update(1, self.keeps(0)[1])
        else:
            for g in ids:
                self.m.delete_growing(g)
            if ids:
                self.grow.delete(ids)
                # (the tenant bitmap implies `alive`; the segment's own deleted flags hide the rows under every selector)

    # ---- SELECT

    @staticmethod
    def csr(gix, queries):
        ids = [gix.lookup_terms(list(q)) for q in queries]
        ids = [np.sort(t[t != NONE]) for t in ids]
        return np.concatenate(ids).astype(np.uint32), np.r_[0, np.cumsum([len(t) for t in ids])].astype(np.uint32)

    def ask(self, front, queries, selectors, k):
        """(hits, n_hits, the k served) of one front end of the long-lived handles"""
        terms, off = self.csr(self.gix, queries)
        sel = np.array(selectors, np.uint32)
        if front == 0:
            return vb.search_batch_growing_masked(self.gix, self.grow, terms, off, k, self.filt, sel) + (k,)
        if front == 1:
            self.batch.set_filter(self.filt, sel)
            self.batch.set_queries(terms, off)
            self.batch.run()
            return self.batch.fetch() + (self.k,)
        self.ring.submit(terms, off, q_filter=sel)
        assert self.ring.in_flight == 1
        return self.ring.collect() + (self.k,)   # (collected before the next mutation)

    def select(self, queries, selectors, k, front, count=True):
        hits, n_hits, k = self.ask(front, queries, selectors, k)
        for q, (keys, sel) in enumerate(zip(queries, selectors)):
            want = self.m.select(keys, k, self.m.keep_of(sel), count=count)
            what = f"epoch {self.epoch} front end {front} k={k} selector {sel} query {q}"
            assert n_hits[q] == len(want), f"{what}: {n_hits[q]} records, the model has {len(want)}"
            assert_bit_exact(want, hits[q, :n_hits[q]], what)
        self.last = (queries, selectors)

    # ---- REOPEN: the incremental state is the relation's state

    def reopen(self):
        pl = self.m.page_list()
        ds = vb.DeviceSegment.from_pages(pl)
        assert_same_index(ds.download(), self.m.oix)
        gix = vb.GpuIndex(ds)
        grow, csr = vb.GrowingSegment.from_pages(gix, pl, return_csr=True)
        V.assert_same_csr(csr, self.m.growing_csr(), f"epoch {self.epoch}: the vectors tape")
        alive_s = ~vb.sealed_deleted_from_pages(pl)
        alive_g = csr["g_deleted"] == 0
        filt = vb.DocFilter(gix, np.stack([alive_s, alive_s & self.m.tenant_bits(self.m.sealed)]))
        filt.set_growing(grow, np.stack([alive_g, alive_g & (csr["g_payload"].reshape(-1, 3)[:, 2] % 3 == 0)]))
        queries, selectors = self.last
        terms, off = self.csr(gix, queries)
        hits, n_hits = vb.search_batch_growing_masked(gix, grow, terms, off, 300, filt, np.array(selectors, np.uint32))
        held, n_held, _ = self.ask(0, queries, selectors, 300)
        assert n_hits.tobytes() == n_held.tobytes(), f"epoch {self.epoch}: the reopened relation and the long-lived handles count differently"
        for q in range(len(queries)):
            assert hits[q, :n_hits[q]].tobytes() == held[q, :n_hits[q]].tobytes(), \
                f"epoch {self.epoch}: the reopened relation and the long-lived handles answer query {q} differently"

    # ---- VACUUM

    def vacuum(self, seed32=SEED32, dv=None):
        """dv: the compaction inputs of the relation as it is now, where the caller holds them already (default: read from the pages)"""
        self.reopen()
        m = self.m
        pl = m.page_list()
        if dv is None:
            dv = vb.DeviceVacuum.from_pages(self.gix, pl)
        assert (dv.n_sealed, dv.n_sealed_deleted, dv.n_grow, dv.n_grow_deleted, dv.n_elements) == m.counts()
        ds, relabel = vb.DeviceSegment.maintain_device(self.gix, dv, return_relabel=True)
        want_relabel = m.vacuum()
        assert np.array_equal(relabel, want_relabel), f"epoch {self.epoch}: relabel"
        assert_same_index(ds.download(), m.oix)
        written = ds.to_relation(seed32)
        assert_same_pages(written, m.page_list(), f"epoch {self.epoch}: the written relation")
        gix = vb.GpuIndex(ds)
        filt = self.filt.remap_device(gix, dv)
        for i in (0, 1):   # the payload travels with the row: the predicate over the new rows
            assert np.array_equal(filt.read(i), packed(self.keeps(0)[i])), f"epoch {self.epoch}: remapped bitmap {i}"
        queries, selectors = self.last
        terms, off = self.csr(gix, queries)
        hits, n_hits = vb.MultiIndex.from_device(ds, [0, 0]).search_batch(terms, off, 300)
        for q, keys in enumerate(queries):
            assert_bit_exact(m.select(keys, 300, None, count=False), hits[q, :n_hits[q]], f"epoch {self.epoch}: replicas, query {q}")
        # the next epoch's handles, made from the WRITTEN relation; the old ones go after the new ones have served a select
        old = (self.gix, self.grow, self.filt, self.batch, self.ring, dv)
        self.epoch += 1
        self.gix, self.filt = gix, filt
        self.grow = vb.GrowingSegment.from_pages(gix, written)
        assert self.grow.n_docs == 0
        self.filt.set_growing(self.grow)
        self.attach()
        for front in (0, 1, 2):
            self.select(queries, selectors, 300, front, count=False)
        del old

    def run(self, op):
        if op[0] == "insert":
            for payload, kt in op[1]:
                self.insert(payload, kt)
        elif op[0] == "delete":
            self.delete(op[1], op[2])
        elif op[0] == "select":
            assert op[4] == 0 or op[3] == self.k   # (the k the sequence counts on is the k the resident front ends serve)
            self.select(*op[1:])
        elif op[0] == "reopen":
            self.reopen()
        else:
            self.vacuum()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_life(seed):
    t0 = time.time()
    m, universe = new_table(seed)
    life = Life(m)
    for op in m.ops(seed, N_OPS, universe):
        life.run(op)
    life.reopen()
    assert_coverage(m, f"seed {seed}")
    print(f"seed {seed}: {time.time() - t0:.1f} s")


def test_scripted_corners():
    """what chance may not give, in one sequence; 700 rows: the documents tape crosses one page (680 tuples)"""
    rows, universe = T.random_rows(700, 300, 5)
    m = T.Table(rows, 1.2, 0.75, SEED32)
    life = Life(m)
    sel = [(NONE, 0, 1)[q % 3] for q in range(8)]

    def selects(queries, ks=(10, 300)):
        queries = (queries * 8)[:8]
        for front, k in [(f, k) for f in (0, 1, 2) for k in ks]:
            life.select(queries, sel, k, front)

    # a growing copy of a sealed row: the same keys, term frequencies and length, hence the same score bits -- a tie across the
    # segments, sealed first
    twin = max(range(700), key=lambda d: (rows[d][0][2] % 3 == 0, -len(rows[d][1])))
    rare = sorted(rows[twin][1], key=lambda key: sum(key in kt for _, kt, _ in rows))[:2]
    life.insert((7, 7, rows[twin][0][2]), rows[twin][1])
    selects([sorted(rare), [rare[0]]])
    assert m.stats["mixed_ties"] > 0, "no tie group mixed a sealed and a growing record"
    life.delete("growing", [0])
    # a VACUUM of one deleted growing row and nothing else, then two with nothing to do
    for _ in range(3):
        life.vacuum()
        selects([[universe[3], universe[40]], [universe[100]]])
    assert m.vacuums[-2:] == [(0, 0, 0), (0, 0, 0)] and len(m.sealed) == 700
    # only sealed deletes (the same rows twice), across the page boundary of the documents tape
    for _ in range(2):
        life.delete("sealed", [0, 63, 64, 65, 679, 680, 699])
    selects([[universe[0], universe[1]]])
    life.vacuum()
    assert m.vacuums[-1] == (7, 0, 0)
    # only inserts, one of them with keys that are all unknown, one without keys
    life.insert((1, 2, 3), {universe[5]: 2, universe[200]: 1, universe[250]: 3})
    life.insert((1, 2, 4), {T.new_key(1): 1, T.new_key(2): 4})
    life.insert((1, 2, 6), {})
    selects([[universe[5], universe[250]], [T.new_key(1), T.new_key(2)], [T.new_key(2), universe[250]]])
    life.vacuum()
    assert m.vacuums[-1] == (0, 0, 2) and len(m.sealed) == 696
    selects([[T.new_key(1), T.new_key(2)], [T.new_key(2), universe[250]]])
    # a growing row deleted twice
    life.insert((9, 9, 9), {universe[7]: 1})
    life.insert((9, 9, 12), {universe[7]: 2})
    for _ in range(2):
        life.delete("growing", [1])
    selects([[universe[7]]], ks=(1025,))
    # every posting of three tokens deleted: they vanish from the vocabulary; one of them comes back with an insert
    df = {key: [d for d, (_, kt, _) in enumerate(m.sealed) if key in kt] for key in m.vocab}
    gone = sorted((key for key in m.vocab if key not in (universe[7],)), key=lambda key: len(df[key]))[:3]
    life.delete("sealed", sorted({d for key in gone for d in df[key]}))
    life.vacuum()
    assert not set(gone) & set(m.vocab)
    life.insert((3, 3, 3), {gone[0]: 2, universe[0]: 1})
    selects([[gone[0]], [gone[0], gone[1], universe[0]]])
    life.vacuum()
    assert gone[0] in m.vocab and gone[1] not in m.vocab
    selects([[gone[0]], [gone[0], gone[1], universe[0]]])
    # everything deleted: the empty table; rows inserted into it score nothing until a VACUUM seals them
    life.insert((4, 4, 4), {universe[1]: 1})
    life.delete("sealed", list(range(len(m.sealed))))
    life.delete("growing", [0])
    selects([[universe[0], universe[1]]])
    life.vacuum()
    assert len(m.sealed) == 0 and len(m.page_list()) == 10
    before = dict(m.stats)
    selects([[universe[0], universe[1]]])
    life.insert((5, 5, 6), {universe[1]: 2, universe[2]: 1})
    life.insert((5, 5, 7), {universe[2]: 5})
    selects([[universe[2]], [universe[1], universe[2]]])
    assert m.stats["nothing"] - before["nothing"] == m.stats["selects"] - before["selects"] == 96
    life.vacuum()
    assert len(m.sealed) == 2
    before = dict(m.stats)
    selects([[universe[2]], [universe[1], universe[2]]])
    assert m.stats["nothing"] == before["nothing"]
    life.reopen()


def test_bulk_insert_across_a_tile():
    """one append past a growing tile (GT documents), deletes on both sides of the tile boundary, two VACUUMs"""
    rows, universe = T.random_rows(1000, 300, 6)
    m = T.Table(rows, 1.2, 0.75, SEED32)
    life = Life(m)
    rng = np.random.default_rng(6)

    def doc(i):
        keys = [universe[j] for j in rng.choice(300, int(rng.integers(3, 7)), replace=False)]
        if i % 50 == 0:
            keys[0] = T.new_key(i)
        return tuple(int(x) for x in rng.integers(0, 65536, 3)), {key: int(tf) for key, tf in zip(keys, rng.integers(1, 9, len(keys)))}

    life.insert_many([doc(i) for i in range(8300)])
    assert life.grow.n_docs == 8300 > GT
    life.delete("growing", sorted({GT - 1, GT, 0, 8299} | {int(g) for g in rng.choice(8300, 196, replace=False)}))
    sel = [(NONE, 0, 1)[q % 3] for q in range(8)]
    n_selects = 0

    def selects():
        nonlocal n_selects
        for front in (0, 1, 2):
            for k in (10, 1025):
                queries = [sorted({universe[j] for j in rng.choice(300, int(rng.integers(1, 4)))}) for _ in range(8)]
                life.select(queries, sel, k, front)
                n_selects += 1

    selects()
    assert m.stats["both"] > 0
    life.reopen()
    life.vacuum()
    assert m.vacuums[-1][1] >= 196 and m.vacuums[-1][2] > 100
    selects()
    life.insert_many([doc(i + 8300) for i in range(100)])
    life.delete("sealed", [int(d) for d in rng.choice(len(m.sealed), 300, replace=False)])
    selects()
    life.vacuum()
    selects()
