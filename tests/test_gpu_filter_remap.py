"""vbm25_filter_remap and vbm25_filter_read: a filter carried across vbm25_index_maintain on the device.  The words of the remapped
filter, read back, are byte for byte those of the numpy model (tests/filter_remap_model.py: the kept sealed bits, then the live
growing bits); searches through it are byte-identical to searches through a filter created on the new index from the model's
bits; refusals leave nothing behind and the old filter serving.  -m gpu only."""
import ctypes as C

import numpy as np
import pytest

import vectorchord_bm25_amd as vb
from corpus import make_corpus
from filter_remap_model import deletion_patterns, remap_bits, remap_words
from growing_data import make_growing
from test_gpu_growing_append import docs

pytestmark = pytest.mark.gpu
NONE = vb.NO_FILTER
INVALID, UNSUPPORTED = -1, -4
G_MAX = 3000

_C = {}


def setup(n):
    """n sealed documents (the lognormal corpus of tests/test_gpu_maintain.py at 20 000), their index, G_MAX growing documents"""
    if n not in _C:
        if n >= 1000:
            c = make_corpus(n, 600, seed=1, length="lognormal", mean_len=40)
        else:
            c = make_corpus(n, 50, seed=n, length="lognormal", mean_len=12)
        seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
        G, _ = make_growing(seg.arrays()["term_key"], 5000, seed=8, deleted=None)
        _C[n] = (seg, vb.GpuIndex(seg), G)
    return _C[n]


def grow_flags(g, how, rng):
    if how == "all":
        return np.ones(g, np.uint8)
    return (rng.random(g) < how).astype(np.uint8)


def old_filter(gix, n, G, g, F, rng):
    """a filter of F random bitmaps on gix and, for g > 0, on an upload of G's first g documents"""
    bits_s = rng.random((F, n)) < 0.5
    f = vb.DocFilter(gix, bits_s)
    gs, bits_g = None, None
    if g:
        gs = vb.GrowingSegment(gix, **docs(G, 0, g))
        bits_g = rng.random((F, g)) < 0.5
        f.set_growing(gs, bits_g)
    return f, gs, bits_s, bits_g


def compact_remap_check(gix, n, G, deleted, g, gdel, F, rng, what):
    """maintain -> GpuIndex -> remap -> read: the words equal the model's; the old filter reads back unchanged"""
    f, gs, bits_s, bits_g = old_filter(gix, n, G, g, F, rng)
    grow = None
    if g:
        grow = docs(G, 0, g)
        grow["g_deleted"] = gdel
    ds = vb.DeviceSegment.maintain(gix, deleted, grow)
    nix = vb.GpuIndex(ds)
    want = remap_words(bits_s, deleted, bits_g, gdel)
    assert nix.n_docs == int((~deleted).sum()) + (int((gdel == 0).sum()) if g else 0), what
    nf = f.remap(nix, deleted, gdel if g else None)
    assert nf.n_bitmaps == F and want.shape == (F, (nix.n_docs + 63) // 64)
    for i in range(F):
        got = nf.read(i)
        assert got.tobytes() == want[i].tobytes(), f"{what}: bitmap {i} differs at words {np.flatnonzero(got != want[i])[:8]}"
    with pytest.raises(vb.Vbm25Error) as e:  # the new filter has no growing bitmaps
        nf.read(0, growing=True)
    assert e.value.code == INVALID
    old_s, old_g = vb.DocFilter.pack(bits_s, n), (vb.DocFilter.pack(bits_g, g) if g else None)
    for i in range(F):
        assert f.read(i).tobytes() == old_s[i].tobytes(), f"{what}: the old filter's bitmap {i} changed"
        if g:
            assert f.read(i, growing=True).tobytes() == old_g[i].tobytes(), f"{what}: the old filter's growing bitmap {i} changed"
    return nf, nix, ds


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 1000, 20_000])
def test_words_byte_for_byte(n):
    """every deletion pattern (growing count, growing deletes and F in rotation), then every growing count x growing delete rate under
    the half-deleted pattern"""
    seg, gix, G = setup(n)
    rng = np.random.default_rng(1000 + n)
    gs_, gd_, fs_ = (0, 1, 63, 64, 65, G_MAX), (0.0, 0.1, "all"), (1, 3, 17)
    pats = deletion_patterns(n, rng)
    cases = [(name, gs_[(i + 1) % 6], gd_[i % 3], fs_[i % 3]) for i, name in enumerate(pats)]
    cases += [("random_0.5", g, gd, fs_[(i + j) % 3]) for i, g in enumerate(gs_) for j, gd in enumerate(gd_)]
    assert {c[0] for c in cases} >= {"none", "all_but_first", "all_but_last", "every_other", "range", "random_0.01", "random_0.5",
                                     "random_0.99"}
    for name, g, gd, F in cases:
        deleted = pats[name]
        if name == "range" and n >= 1000:  # at least three whole words emptied
            assert deleted[:n // 64 * 64].reshape(-1, 64).all(axis=1).sum() >= 3
        gdel = grow_flags(g, gd, rng)
        compact_remap_check(gix, n, G, deleted, g, gdel, F, rng, f"n={n} {name} G={g} gdel={gd} F={F}")


@pytest.mark.parametrize("rem", [0, 1, 31, 63])
def test_growing_run_starts_at_every_kind_of_bit(rem):
    """n_kept % 64 = 0, 1, 31, 63: the growing run starts aligned, one bit in, in the middle and one bit short of a word"""
    n = 1000
    seg, gix, G = setup(n)
    rng = np.random.default_rng(rem)
    for g, gd in ((1, 0.0), (65, 0.1), (300, 0.1), (64, 0.0)):
        n_kept = 640 + rem
        deleted = np.zeros(n, bool)
        deleted[rng.choice(n, n - n_kept, replace=False)] = True
        gdel = grow_flags(g, gd, rng)
        nf, nix, _ = compact_remap_check(gix, n, G, deleted, g, gdel, 3, rng, f"n_kept % 64 = {rem} G={g}")
        assert (nix.n_docs - int((gdel == 0).sum())) % 64 == rem


def queries(n_terms, nq, nt, seed):
    rng = np.random.default_rng(seed)
    terms = np.sort(np.stack([rng.choice(n_terms, nt, replace=False) for _ in range(nq)]), axis=1).reshape(-1).astype(np.uint32)
    return terms, (np.arange(nq + 1) * nt).astype(np.uint32)


def test_through_a_search():
    n, g = 20_000, 5000
    seg, gix, G = setup(n)
    rng = np.random.default_rng(7)
    deleted = rng.random(n) < 0.05
    gdel = (rng.random(g) < 0.1).astype(np.uint8)
    # a random half, one contiguous tenant that reaches into the growing documents, a single document
    bits = np.zeros((3, n + g), bool)
    bits[0] = rng.random(n + g) < 0.5
    bits[1, n - 3000: n + 1000] = True
    single = int(np.flatnonzero(~deleted)[1234])
    bits[2, single] = True
    f = vb.DocFilter(gix, bits[:, :n])
    gs = vb.GrowingSegment(gix, **docs(G, 0, g))
    f.set_growing(gs, bits[:, n:])
    grow = docs(G, 0, g)
    grow["g_deleted"] = gdel
    ds = vb.DeviceSegment.maintain(gix, deleted, grow)
    nix = vb.GpuIndex(ds)
    nf = f.remap(nix, deleted, gdel)
    ff = vb.DocFilter(nix, remap_bits(bits[:, :n], deleted, bits[:, n:], gdel))
    terms, off = queries(ds.n_terms, 24, 3, seed=3)
    sel = (np.arange(24) % 4).astype(np.uint32)
    sel[sel == 3] = NONE
    seen = 0
    for k in (10, 1500):
        h1, n1 = vb.search_batch_masked(nix, terms, off, k, nf, sel)
        h2, n2 = vb.search_batch_masked(nix, terms, off, k, ff, sel)
        assert np.array_equal(n1, n2) and h1.tobytes() == h2.tobytes(), k
        seen += int(n1.sum())
    assert seen > 0
    # the single document's bitmap returns that document (at its new id) or nothing
    new_id = int((~deleted[:single]).sum())
    h, nh = vb.search_batch_masked(nix, terms, off, 10, nf, np.full(24, 2, np.uint32))
    assert all(set(h["doc_id"][q, :nh[q]].tolist()) <= {new_id} for q in range(24))


def test_everything_deleted():
    n, g = 1000, 65
    seg, gix, G = setup(n)
    rng = np.random.default_rng(2)
    f, gs, bits_s, bits_g = old_filter(gix, n, G, g, 3, rng)
    grow = docs(G, 0, g)
    grow["g_deleted"] = np.ones(g, np.uint8)
    deleted = np.ones(n, bool)
    ds = vb.DeviceSegment.maintain(gix, deleted, grow)
    assert ds.n_docs == 0
    nix = vb.GpuIndex(ds)
    nf = f.remap(nix, deleted, grow["g_deleted"])
    assert nf.words == 0 and all(len(nf.read(i)) == 0 for i in range(3))
    h, nh = vb.search_batch_masked(nix, np.array([0, 1, 2], np.uint32), np.array([0, 2, 3], np.uint32), 10, nf, np.array([0, NONE], np.uint32))
    assert nh.tolist() == [0, 0]


def test_refusals_leave_nothing_behind():
    n, g = 1001, 70
    c = make_corpus(n, 50, seed=77, length="lognormal", mean_len=12)
    seg = vb.Segment.build(1.2, 0.75, c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])
    gix = vb.GpuIndex(seg)
    G, _ = make_growing(seg.arrays()["term_key"], g, seed=3, deleted=None)
    rng = np.random.default_rng(4)
    f, gs, bits_s, bits_g = old_filter(gix, n, G, g, 2, rng)
    f_plain = vb.DocFilter(gix, bits_s)  # (no growing bitmaps)
    deleted = rng.random(n) < 0.3
    gdel = (rng.random(g) < 0.2).astype(np.uint8)
    grow = docs(G, 0, g)
    grow["g_deleted"] = gdel
    nix = vb.GpuIndex(vb.DeviceSegment.maintain(gix, deleted, grow))
    other = vb.GpuIndex(vb.DeviceSegment.maintain(gix, deleted, None))  # another compaction: the growing documents are missing
    terms, off = queries(seg.n_terms, 8, 3, seed=1)
    sel = (np.arange(8) % 2).astype(np.uint32)
    before = vb.search_batch_growing_masked(gix, gs, terms, off, 20, f, sel)
    L = vb.lib()
    words = vb.api._deleted_words(deleted, n)
    assert n % 64
    beyond = words.copy()
    beyond[-1] |= np.uint64(1) << np.uint64(63)
    W, Dg = words.ctypes.data, gdel.ctypes.data

    def refused(code, *args, message=()):
        out = C.c_void_p(1)
        assert L.vbm25_filter_remap(*args, C.byref(out)) == code, args
        assert out.value is None, "*out must be NULL after a refusal"
        err = L.vbm25_last_error().decode()
        assert all(str(m) in err for m in message), err
        after = vb.search_batch_growing_masked(gix, gs, terms, off, 20, f, sel)
        assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1])

    refused(INVALID, None, W, g, Dg, nix.h)
    refused(INVALID, f.h, W, g, Dg, None)
    assert L.vbm25_filter_remap(f.h, W, g, Dg, nix.h, None) == INVALID
    refused(INVALID, f.h, beyond.ctypes.data, g, Dg, nix.h, message=("n_docs", n))
    refused(UNSUPPORTED, f_plain.h, W, g, Dg, nix.h, message=("growing bitmaps",))
    refused(INVALID, f.h, W, g - 1, Dg, nix.h, message=(g, g - 1))
    refused(INVALID, f.h, W, g, Dg, other.h, message=(nix.n_docs, other.n_docs))  # remapped against the wrong compaction
    refused(INVALID, f.h, None, g, Dg, nix.h, message=(nix.n_docs,))  # ... or with other deletion inputs
    import torch
    if torch.cuda.device_count() > 1:  # (a new index on another device: only where there is one)
        far = vb.GpuIndex(seg, device=1)
        refused(INVALID, f.h, W, g, Dg, far.h, message=("device",))
    # n_grow == 0: the growing bitmaps are ignored
    nf = f.remap(other, deleted, np.zeros(0, np.uint8))
    want = remap_words(bits_s, deleted)
    assert all(nf.read(i).tobytes() == want[i].tobytes() for i in range(2))
    # and the valid call still works after all the refusals
    nf = f.remap(nix, deleted, gdel)
    want = remap_words(bits_s, deleted, bits_g, gdel)
    assert all(nf.read(i).tobytes() == want[i].tobytes() for i in range(2))


@pytest.mark.parametrize("rem", [0, 1, 31, 63])
def test_read(rem):
    """sealed and growing bitmaps read back after create, update, set_growing and extend_growing equal what DocFilter.pack makes of
    the bits; the growing base count is 0 / 1 / 31 / 63 mod 64"""
    n = 1000
    seg, gix, G = setup(n)
    rng = np.random.default_rng(50 + rem)
    F = 3
    bits = rng.random((F, n)) < 0.5
    f = vb.DocFilter(gix, bits)
    with pytest.raises(vb.Vbm25Error) as e:
        f.read(0, growing=True)
    assert e.value.code == INVALID
    with pytest.raises(vb.Vbm25Error) as e:
        f.read(F)
    assert e.value.code == INVALID

    def check(gbits=None):
        want = vb.DocFilter.pack(bits, n)
        for i in range(F):
            assert f.read(i).tobytes() == want[i].tobytes()
        if gbits is not None:
            gwant = vb.DocFilter.pack(gbits, gbits.shape[1])
            for i in range(F):
                got = f.read(i, growing=True)
                assert len(got) == gwant.shape[1] and got.tobytes() == gwant[i].tobytes()

    check()
    bits[1] = rng.random(n) < 0.2
    f.update(1, bits[1])
    check()
    n_old = 128 + rem
    gbits = rng.random((F, n_old + 1065)) < 0.5
    gs = vb.GrowingSegment(gix, **docs(G, 0, n_old))
    f.set_growing(gs, gbits[:, :n_old])
    check(gbits[:, :n_old])
    at = n_old
    for d in (1, 64, 1000):  # the second stays inside the capacity or re-strides, the third re-strides
        gs.append(**docs(G, at, at + d))
        f.extend_growing(gs, gbits[:, at:at + d])
        at += d
        check(gbits[:, :at])
    gbits[2, :at] = rng.random(at) < 0.7
    f.update_growing(2, gbits[2, :at])
    check(gbits[:, :at])
