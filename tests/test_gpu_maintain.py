"""vbm25_index_maintain on the device: every compacted segment, downloaded, is byte for byte what the host builder makes of the numpy
model of maintain.rs (tests/maintain_model.py), whatever index it starts from; searches on it match a host rebuild and the oracle."""
import numpy as np
import pytest

import orc
import vectorchord_bm25_amd as vb
from corpus import make_corpus, make_long_corpus, token_keys
from growing_data import make_growing
from maintain_model import NONE, maintain, make_growing_new_keys
from parity import assert_bit_exact

pytestmark = pytest.mark.gpu


def build_args(c):
    return (c["doc_len"], c["doc_payload"], c["term_key"], c["term_start"], c["post_doc"], c["post_tf"])


def corpus(kind, n=20_000, seed=1):
    if kind == "lognormal":
        return make_corpus(n, 600, seed=seed, length="lognormal", mean_len=40)
    if kind == "zipf":
        return make_corpus(n, 2000, seed=seed, length="lognormal", mean_len=40, zipf=1.0)
    return make_long_corpus(n // 2, 400, seed=seed, wide_tf=True)


def deletes(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "range":
        d = np.zeros(n, bool)
        d[n // 3: n // 3 + n // 5] = True
        return d
    return rng.random(n) < kind


def assert_same_segment(got, want, what=""):
    assert got.meta() == want.meta(), (what, got.meta(), want.meta())
    a, b = got.arrays(), want.arrays()
    for name in b:
        assert np.array_equal(a[name].reshape(-1), b[name].reshape(-1)), f"{what}: {name}"


def compact_and_check(gix, seg, deleted, growing, what=""):
    ds, relabel = vb.DeviceSegment.maintain(gix, deleted, growing, return_relabel=True)
    args, want_relabel = maintain(seg.arrays(), seg.meta(), deleted, growing)
    want = vb.Segment.build(*args)
    got = ds.download()
    assert_same_segment(got, want, what)
    assert np.array_equal(relabel, want_relabel), what
    return ds, got, args


@pytest.mark.parametrize("kind", ["lognormal", "zipf", "widetf"])
@pytest.mark.parametrize("dele", [0.0, 0.01, 0.5, 0.99, "range"])
@pytest.mark.parametrize("grow", [None, "mixed"])
def test_compaction_equals_the_model(kind, dele, grow):
    c = corpus(kind)
    seg = vb.Segment.build(1.2, 0.75, *build_args(c))
    gix = vb.GpuIndex(seg)
    G = None
    if grow:
        G = make_growing_new_keys(seg.arrays()["term_key"], 3000, seed=7)
        G2, _ = make_growing(seg.arrays()["term_key"], 2000, seed=8, deleted=0.1)
        # both kinds appended: make_growing's unknown keys sort after every sealed key, make_growing_new_keys' before / between / after
        G = {k: np.concatenate([G[k], G2[k] if k != "g_start" else G2[k][1:] + G[k][-1]]) for k in G}
    compact_and_check(gix, seg, deletes(dele, seg.n_docs), G, f"{kind} {dele} {grow}")


def edge_corpus():
    """Kept: documents 0 .. 128 and every 3rd of 129 .. 999.  Terms left with 1, 127, 128 and 129 postings of far more, a term that
    vanishes, blocks emptied entirely, full bit-packed blocks that become byte-packed tails, widths that shrink (stride 3 -> 1)"""
    n = 3000
    rng = np.random.default_rng(5)
    lists = [np.r_[5, 1000:1400], np.r_[0:127, 1000:3000:2], np.r_[0:128, 1000:3000], np.r_[0:129, 1000:3000], np.arange(1000, 3000, 3),
             np.arange(129, 1000, 3), np.arange(129, 1000), np.arange(0, 3000, 97), np.r_[0, 2999]]
    keys, _ = token_keys(len(lists))
    docs, tfs, ts = [], [], [0]
    for l in lists:
        docs.append(l)
        tfs.append(np.where(rng.random(len(l)) < 0.05, rng.integers(1000, 70000, len(l)), rng.integers(1, 6, len(l))))
        ts.append(ts[-1] + len(l))
    docs, tfs = np.concatenate(docs).astype(np.uint32), np.concatenate(tfs).astype(np.uint32)
    doc_len = np.bincount(docs, weights=tfs, minlength=n).astype(np.uint32)
    payload = rng.integers(0, 65535, (n, 3)).astype(np.uint16)
    deleted = np.ones(n, bool)
    deleted[:129] = False
    deleted[129:1000:3] = False
    return (doc_len, payload, keys, np.array(ts, np.uint64), docs, tfs), deleted


def test_codec_edges():
    args, deleted = edge_corpus()
    seg = vb.Segment.build(1.2, 0.75, *args)
    gix = vb.GpuIndex(seg)
    ds, got, margs = compact_and_check(gix, seg, deleted, None, "edges")
    df = np.diff(margs[5].astype(np.int64))
    assert {1, 127, 128, 129} <= set(df.tolist()), df
    assert got.n_terms < seg.n_terms  # a term vanished
    a = got.arrays()
    assert np.any(a["blk_meta_doc"] >= 0x80) and np.any(a["blk_meta_doc"] < 0x80)
    # also with everything in the upper range kept instead (other tails)
    compact_and_check(gix, seg, ~deleted, None, "edges inverted")


@pytest.mark.parametrize("source", ["host", "device", "win_planes", "rel16_plane", "id16_plane"])
def test_every_kind_of_index_gives_the_same_bytes(tuning, source):
    c = corpus("lognormal", n=30_000, seed=3)
    seg = vb.Segment.build(1.2, 0.75, *build_args(c))
    if source == "device":
        gix = vb.GpuIndex(vb.DeviceSegment.build(1.2, 0.75, *build_args(c)))
    else:
        if source != "host":
            tuning(**{source: 0})
        gix = vb.GpuIndex(seg)
    G, _ = make_growing(seg.arrays()["term_key"], 1000, seed=2)
    compact_and_check(gix, seg, deletes(0.1, seg.n_docs, seed=4), G, source)


def test_packed_words_and_no_relabel():
    """The default call: sealed_deleted as packed uint64 words (packed here with numpy, not by the API) and relabel NULL -- the same
    bytes as the bool-array call that asks for relabel, and as the model"""
    c = corpus("zipf", n=12_345, seed=4)
    seg = vb.Segment.build(1.2, 0.75, *build_args(c))
    gix = vb.GpuIndex(seg)
    deleted = deletes(0.2, seg.n_docs, seed=2)
    words = np.zeros((seg.n_docs + 63) // 64, np.uint64)
    packed = np.packbits(deleted, bitorder="little")
    words.view(np.uint8)[:len(packed)] = packed
    G = make_growing_new_keys(seg.arrays()["term_key"], 1500, seed=9)
    ds = vb.DeviceSegment.maintain(gix, words, G)
    assert isinstance(ds, vb.DeviceSegment)
    got = ds.download()
    args, _ = maintain(seg.arrays(), seg.meta(), deleted, G)
    assert_same_segment(got, vb.Segment.build(*args), "packed words, no relabel")
    ds2, _, _ = compact_and_check(gix, seg, deleted, G, "bool flags, relabel")
    assert_same_segment(got, ds2.download(), "words vs flags")


def test_index_and_growing_from_pages():
    """An index flattened from the reference's page layout (vbm25_segment_from_pages) and its growing segment as
    vbm25_growing_from_pages reads it from the vectors tape: documents with no element, documents larger than a page, keys the sealed
    segment lacks, deleted growing documents"""
    c = make_corpus(3000, 500, seed=3, length="lognormal", mean_len=40)
    seg = vb.Segment.build(1.2, 0.75, *build_args(c))
    oix = orc.OracleIndex.from_arrays(seg.meta(), seg.arrays())
    pages = orc.Pages(oix, seed=bytes(range(32)))
    keys = [bytes(k) for k in seg.arrays()["term_key"]]
    extra = [b"\x01" + bytes([i]) + b"\0" * 14 for i in range(1, 4)] + [b"\xfe" + bytes([i]) * 15 for i in range(1, 4)]
    extra += [k[:k.index(b"\0")] + b"\x01" + k[k.index(b"\0") + 1:] for k in keys[10:13]]  # between a key and the keys it prefixes
    universe = sorted(set(keys + extra))
    rng = np.random.default_rng(4)
    for i in range(150):
        n = int(rng.choice([0, 1, 3, 40, 200, 900]))
        ks = [universe[j] for j in sorted(rng.choice(len(universe), min(n, len(universe)), replace=False))]
        if i < len(extra):
            ks = sorted(set(ks) | {extra[i]})
        pages.insert(rng.integers(0, 65535, 3).astype(np.uint16), ks, rng.integers(1, 9, len(ks)).astype(np.uint32))
    pages.mark_deleted_growing(7)
    pages.mark_deleted_growing(88)
    pl = [pages.page(i) for i in range(len(pages))]
    flat = vb.segment_from_pages(pl)
    g = vb.growing_from_pages(pl)
    assert g["g_deleted"].sum() == 2 and (np.diff(g["g_start"].astype(np.int64)) == 0).any()
    gix = vb.GpuIndex(flat)
    ds, got, args = compact_and_check(gix, flat, deletes(0.1, flat.n_docs, seed=6), g, "pages")
    assert got.n_terms > seg.n_terms  # the new keys became tokens


def test_no_deletes_no_growing_recomputes_the_fieldnorms():
    """rule 2 (maintain.rs:344-362): lengths become the number of distinct tokens, so fieldnorm codes change where a tf > 1"""
    c = corpus("lognormal", seed=9)
    seg = vb.Segment.build(1.2, 0.75, *build_args(c))
    ds, got, _ = compact_and_check(vb.GpuIndex(seg), seg, None, None, "identity")
    assert got.n_docs == seg.n_docs and got.n_terms == seg.n_terms
    fn0, fn1 = seg.arrays()["doc_fieldnorm"], got.arrays()["doc_fieldnorm"]
    assert np.any(fn0 != fn1) and np.all(fn1 <= fn0)


def test_everything_deleted():
    c = corpus("lognormal", n=5000, seed=2)
    seg = vb.Segment.build(1.2, 0.75, *build_args(c))
    gix = vb.GpuIndex(seg)
    ds, relabel = vb.DeviceSegment.maintain(gix, np.ones(seg.n_docs, bool), None, return_relabel=True)
    assert (ds.n_docs, ds.n_terms, ds.n_blocks, ds.n_postings) == (0, 0, 0, 0)
    assert np.all(relabel == NONE)
    eix = vb.GpuIndex(ds)
    hits, nh = vb.search_batch(eix, np.array([0, 1, 2], np.uint32), np.array([0, 2, 3], np.uint32), 10)
    assert nh.tolist() == [0, 0]
    # everything sealed deleted, growing documents present: only they are left
    G, _ = make_growing(seg.arrays()["term_key"], 500, seed=4)
    G["g_deleted"][:] = 1
    ds, relabel = vb.DeviceSegment.maintain(gix, np.ones(seg.n_docs, bool), G, return_relabel=True)
    assert ds.n_docs == 0 and np.all(relabel == NONE)
    G["g_deleted"][::2] = 0
    ds2, got, _ = compact_and_check(gix, seg, np.ones(seg.n_docs, bool), G, "growing only")
    assert got.n_docs == int((G["g_deleted"] == 0).sum())


def test_search_after_compaction():
    c = corpus("zipf", n=40_000, seed=11)
    seg = vb.Segment.build(1.2, 0.75, *build_args(c))
    gix = vb.GpuIndex(seg)
    G = make_growing_new_keys(seg.arrays()["term_key"], 4000, seed=3)
    ds, got, args = compact_and_check(gix, seg, deletes(0.05, seg.n_docs, seed=1), G, "search")
    cix = vb.GpuIndex(ds)
    want = vb.Segment.build(*args)
    hix = vb.GpuIndex(want)
    rng = np.random.default_rng(2)
    nq, nt = 64, 3
    terms = np.sort(np.stack([rng.choice(got.n_terms, nt, replace=False) for _ in range(nq)]), axis=1).reshape(-1).astype(np.uint32)
    off = (np.arange(nq + 1) * nt).astype(np.uint32)
    oix = orc.OracleIndex.from_arrays(got.meta(), got.arrays())
    for k in (1, 10, 100, 1000, 1500):
        h1, n1 = vb.search_batch(cix, terms, off, k)
        h2, n2 = vb.search_batch(hix, terms, off, k)
        assert np.array_equal(n1, n2) and h1.tobytes() == h2.tobytes(), k
    for k in (10, 100):
        h1, n1 = vb.search_batch(cix, terms[:16 * nt], off[:17], k)
        ref, nref, _ = oix.search_batch(terms[:16 * nt], off[:17], k, mode="brute", threads=8)
        assert np.array_equal(n1, nref)
        for q in range(16):
            assert_bit_exact(ref[q, :nref[q]], h1[q, :n1[q]], what=f"k={k} q{q}")


def test_rejected_inputs_leave_the_index_serving():
    c = corpus("lognormal", n=8001, seed=6)
    seg = vb.Segment.build(1.2, 0.75, *build_args(c))
    gix = vb.GpuIndex(seg)
    rng = np.random.default_rng(0)
    terms = np.sort(np.stack([rng.choice(seg.n_terms, 3, replace=False) for _ in range(8)]), axis=1).reshape(-1).astype(np.uint32)
    off = (np.arange(9) * 3).astype(np.uint32)
    before = vb.search_batch(gix, terms, off, 20)
    G, _ = make_growing(seg.arrays()["term_key"], 200, seed=1)
    bad = []
    g = {k: v.copy() for k, v in G.items()}
    s, e = int(g["g_start"][3]), int(g["g_start"][4])
    assert e - s >= 2
    keys = g["g_key"].reshape(-1, 16)
    keys[[s, s + 1]] = keys[[s + 1, s]]  # keys not ascending
    bad.append((None, g))
    g = {k: v.copy() for k, v in G.items()}
    g["g_tf"][5] = 0
    bad.append((None, g))
    g = {k: v.copy() for k, v in G.items()}
    g["g_start"][7] = g["g_start"][8] + 1  # start not monotone
    bad.append((None, g))
    g = {k: v.copy() for k, v in G.items()}
    g["g_start"][-1] = len(g["g_tf"]) + 1  # beyond the elements
    bad.append((None, g))
    words = np.zeros((seg.n_docs + 63) // 64, np.uint64)
    assert seg.n_docs % 64
    words[-1] = np.uint64(1) << np.uint64(63)  # a bit beyond n_docs
    bad.append((words, None))
    for deleted, grow in bad:
        with pytest.raises(vb.Vbm25Error) as e:
            vb.DeviceSegment.maintain(gix, deleted, grow)
        assert e.value.code == -1
    after = vb.search_batch(gix, terms, off, 20)
    assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1])


def test_full_size_c3():
    """C3's device-generated index (10 M documents), 1 % deleted and 100 k growing documents: compacted, indexed, C3's 1024-query
    batch bit-exact against the oracle over the downloaded segment"""
    dseg = vb.DeviceSegment.synth(10_000_000, 30_000, mean_len=100, len_mode=1, zipf_s=0.0, seed=20260925)
    gix = vb.GpuIndex(dseg)
    n = dseg.n_docs
    deleted = np.random.default_rng(1).random(n) < 0.01
    keys, _ = token_keys(30_000)  # (the synthetic corpus' keys: decimals, bytewise order)
    G = make_growing_new_keys(keys, 100_000, seed=5, mean_elems=60)
    ds, relabel = vb.DeviceSegment.maintain(gix, deleted, G, return_relabel=True)
    del gix, dseg
    live_g = G["g_deleted"] == 0
    n_kept = int((~deleted).sum())
    assert ds.n_docs == n_kept + int(live_g.sum())
    assert np.array_equal(relabel[:n][~deleted], np.arange(n_kept)) and np.all(relabel[:n][deleted] == NONE)
    got = ds.download()
    # sum_len = the kept sealed documents' posting counts (rule 2) + the live growing documents' tf sums
    start = G["g_start"].astype(np.int64)
    e_live = np.repeat(live_g, np.diff(start))
    n_grow_post = int(e_live.sum())
    assert ds.n_postings == int(got.arrays()["term_df"].astype(np.int64).sum())
    assert got.desc.sum_len == (ds.n_postings - n_grow_post) + int(G["g_tf"][e_live].astype(np.int64).sum())
    cix = vb.GpuIndex(ds)
    rng = np.random.default_rng(3)
    terms = np.sort(np.stack([rng.choice(got.n_terms, 5, replace=False) for _ in range(1024)]), axis=1).reshape(-1).astype(np.uint32)
    off = (np.arange(1025) * 5).astype(np.uint32)
    hits, nh = vb.search_batch(cix, terms, off, 10)
    oix = orc.OracleIndex.from_arrays(got.meta(), got.arrays())
    ref, nref, _ = oix.search_batch(terms, off, 10, mode="brute", threads=16)  # (brute: ties by ascending id, as the device)
    assert np.array_equal(nh, nref)
    assert np.array_equal(hits["doc_id"], ref["doc_id"]) and np.array_equal(hits["score"].view(np.uint64), ref["score"].view(np.uint64))
    assert np.array_equal(hits["payload"], ref["payload"])
