"""vbm25_caster on the device: what collect hands out equals the host model's cast (tests/cast_model.py), or the one-shot
Documents.cast where the model would be slow, array for array and under every cast_pack setting -- the packing edges, isolation
between the documents of one wave, the in-lane intern, the grid stride, the ring, the refusals word for word, no allocation per call,
slot reuse, the consumers of a collected handle, Documents.extend, and two threads.  -m gpu only."""
import threading

import numpy as np
import pytest

import cast_model as cm
import caster_data as cd
import vectorchord_bm25_amd as vb

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
PACKS = (0, 1, 2)
M = 0xFFFFFFFF


@pytest.fixture(scope="module")
def caster():
    """one ring of three slots for the small batches: 1200 documents, 16384 lexemes (4096 of them in long documents), 1 MiB"""
    c = vb.Caster(0, 3, 1200, 16384, 1 << 20, max_long_lexemes=4096, seed=cm.SEED)
    yield c
    c.close()


def through(c, docs, pay=None):
    c.submit(docs, pay)
    return c.collect()


def check(c, docs, what, pay="make"):
    if isinstance(pay, str):  # (the download of 0 documents has no payload array, whether the cast was given one or not)
        pay = cm.payloads(len(docs), seed=len(docs)) if docs else None
    want = cm.cast(docs, pay)
    h = through(c, docs, pay)
    assert (h.n_docs, h.n_elements, h.device) == (len(docs), len(want["g_tf"]), 0), what
    cm.assert_same(h.download(), want, what)
    return h


@pytest.mark.parametrize("pack", PACKS)
def test_packing_edges(caster, tuning, pack):
    tuning(cast_pack=pack)
    for name, sizes in cd.PACKING.items():
        check(caster, cd.docs_of(sizes, seed=len(sizes)), f"{name} (cast_pack {pack})")
    assert through(caster, [], np.zeros((0, 3), np.uint16)).n_docs == 0
    tuning(cast_wave_max=8)
    check(caster, cd.docs_of(cd.WAVE_MAX_8, pool=12), f"cast_wave_max 8 (cast_pack {pack})")
    tuning(cast_wave_max=8, cast_group_max=16)  # (the 70-lexeme document takes the general class)
    check(caster, cd.docs_of(cd.WAVE_MAX_8, pool=12), f"cast_wave_max 8, cast_group_max 16 (cast_pack {pack})")


@pytest.mark.parametrize("pack", PACKS)
def test_documents_of_one_wave_never_merge(caster, tuning, pack):
    tuning(cast_pack=pack)
    k, o = b"k", b"a-long-lexeme-shared-by-neighbours"
    docs = [[(k, 1)], [(k, 1)], [(k, 2), (o, 1), (k, 3)], [(o, 1), (k, 4), (o, 2)], [(k, 1)], [],
            [(k, M), (k, 1)], [(k, 1)],                                  # saturation inside a document, its neighbour's k stays 1
            [(b"p", 0xFFFFFFF0), (b"q", 0xFFFFFFF0)], [(b"p", M), (b"q", M), (b"r", M)], [(k, 1)]]  # two lengths that saturate
    got = check(caster, docs, f"isolation (cast_pack {pack})").download()
    s = got["g_start"].astype(np.int64)
    tf = lambda d: got["g_tf"][s[d]:s[d + 1]].tolist()  # noqa: E731
    # the model's own figures, so that a model and a kernel wrong in the same way do not agree unseen
    assert tf(0) == [1] and tf(1) == [1] and sorted(tf(2)) == [1, 5] and sorted(tf(3)) == [3, 4] and tf(4) == [1] and tf(5) == []
    assert tf(6) == [M] and tf(7) == [1] and tf(10) == [1]
    assert got["length"][8] == M and got["length"][9] == M and got["g_fieldnorm"][8] == 255 and got["length"][7] == 1


@pytest.mark.parametrize("pack", PACKS)
def test_intern_in_the_lanes(caster, tuning, pack):
    tuning(cast_pack=pack)
    docs = cd.intern_docs()
    want = cm.shared("caster intern", lambda: cm.cast(docs, cm.payloads(len(docs))))
    h = through(caster, docs, cm.payloads(len(docs)))
    cm.assert_same(h.download(), want, f"all wave class: the fused path under cast_pack 2 (cast_pack {pack})")
    # settings 1 and 2 give the same bytes by design: which kernels ran is what tells them apart
    assert cd.launched(caster) == (cd.INTERN | cd.WAVE, cd.INTERN | cd.PACK, cd.PACK_FUSED)[pack]
    # the same documents and one of 3000 lexemes: the keys go through HBM
    long_doc = [(cd.lex(i % 1700), 1 + i % 3) for i in range(3000)]
    want2 = cm.shared("caster intern + long", lambda: cm.cast(docs + [long_doc], cm.payloads(len(docs) + 1)))
    h2 = through(caster, docs + [long_doc], cm.payloads(len(docs) + 1))
    cm.assert_same(h2.download(), want2, f"with a general-class document (cast_pack {pack})")
    assert cd.launched(caster) == (cd.INTERN | cd.WAVE, cd.INTERN | cd.PACK, cd.INTERN | cd.PACK)[pack]


@pytest.fixture(scope="module")
def stride():
    """20 000 documents of 1 .. 3 lexemes, their one-shot cast and a caster that takes them"""
    rng = np.random.default_rng(8)
    docs = cd.docs_of(rng.integers(1, 4, 20_000).tolist(), pool=300, seed=9)
    packed, pay = vb.pack_documents(docs), cm.payloads(len(docs))
    want = vb.Documents.cast(packed, pay, seed=cm.SEED).download()
    c = vb.Caster(0, 1, 20_000, 60_000, 1 << 20, seed=cm.SEED)
    yield packed, pay, want, c
    c.close()


@pytest.mark.parametrize("pack", PACKS)
@pytest.mark.parametrize("grid", (1, 3))
def test_grid_stride(stride, tuning, pack, grid):
    packed, pay, want, c = stride
    tuning(cast_pack=pack, cast_grid=grid)
    cm.assert_same(through(c, packed, pay).download(), want, f"20 000 documents (cast_pack {pack}, cast_grid {grid})")


@pytest.mark.parametrize("depth", (1, 2, 3))
def test_ring(depth):
    batches = [cd.docs_of(sizes, seed=i) for i, sizes in enumerate(([3, 0, 64, 5], [70, 1, 1], [2] * 40, [0], [9, 9, 9]))]
    with vb.Caster(0, depth, 64, 256, 8192, seed=cm.SEED) as c:
        assert c.in_flight() == 0
        rc, out, msg = cd.raw_collect(c)
        assert (rc, out, msg) == (INVALID, None, "nothing is in flight on the caster")
        for b in batches[:depth]:
            c.submit(b, cm.payloads(len(b)))
        assert c.in_flight() == depth
        rc, msg = cd.raw_submit(c, *vb.pack_documents(batches[0]), len(batches[0]))
        assert (rc, msg) == (INVALID, f"the caster's {depth} slots are all in flight: collect first") and c.in_flight() == depth
        # first in, first out; the ring keeps turning past its depth
        for i, b in enumerate(batches):
            cm.assert_same(c.collect().download(), cm.cast(b, cm.payloads(len(b))), f"depth {depth} batch {i}")
            if i + depth < len(batches):
                nxt = batches[i + depth]
                c.submit(nxt, cm.payloads(len(nxt)))
        assert c.in_flight() == 0
        with pytest.raises(vb.Vbm25Error, match="nothing is in flight"):
            c.collect()


@pytest.mark.parametrize("depth", (1, 16))
def test_ring_wraps_at_the_extreme_depths(depth):
    """2 * depth + 1 batches of two to four documents through a ring of `depth` slots: full, then collect one and submit one until
    none is left, then drained -- the cursor passes its end twice; every batch against the one-shot Documents.cast"""
    rng = np.random.default_rng(depth)
    batches = [cd.docs_of(rng.integers(0, 9, 2 + i % 3).tolist(), seed=100 + i) for i in range(2 * depth + 1)]
    pays = [cm.payloads(len(b), seed=i) if i % 3 else None for i, b in enumerate(batches)]
    want = [vb.Documents.cast(b, p, seed=cm.SEED).download() for b, p in zip(batches, pays)]
    with vb.Caster(0, depth, 4, 64, 2048, seed=cm.SEED) as c:
        made = (c.allocations(), c.device_bytes())
        got = []
        for i, (b, p) in enumerate(zip(batches, pays)):
            if c.in_flight() == depth:
                got.append(c.collect().download())  # (downloaded before the slot is taken again)
            c.submit(b, p)
            assert c.in_flight() == min(i + 1, depth)
        while c.in_flight():
            got.append(c.collect().download())
        assert len(got) == len(batches)
        for i, (g, w) in enumerate(zip(got, want)):
            cm.assert_same(g, w, f"depth {depth} batch {i}")
        assert (c.allocations(), c.device_bytes()) == made and made[0] == depth * (3 + 2 + 12)  # (max_long_lexemes 0: no general scratch)
        with pytest.raises(vb.Vbm25Error, match="nothing is in flight"):
            c.collect()


def test_refusals_of_the_cast_word_for_word_and_the_casters_own():
    data = np.frombuffer(b"abc" + b"x" * 17 + b"d\0e", dtype=np.uint8)
    lex_off = np.array([0, 3, 20, 23], dtype=np.uint64)
    count = np.array([1, 2, 3], dtype=np.uint32)
    doc_lex = np.array([0, 2, 2, 3], dtype=np.uint32)
    good = [[(b"abc", 1), (b"x" * 17, 2)], [], [(b"d\0e", 3)]]
    with vb.Caster(0, 2, 4, 8, 64, seed=bytes(32)) as c, vb.Caster(0, 1, 4, 8, 64) as bare:
        c.submit(good)  # (one batch in flight: every refusal below leaves it there)
        cases = [((data, None, count, doc_lex, 3), INVALID, "NULL argument"),
                 ((data, lex_off, None, doc_lex, 3), INVALID, "NULL argument"),
                 ((data, lex_off, count, None, 3), INVALID, "NULL argument"),
                 ((None, lex_off, count, doc_lex, 3), INVALID, "NULL argument"),
                 ((data, lex_off, count, np.array([1, 2, 2, 3], dtype=np.uint32), 3), INVALID, "doc_lex[0] is 1, not 0"),
                 ((data, lex_off, count, np.array([0, 2, 1, 3], dtype=np.uint32), 3), INVALID, "doc_lex is not monotone at document 1"),
                 ((data, np.array([0, 3, 2, 23], dtype=np.uint64), count, doc_lex, 3), INVALID, "lex_off is not monotone at lexeme 1"),
                 ((data, lex_off, np.array([1, 0, 0], dtype=np.uint32), doc_lex, 3), INVALID, "lexeme 1 (document 0) has count 0"),
                 ((data, lex_off, np.array([1, 1, 0], dtype=np.uint32), doc_lex, 3), INVALID, "lexeme 2 (document 2) has count 0"),
                 ((data, lex_off, count, np.array([0, 1 << 31], dtype=np.uint32), 1), UNSUPPORTED, "2147483648 lexemes: one cast takes fewer than 2^31"),
                 # the caster's own: documents, lexemes and bytes over its capacities
                 ((data[:5], np.arange(6, dtype=np.uint64), np.ones(5, np.uint32), np.arange(6, dtype=np.uint32), 5), INVALID,
                  "5 documents exceed the caster's max_docs 4"),
                 ((data[:9], np.arange(10, dtype=np.uint64), np.ones(9, np.uint32), np.array([0, 9], dtype=np.uint32), 1), INVALID,
                  "9 lexemes exceed the caster's max_lexemes 8"),
                 ((np.zeros(65, np.uint8) + 97, np.array([0, 10, 65], dtype=np.uint64), np.ones(2, np.uint32), np.array([0, 2], dtype=np.uint32), 1), INVALID,
                  "65 bytes exceed the caster's max_bytes 64")]
        for args, code, text in cases:
            assert cd.raw_submit(c, *args) == (code, text), text
            assert c.in_flight() == 1
        # without a seed: the resolver's and vbm25_intern's words
        rc, msg = cd.raw_submit(bare, data, lex_off, count, doc_lex, 3)
        assert (rc, msg) == (INVALID, "a lexeme of 16 bytes or more needs the index's seed (Meta tuple)") and bare.in_flight() == 0
        rc, msg = cd.raw_submit(bare, data[20:], np.array([0, 3], dtype=np.uint64), count[:1], np.array([0, 1], dtype=np.uint32), 1)  # the NUL inside
        assert rc == INVALID and "needs the index's seed" in msg
        # a failed submit followed by a good one; the batch in flight all along is still right
        c.submit([[(b"z", 1), (b"a", 2), (b"z", 3)]])
        cm.assert_same(c.collect().download(), cm.cast(good, seed=bytes(32)), "the batch the refusals left in flight")
        cm.assert_same(c.collect().download(), cm.cast([[(b"z", 1), (b"a", 2), (b"z", 3)]], seed=bytes(32)), "the good submit behind them")
        cm.assert_same(through(bare, [[(b"b", 1), (b"a", 2), (b"b", 3)]]).download(), cm.cast([[(b"b", 1), (b"a", 2), (b"b", 3)]], seed=None), "no seed")


def test_general_class_capacity(tuning):
    long_doc = [(cd.lex(i), 1) for i in range(2049)]
    with vb.Caster(0, 1, 8, 4200, 1 << 17, max_long_lexemes=0, seed=cm.SEED) as none, \
            vb.Caster(0, 1, 8, 4200, 1 << 17, max_long_lexemes=2049, seed=cm.SEED) as some:
        with pytest.raises(vb.Vbm25Error, match="document 1 has 2049 lexemes: the caster was created with max_long_lexemes 0") as e:
            none.submit([[(b"a", 1)], long_doc, long_doc])
        assert e.value.code == UNSUPPORTED and none.in_flight() == 0
        cm.assert_same(through(none, [long_doc[:2048], []]).download(), cm.cast([long_doc[:2048], []]), "2048 lexemes are the workgroup's")
        with pytest.raises(vb.Vbm25Error, match="4098 lexemes in documents of the general class exceed the caster's max_long_lexemes 2049") as e:
            some.submit([long_doc, long_doc])
        assert e.value.code == INVALID and some.in_flight() == 0
        cm.assert_same(through(some, [long_doc, [(b"a", 1)]]).download(), cm.cast([long_doc, [(b"a", 1)]]), "2049 lexemes fit")
        # with both classes off an empty document is of the general class and needs no scratch
        tuning(cast_wave_max=0, cast_group_max=0)
        cm.assert_same(through(none, [[], []]).download(), cm.cast([[], []]), "empty general-class documents")


def test_no_allocation_per_call():
    with vb.Caster(0, 2, 700, 9000, 1 << 18, max_long_lexemes=3000, seed=cm.SEED) as c:
        allocations, held = c.allocations(), c.device_bytes()
        # per slot: a stream, two events, two pinned blocks, 6 scratch + 8 general + 6 result arrays
        assert allocations == 2 * (3 + 2 + 20) and held > 2 * (20 * 9000 * 2 + 16 * 9000)
        rng = np.random.default_rng(2)
        for i in range(20):
            n = [1, 40, 700, 3, 250, 0, 699, 12][i % 8]
            sizes = rng.integers(0, 12, n).tolist()
            if i % 5 == 4:
                sizes[0] = 2500  # (the general class)
            docs = cd.docs_of(sizes, pool=500, seed=i)
            pay = cm.payloads(n) if i % 3 else None
            got = through(c, docs, pay)
            cm.assert_same(got.download(), vb.Documents.cast(docs, pay, seed=cm.SEED).download(), f"round {i}")
            assert (c.allocations(), c.device_bytes()) == (allocations, held), f"round {i}"


def test_a_closed_caster_takes_its_documents_along():
    docs = cd.docs_of([3, 0, 5])
    with vb.Caster(0, 2, 8, 64, 1024, seed=cm.SEED) as c:
        pay = cm.payloads(len(docs))
        first, second = through(c, docs, pay), through(c, docs, pay)
        cm.assert_same(first.download(), cm.cast(docs, pay), "before close")
    for h in (first, second):  # (freed with the caster: refused in Python, nothing reads the arrays)
        with pytest.raises(vb.Vbm25Error, match="Caster that has been closed"):
            h.download()
        with pytest.raises(vb.Vbm25Error, match="Caster that has been closed"):
            vb.Documents.empty(payload=True).extend(h)
    del first, second


def test_slot_reuse():
    a, b, c3 = (cd.docs_of(s, seed=i) for i, s in enumerate(([5, 6, 7], [60, 3], [1, 1, 1, 1])))
    with vb.Caster(0, 2, 8, 128, 4096, seed=cm.SEED) as c:
        c.submit(a)
        ha = c.collect()
        c.submit(b)
        hb = c.collect()
        cm.assert_same(ha.download(), cm.cast(a), "batch i after batch i + 1 was submitted and collected")
        c.submit(c3)  # (takes batch a's slot; hb's is the other one)
        hc = c.collect()
        cm.assert_same(hb.download(), cm.cast(b), "batch i + 1 after batch i + 2")
        cm.assert_same(hc.download(), cm.cast(c3), "batch i + 2")
        assert hc.h.value == ha.h.value != hb.h.value
        vb.lib().vbm25_documents_free(hb.h)  # (does nothing: the handle is the caster's)
        cm.assert_same(hb.download(), cm.cast(b), "after vbm25_documents_free on a collected handle")
    del ha, hb, hc


KNOWN, UNKNOWN = cm.words(120), cm.words(20, tag=b"unknown")


@pytest.fixture(scope="module")
def world():
    docs = cm.corpus(KNOWN, 1500, seed=1, mean=10)
    seg = cm.build_segment(cm.cast(docs, cm.payloads(1500, seed=1)), 1.2, 0.75)
    gix = vb.GpuIndex(seg)
    rng = np.random.default_rng(4)
    terms = np.concatenate([np.sort(rng.choice(seg.n_terms, 3, replace=False)) for _ in range(24)]).astype(np.uint32)
    return gix, terms, (np.arange(25) * 3).astype(np.uint32)


def test_consumers_of_a_collected_handle(caster, world):
    gix, terms, off = world
    first = cm.corpus(KNOWN, 200, seed=7)
    docs = cm.corpus(KNOWN + UNKNOWN, 900, seed=8, mean=9)
    pay = cm.payloads(len(docs), seed=3)
    one_shot = vb.Documents.cast(docs, pay, seed=cm.SEED)
    got = through(caster, docs, pay)
    # the growing append
    base = cm.cast(first, cm.payloads(200))
    ga, gb = vb.GrowingSegment.from_dict(gix, base), vb.GrowingSegment.from_dict(gix, base)
    ga.append_documents(got)
    gb.append_documents(one_shot)
    assert ga.n_docs == gb.n_docs == 1100
    for k in (1, 10, 1500):
        cm.same_records(vb.search_batch_growing(gix, ga, terms, off, k), vb.search_batch_growing(gix, gb, terms, off, k), f"append k={k}")
    # bind and evaluate
    r = vb.Resolver(gix, 1, 64, 4096, 1 << 16, seed=cm.SEED)
    da, db = got.bind(r), one_shot.bind(r)
    for x, y in zip(da.download(), db.download()):
        assert np.array_equal(x, y)
    sa, sb = da.evaluate(terms, off), db.evaluate(terms, off)
    assert sa.tobytes() == sb.tobytes() and (sa > 0).any()
    # the index build
    cm.same_segment(vb.DeviceSegment.from_documents(got, 1.2, 0.75).download(), vb.DeviceSegment.from_documents(one_shot, 1.2, 0.75).download(),
                    "from_documents of a collected handle")
    assert got.device_bytes() >= one_shot.device_bytes()


def test_extend_chunks_through_the_ring(tuning):
    docs = cm.corpus(KNOWN + UNKNOWN, 1065, seed=12, mean=7)
    docs[1001] = [(KNOWN[i % 120], 1 + i % 2) for i in range(2100)]  # (a general-class document inside the large chunk)
    pay = cm.payloads(len(docs), seed=5)
    cuts = [0, 0, 1, 1001, 1065]  # chunks of 0, 1, 1000 and 64 documents
    whole = vb.Documents.empty(payload=True)
    assert (whole.n_docs, whole.n_elements) == (0, 0)
    with vb.Caster(0, 2, 1000, 16384, 1 << 18, max_long_lexemes=2100, seed=cm.SEED) as c:
        pending = []
        for lo, hi in zip(cuts, cuts[1:]):
            c.submit(docs[lo:hi], pay[lo:hi])
            pending.append(hi - lo)
            if len(pending) == 2:
                part = c.collect()
                assert part.n_docs == pending.pop(0)
                assert whole.extend(part) is whole
        whole.extend(c.collect())
    one_shot = vb.Documents.cast(docs, pay, seed=cm.SEED)
    assert (whole.n_docs, whole.n_elements) == (one_shot.n_docs, one_shot.n_elements) == (1065, one_shot.n_elements)
    cm.assert_same(whole.download(), one_shot.download(), "chunks of 0, 1, 1000 and 64 documents")
    cm.same_segment(vb.DeviceSegment.from_documents(whole, 1.2, 0.75).download(), vb.DeviceSegment.from_documents(one_shot, 1.2, 0.75).download(),
                    "from_documents of the extended handle")
    # an owned handle extends by an owned handle as well, and without payloads
    a, b = vb.Documents.cast(docs[:10], None, seed=cm.SEED), vb.Documents.cast(docs[10:40], None, seed=cm.SEED)
    for _ in range(3):
        a.extend(b)
    cm.assert_same(a.download(), vb.Documents.cast(docs[:10] + docs[10:40] * 3, None, seed=cm.SEED).download(), "owned onto owned, three times")


def test_extend_refusals_leave_dst_as_it_was():
    docs = cd.docs_of([3, 4, 5])
    pay = cm.payloads(3)
    L = vb.lib()
    dst = vb.Documents.cast(docs, pay, seed=cm.SEED)
    before = dst.download()
    bare = vb.Documents.cast(docs, None, seed=cm.SEED)
    with vb.Caster(0, 1, 8, 64, 1024, seed=cm.SEED) as c:
        mine = through(c, docs, pay)
        for d, s, text in ((dst.h, None, "NULL argument"), (None, dst.h, "NULL argument"), (dst.h, dst.h, "dst and src are the same handle"),
                           (mine.h, dst.h, "dst belongs to a caster: only an owned handle is extended"),
                           (dst.h, bare.h, "one handle has payloads and the other has none"),
                           (bare.h, dst.h, "one handle has payloads and the other has none")):
            assert L.vbm25_documents_extend(d, s) == INVALID and L.vbm25_last_error().decode() == text
        cm.assert_same(dst.download(), before, "dst after the refusals")
        dst.extend(mine)
        cm.assert_same(dst.download(), cm.cast(docs + docs, np.concatenate([pay, pay])), "and it still extends")
    import torch
    if torch.cuda.device_count() > 1:  # (different devices: only where a second one is there)
        other = vb.Documents.cast(docs, pay, seed=cm.SEED, device=1)
        assert L.vbm25_documents_extend(dst.h, other.h) == INVALID and b"device" in L.vbm25_last_error()


def test_two_threads(world):
    """two casters on one device, one thread each; then a caster beside a Stream that keeps answering with the records it gives alone"""
    gix, terms, off = world
    jobs = [(cd.docs_of([5, 0, 64, 9] * 40, seed=1), 1), (cd.docs_of([2, 2, 70, 1] * 40, pool=9, seed=2), 2)]
    wants = [cm.cast(d) for d, _ in jobs]
    errors = []

    def cast_loop(docs, depth, want, rounds=6):
        try:
            with vb.Caster(0, depth, 200, 8192, 1 << 17, seed=cm.SEED) as c:
                for _ in range(depth - 1):
                    c.submit(docs)
                for _ in range(rounds):
                    c.submit(docs)
                    cm.assert_same(c.collect().download(), want, "thread")
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=cast_loop, args=(d, depth, w)) for (d, depth), w in zip(jobs, wants)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    st = vb.Stream(gix, 2, len(off) - 1, len(terms), 10)
    st.submit(terms, off)
    alone = st.collect()
    t = threading.Thread(target=cast_loop, args=(jobs[0][0], 2, wants[0], 10))
    t.start()
    for _ in range(10):
        st.submit(terms, off)
        cm.same_records(st.collect(), alone, "the stream beside a caster")
    t.join()
    assert not errors, errors
