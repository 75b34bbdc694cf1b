"""vbm25_documents_cast on the device against the host model (tests/cast_model.py), array for array: every batch through the default
classes and through each class forced by cast_wave_max / cast_group_max, the class edges, the key order traps, dedup and saturation,
the grid stride, the refusals, two threads at once, and download.

One case of the issue cannot be made from lexemes: two keys that differ ONLY in byte 15.  A lexeme shorter than 16 bytes has key byte
15 == 0 and a hashed key cannot be steered, so that pair is covered where keys can be given directly (tests/native/fuzz_cast.cpp, on
the text the kernels compile); here the lowest byte lexemes reach, byte 14, stands in beside bytes 7 and 8."""
import ctypes as C
import threading

import numpy as np
import pytest

import cast_model as cm
import vectorchord_bm25_amd as vb

pytestmark = pytest.mark.gpu

GM = 2048  # CAST_GROUP_MAX
# (cast_wave_max, cast_group_max): the defaults, each class alone where it can take everything, and lowered bounds that move the edges
SWEEP = [(64, GM), (64, 0), (0, GM), (0, 0), (8, 16), (1, 128), (0, 64)]


def lex(i, hashed=None):
    """lexeme number i: short (the key is the bytes) or long (hashed)"""
    if hashed is None:
        hashed = i % 3 == 0
    return (b"a-long-lexeme-number-%09d" % i) if hashed else (b"t%d" % i)


def doc_of(n, base=0, repeat_every=0):
    """n lexemes, distinct unless repeat_every: then every repeat_every-th repeats an earlier one"""
    out = []
    for j in range(n):
        i = base + (j // 2 if repeat_every and j % repeat_every == 0 else j)
        out.append((lex((i * 7919) % 100003), 1 + (j * 5) % 9))  # (a permutation: the input is not in key order)
    return out


def edge_docs():
    sizes = [0, 0, 1, 2, 63, 64, 65, 0, GM - 1, GM, GM + 1, 0, 0, 64, 65, 3 * GM + 5, 0]
    return [doc_of(n, base=37 * k, repeat_every=(5 if k % 2 else 0)) for k, n in enumerate(sizes)]


def order_docs():
    long_a, long_b = b"x" * 1500, b"y" * 8193
    lexemes = [b"", b"\x01", b"\x7f", b"\x80", b"\x7fz", b"\x80a",
               b"abcdefgh1", b"abcdefgh2", b"1bcdefghXYZ", b"2bcdefghXYZ",         # equal first halves / equal second halves
               b"\x01" * 7 + b"\x02", b"\x01" * 8 + b"\x03",                        # byte 7 against byte 8
               b"\x02\x01", b"\x01\x02",                                            # the byte order inside a half
               b"ABCDEFGHIJKLMN1", b"ABCDEFGHIJKLMN2", b"ABCDEFGHIJKLMN" , b"ABCDEFGHIJKLMN1x",  # byte 14; 15 bytes beside 16 (hashed)
               b"ABCDEFGh", b"ABCDEFGi", b"ABCDEFGHi", b"ABCDEFGHj",               # only byte 7, only byte 8
               b"a\0b", b"a", b"\0", b"\xff" * 15, b"\xff" * 16, long_a, long_b, long_a + b"!", b"z" * 1024, b"z" * 1025]
    rng = np.random.default_rng(11)
    docs = [[(t, 1 + i % 4) for i, t in enumerate(lexemes)]]
    docs += [[(lexemes[i], 2), (lexemes[j], 3)] for i, j in rng.integers(0, len(lexemes), (40, 2))]
    docs.append([(lexemes[i], 1) for i in rng.permutation(len(lexemes))] * 3)              # 96 lexemes: past one wave
    docs.append([(t, 1) for t in lexemes] + doc_of(GM, base=5))                            # past one workgroup
    return docs


def dedup_docs():
    M = 0xFFFFFFFF
    docs = [[(b"r", 1)] * 2, [(b"r", 2)] * 3, [(b"r", 3)] * 64, [(b"r", 1)] * 65,
            [(b"same", 7)] * 5, [(b"same", 7)] * 100, [(b"same-but-a-long-lexeme-01", 1)] * 3000,
            [(b"k", M), (b"k", 1)], [(b"k", 0x80000000), (b"j", 5), (b"k", 0x80000000)], [(b"k", 0x7FFFFFFF)] * 3,
            [(b"k", 0x7FFFFFFF)] * 2,                                                 # just below the clamp
            [(b"p", 0xFFFFFFF0), (b"q", 0xFFFFFFF0)],                                 # distinct keys: the length saturates, code 255
            [(b"p", M), (b"q", M), (b"r", M)]]
    # a run of equal keys across a wave boundary (sorted position 64) and across a pass of the workgroup (position 256)
    docs.append([(b"a%03d" % i, 1) for i in range(60)] + [(b"m", 2)] * 10 + [(b"z%03d" % i, 3) for i in range(60)])
    docs.append([(b"z%03d" % i, 3) for i in range(40)] + [(b"m", 0x40000000)] * 12 + [(b"a%03d" % i, 1) for i in range(250)])
    docs.append([(b"m", 1), (b"a", 1)] * 700)
    return docs


BATCHES = {"edges": edge_docs, "order": order_docs, "dedup": dedup_docs}


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, make in BATCHES.items():
        docs = make()
        pay = cm.payloads(len(docs), seed=len(docs))
        out[name] = (docs, pay, cm.cast(docs, pay))
    return out


@pytest.mark.parametrize("name", sorted(BATCHES))
@pytest.mark.parametrize("wave_max,group_max", SWEEP)
def test_every_class_gives_the_models_arrays(models, tuning, name, wave_max, group_max):
    docs, pay, want = models[name]
    tuning(cast_wave_max=wave_max, cast_group_max=group_max)
    h = vb.Documents.cast(docs, pay, seed=cm.SEED)
    assert (h.n_docs, h.n_elements, h.device) == (len(docs), len(want["g_tf"]), 0)
    cm.assert_same(h.download(), want, f"{name} ({wave_max}, {group_max})")
    assert h.device_bytes() >= 8 * (len(docs) + 1) + 20 * h.n_elements + 11 * len(docs)


def test_saturation_figures(models):
    """the model's own figures for the saturation cases, so that a model and a kernel wrong in the same way do not agree unseen"""
    docs, pay, want = models["dedup"]
    got = vb.Documents.cast(docs, pay, seed=cm.SEED).download()
    s = got["g_start"].astype(np.int64)
    tf = lambda d: got["g_tf"][s[d]:s[d + 1]].tolist()  # noqa: E731
    assert tf(0) == [2] and tf(1) == [6] and tf(2) == [192] and tf(3) == [65] and tf(6) == [3000]
    assert tf(7) == [0xFFFFFFFF] and tf(9) == [0xFFFFFFFF] and tf(10) == [0xFFFFFFFE]
    assert tf(8) == [5, 0xFFFFFFFF] and got["length"][8] == 0xFFFFFFFF
    assert got["length"][11] == 0xFFFFFFFF and got["g_fieldnorm"][11] == 255 and tf(11) == [0xFFFFFFF0] * 2
    assert got["length"][12] == 0xFFFFFFFF and got["g_fieldnorm"][12] == 255
    assert tf(14)[250] == 0xFFFFFFFF and tf(15) == [700, 700]


def test_only_empty_documents_and_no_documents(tuning):
    for wave_max, group_max in ((64, GM), (0, GM), (0, 0)):
        tuning(cast_wave_max=wave_max, cast_group_max=group_max)
        docs = [[], [], []]
        h = vb.Documents.cast(docs, cm.payloads(3), seed=cm.SEED)
        assert (h.n_docs, h.n_elements) == (3, 0)
        cm.assert_same(h.download(), cm.cast(docs, cm.payloads(3)), "empty documents")
        h0 = vb.Documents.cast([], None)
        assert (h0.n_docs, h0.n_elements) == (0, 0)
        d0 = h0.download()
        assert d0["g_start"].tolist() == [0] and len(d0["g_tf"]) == 0 and len(d0["length"]) == 0 and d0["g_payload"] is None


@pytest.mark.parametrize("wave_max,group_max", [(64, GM), (0, GM), (0, 0)])
def test_grid_stride(tuning, wave_max, group_max):
    """70 000 documents of 2 lexemes through the wave kernel (more waves than its grid), the workgroup kernel (70 000 workgroup
    documents against a grid of 2048) and the general class"""
    docs, pay, want = cm.grid_stride_model(wide=False)
    tuning(cast_wave_max=wave_max, cast_group_max=group_max)
    cm.assert_same(vb.Documents.cast(docs, pay, seed=cm.SEED).download(), want, f"70 000 x 2 ({wave_max}, {group_max})")


@pytest.mark.parametrize("wave_max,group_max", [(64, GM), (0, 0)])
def test_grid_stride_of_the_per_element_kernels(tuning, wave_max, group_max):
    """560 000 elements: more than the 524 288 threads of one pass, so every thread of the general class's kernels (fill, the key
    passes, flag, head positions, emit) takes a second turn of its grid-stride loop; the defaults beside it for the intern and gather
    kernels at that size"""
    docs, pay, want = cm.grid_stride_model(wide=True)
    assert sum(map(len, docs)) > 2048 * 256
    tuning(cast_wave_max=wave_max, cast_group_max=group_max)
    cm.assert_same(vb.Documents.cast(docs, pay, seed=cm.SEED).download(), want, f"70 000 x 8 ({wave_max}, {group_max})")


def test_refusals_leave_null_and_the_device_usable():
    good = [[(b"abc", 1), (b"x" * 20, 2)], [(b"d", 3)]]
    data, lex_off, count, doc_lex = vb.pack_documents(good)
    L = vb.lib()

    def raw(seed, count):
        out = C.c_void_p(1)
        rc = L.vbm25_documents_cast(0, seed, data.ctypes.data, lex_off.ctypes.data, count.ctypes.data, doc_lex.ctypes.data, 2, None, C.byref(out))
        return rc, out.value, L.vbm25_last_error().decode()

    bad = count.copy()
    bad[-1] = 0  # the last lexeme of the last document
    assert raw(cm.SEED, bad) == (-1, None, "lexeme 2 (document 1) has count 0")
    cm.assert_same(vb.Documents.cast(good, seed=cm.SEED).download(), cm.cast(good), "after the zero count")
    rc, out, msg = raw(None, count)
    assert (rc, out) == (-1, None) and "needs the index's seed" in msg
    cm.assert_same(vb.Documents.cast(good, seed=cm.SEED).download(), cm.cast(good), "after the missing seed")
    # without a seed, short lexemes alone are fine
    short = [[(b"b", 1), (b"a", 2), (b"b", 3)]]
    cm.assert_same(vb.Documents.cast(short).download(), cm.cast(short, seed=None), "no seed")


def test_two_threads_cast_at_once(models):
    docs, pay, want = models["edges"]
    docs2, pay2, want2 = models["order"]
    errors = []

    def work(d, p, w):
        try:
            for _ in range(3):
                cm.assert_same(vb.Documents.cast(d, p, seed=cm.SEED).download(), w, "thread")
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=a) for a in ((docs, pay, want), (docs2, pay2, want2))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_download_forms_and_the_csr_is_a_legal_growing_desc():
    rng = np.random.default_rng(3)
    words = [lex(i) for i in range(60)]
    docs = [[(words[j], int(rng.integers(1, 5))) for j in rng.integers(0, 60, int(rng.integers(0, 30)))] for _ in range(400)]
    pay = cm.payloads(len(docs))
    want = cm.cast(docs, pay)
    h = vb.Documents.cast(docs, pay, seed=cm.SEED)
    cm.assert_same(h.download(), want, "with payload")
    no_len = h.download(with_length=False)
    assert no_len["length"] is None and np.array_equal(no_len["g_tf"], want["g_tf"])
    bare = vb.Documents.cast(docs, None, seed=cm.SEED).download()
    assert bare["g_payload"] is None and np.array_equal(bare["g_key"], want["g_key"])
    # the CSR goes up as a growing segment of an index over half of the words, and searches as the model's arrays do
    seg = cm.build_segment(cm.cast([[(w, 1)] for w in words[::2]] * 3, cm.payloads(90)), 1.2, 0.75)
    gix = vb.GpuIndex(seg)
    ids = np.arange(seg.n_terms, dtype=np.uint32)
    terms = np.concatenate([ids[:3], ids[5:9], ids[10:11]])
    q_off = np.array([0, 3, 7, 8], dtype=np.uint32)
    got = vb.search_batch_growing(gix, vb.GrowingSegment.from_dict(gix, h.download()), terms, q_off, 20)
    ref = vb.search_batch_growing(gix, vb.GrowingSegment.from_dict(gix, want), terms, q_off, 20)
    assert np.array_equal(got[1], ref[1]) and got[0].tobytes() == ref[0].tobytes() and got[1].max() > 0
