"""vbm25_device_growing_append_documents: after every append of cast documents the segment's records and document count equal those of
a FRESH GrowingSegment of the old documents plus the host model's cast of the new ones, byte for byte, at k = 1, 10 and 1500.
-m gpu only."""
import ctypes as C

import numpy as np
import pytest

import cast_model as cm
import vectorchord_bm25_amd as vb

pytestmark = pytest.mark.gpu
GT = 8192  # documents per tile of growing_scan_kernel
KS = (1, 10, 1500)
KNOWN, UNKNOWN = cm.words(120), cm.words(40, tag=b"unknown")


@pytest.fixture(scope="module")
def sealed():
    docs = cm.corpus(KNOWN, 3000, seed=1, mean=10)
    seg = cm.build_segment(cm.cast(docs, cm.payloads(3000, seed=1)), 1.2, 0.75)
    gix = vb.GpuIndex(seg)
    rng = np.random.default_rng(4)
    terms = np.concatenate([np.sort(rng.choice(seg.n_terms, 3, replace=False)) for _ in range(24)]).astype(np.uint32)
    return gix, terms, (np.arange(25) * 3).astype(np.uint32)


class Life:
    """a device growing segment and the model's CSR of the same documents"""

    def __init__(self, sealed, n0=300):
        self.gix, self.terms, self.off = sealed
        self.n = 0
        self.G = cm.cast(self.make(n0, KNOWN + UNKNOWN[:5]), self.pay(n0))
        self.gs = vb.GrowingSegment.from_dict(self.gix, self.G)

    def make(self, n, lexemes, mean=8):
        self.n += 1
        return cm.corpus(lexemes, n, seed=100 + self.n, mean=mean)

    def pay(self, n):
        return cm.payloads(n, seed=1000 + self.n)

    def append_documents(self, docs):
        pay = self.pay(len(docs))
        self.gs.append_documents(vb.Documents.cast(docs, pay, seed=cm.SEED))
        self.G = cm.concat(self.G, cm.cast(docs, pay))

    def append_host(self, docs):
        m = cm.cast(docs, self.pay(len(docs)))
        self.gs.append(m["g_start"], m["g_key"], m["g_tf"], m["g_fieldnorm"], m["g_payload"])
        self.G = cm.concat(self.G, m)

    def check(self, what, ks=KS):
        n = len(self.G["g_start"]) - 1
        assert self.gs.n_docs == n and int(vb.lib().vbm25_device_growing_docs(self.gs.h)) == n, what
        fresh = vb.GrowingSegment.from_dict(self.gix, self.G)
        for k in ks:
            want = vb.search_batch_growing(self.gix, fresh, self.terms, self.off, k)
            cm.same_records(vb.search_batch_growing(self.gix, self.gs, self.terms, self.off, k), want, f"{what} k={k}")
        return want


def test_one_document_then_a_tile_crossing(sealed):
    life = Life(sealed)
    life.append_documents(life.make(1, KNOWN))
    life.check("1 document")
    life.append_documents(life.make(513, KNOWN + UNKNOWN))
    life.check("513 documents")
    life.append_documents(life.make(GT, KNOWN, mean=3))  # past one tile of growing_scan_kernel
    assert life.gs.n_docs > GT
    life.check("across a tile")


def test_two_hundred_single_document_appends(sealed):
    life = Life(sealed)
    for i in range(200):
        life.append_documents(life.make(1, KNOWN + UNKNOWN[:3]))
        if i % 20 == 0:  # (where a drift would begin: every 20th append against a fresh upload; all three k at the end)
            life.check(f"append {i}", ks=(10,))
    life.check("200 appends")


def test_unknown_lexemes_count_for_the_length_and_never_score(sealed):
    life = Life(sealed)
    before = life.check("before")
    life.append_documents(life.make(50, UNKNOWN))  # all unknown to the sealed vocabulary
    after = life.check("all unknown")
    cm.same_records(after, before, "documents of unknown lexemes score nothing")
    # known and unknown mixed: the same known lexemes, with and without a crowd of unknown ones -- the longer document scores lower
    plain = [[(KNOWN[2 * i], 2), (KNOWN[2 * i + 1], 1)] for i in range(30)]
    crowded = [d + [(u, 40) for u in UNKNOWN] for d in plain]
    life.append_documents(plain + crowded)
    n = len(life.G["g_start"]) - 1
    fn = life.G["g_fieldnorm"]
    assert (fn[n - 30:] > fn[n - 60:n - 30]).all()  # the model's fieldnorm counts the unknown lexemes ...
    life.check("known and unknown mixed")  # ... and so does the segment's: its records equal the fresh upload's


def test_empty_documents_empty_handles_and_refusals(sealed):
    life = Life(sealed)
    life.append_documents([[]])
    life.append_documents([[], [(KNOWN[0], 1)], []])
    before = life.check("empty documents")
    n = life.gs.n_docs
    life.gs.append_documents(vb.Documents.cast([], np.zeros((0, 3), np.uint16)))  # a handle of 0 documents changes nothing
    assert life.gs.n_docs == n
    cm.same_records(life.check("a handle of 0 documents"), before, "a handle of 0 documents")
    bare = vb.Documents.cast(life.make(4, KNOWN), None, seed=cm.SEED)
    with pytest.raises(vb.Vbm25Error, match="without payloads") as e:
        life.gs.append_documents(bare)
    assert e.value.code == -1 and life.gs.n_docs == n
    cm.same_records(life.check("after the refusal"), before, "after the refusal")
    assert vb.lib().vbm25_device_growing_append_documents(life.gs.h, None) == -1
    assert vb.lib().vbm25_device_growing_append_documents(None, bare.h) == -1


def test_interleaved_with_host_appends_and_a_resident_batch(sealed):
    life = Life(sealed)
    batch = vb.Batch(life.gix, len(life.off) - 1, len(life.terms), 10)
    batch.set_growing(life.gs)
    batch.set_queries(life.terms, life.off)
    for i in range(6):
        docs = life.make(40 + i, KNOWN + UNKNOWN[:4])
        (life.append_documents if i % 2 else life.append_host)(docs)
        want = life.check(f"step {i}", ks=(10,))
        batch.run()
        cm.same_records(batch.fetch(), want, f"step {i}: the resident batch")
