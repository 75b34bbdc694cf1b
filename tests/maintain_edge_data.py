"""Inputs of vbm25_index_maintain at the edges of its value ranges and input forms, shared by tests/test_gpu_maintain_edges.py (the
device against the model) and tests/test_maintain_model.py (the model against the oracle's flush): sealed documents without a
posting, growing lengths at and beyond 2^32 - 1, a growing CSR that is a slice of a larger one, growing segments that are all empty,
all deleted, without and with nothing but unknown keys."""
import numpy as np

from corpus import make_corpus
from growing_data import make_growing

U32 = 2 ** 32 - 1
N_DOCS = 3000
FORMS = ["sliced", "no_flags", "all_empty", "all_deleted", "none_unknown", "all_unknown"]


def sparse_corpus(seed=3, n_docs=N_DOCS, n_bare=200):
    """build arguments after (k1, b) of a lognormal corpus whose documents are spread over n_docs ids, n_bare of them without any
    posting (length 0), and the ids of those"""
    c = make_corpus(n_docs - n_bare, 150, seed=seed, length="lognormal", mean_len=30, zipf=1.0)
    rng = np.random.default_rng(seed)
    at = np.sort(rng.choice(n_docs, n_docs - n_bare, replace=False))  # monotone: every list stays ascending
    doc_len = np.zeros(n_docs, np.uint32)
    doc_len[at] = c["doc_len"]
    payload = rng.integers(0, 65535, (n_docs, 3)).astype(np.uint16)
    bare = np.setdiff1d(np.arange(n_docs), at)
    return (doc_len, payload, c["term_key"], c["term_start"], at[c["post_doc"]].astype(np.uint32), c["post_tf"]), bare


def sparse_deletes(bare, seed=3, n_docs=N_DOCS):
    """a fifth of all documents deleted; of the documents without a posting every second one whatever the draw says"""
    deleted = np.random.default_rng(seed + 100).random(n_docs) < 0.2
    deleted[bare[::2]] = True
    deleted[bare[1::2]] = False
    return deleted


def hand_tf_growing(term_key, seed=3, n_grow=400):
    """make_growing's documents (about 3 elements each, keys the sealed segment lacks among them) with the tfs of four live documents
    set by hand -> (G, {case: (growing document, its Document::length())}):
    one: a single tf of 2^32 - 1; below: 2^31 - 1 twice = 2^32 - 2; at: 2^31 + (2^31 - 1) = 2^32 - 1, the clamp's value reached
    without saturating; over: 2^31 - 1 three times, saturated to 2^32 - 1"""
    G, _ = make_growing(term_key, n_grow, seed=seed, mean_elems=3, n_unknown=20)
    start = G["g_start"].astype(np.int64)
    n_el = np.diff(start)
    cases = {"one": [U32], "below": [2 ** 31 - 1, 2 ** 31 - 1], "at": [2 ** 31, 2 ** 31 - 1], "over": [2 ** 31 - 1] * 3}
    picked, used = {}, set()
    for name, tfs in cases.items():
        g = next(int(g) for g in np.flatnonzero(n_el == len(tfs)) if int(g) not in used)  # exactly that many elements: the sum is exact
        used.add(g)
        G["g_tf"][start[g]:start[g + 1]] = tfs
        G["g_deleted"][g] = 0
        picked[name] = (g, min(sum(tfs), U32))
    return G, picked


def growing_form(form, term_key, seed=5):
    """the growing dict of one input form"""
    if form == "sliced":  # documents 150 .. 449 of 600: start[0] != 0, the element arrays passed whole
        G, _ = make_growing(term_key, 600, seed=seed, mean_elems=6, n_unknown=20)
        assert G["g_start"][150] != 0 and G["g_start"][450] != len(G["g_tf"])
        return dict(g_start=G["g_start"][150:451].copy(), g_key=G["g_key"], g_tf=G["g_tf"], g_fieldnorm=G["g_fieldnorm"][150:450],
                    g_payload=G["g_payload"][150:450], g_deleted=G["g_deleted"][150:450])
    if form == "all_unknown":  # every key = a sealed key with 0x01 in its first zero byte: between the sealed keys, none of them
        G, _ = make_growing(term_key, 300, seed=seed, mean_elems=6, n_unknown=0)
        keys = G["g_key"].reshape(-1, 16).copy()
        assert (keys[:, 15] == 0).all()
        keys[np.arange(len(keys)), (keys == 0).argmax(axis=1)] = 1
        G["g_key"] = keys.reshape(-1)
        return G
    G, _ = make_growing(term_key, 300, seed=seed, mean_elems=6, n_unknown=0 if form == "none_unknown" else 20)
    if form == "no_flags":
        G["g_deleted"] = None
    elif form == "all_empty":  # every document live and without an element
        G.update(g_start=np.zeros(301, np.uint64), g_key=np.zeros(0, np.uint8), g_tf=np.zeros(0, np.uint32), g_deleted=np.zeros(300, np.uint8))
    elif form == "all_deleted":
        G["g_deleted"] = np.ones(300, np.uint8)
    else:
        assert form == "none_unknown"
    return G
