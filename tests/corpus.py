"""Small synthetic corpora for tests (numpy, doc-major; mirrors tests/fuzz:168-205 of the
reference: each document is L i.i.d. token draws, tf = multiplicity, length = sum tf)."""
import numpy as np


def token_keys(vocab):
    """intern() short path (vector.rs:21-24): ASCII decimal, zero padded to 16 bytes.
    Returns (keys sorted bytewise [V,16], rank_of_token[V])."""
    raw = np.zeros((vocab, 16), dtype=np.uint8)
    for t in range(vocab):
        s = str(t).encode()
        raw[t, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    order = np.lexsort(raw.T[::-1])  # bytewise lexicographic
    rank = np.empty(vocab, dtype=np.int64)
    rank[order] = np.arange(vocab)
    return raw[order], rank


def make_corpus(n_docs, vocab, seed=0, length="fixed", mean_len=100, zipf=None, max_len=2000):
    """Returns dict with doc_len, doc_payload, term_key (only terms that occur),
    term_start, post_doc, post_tf, and token->rank map (-1 if absent)."""
    rng = np.random.default_rng(seed)
    if length == "fixed":
        lens = np.full(n_docs, mean_len, dtype=np.int64)
    elif length == "lognormal":
        lens = np.clip(np.rint(rng.lognormal(np.log(mean_len * 0.8), 0.6, n_docs)), 8,
                       max_len).astype(np.int64)
    elif length == "mixed":  # a few very short / very long docs, exercises fieldnorm range
        lens = np.clip(np.rint(rng.lognormal(np.log(mean_len * 0.8), 1.0, n_docs)), 1,
                       max_len).astype(np.int64)
    else:
        raise ValueError(length)
    total = int(lens.sum())
    if zipf is None:
        toks = rng.integers(0, vocab, total)
    else:
        p = 1.0 / np.arange(1, vocab + 1) ** zipf
        p /= p.sum()
        toks = rng.choice(vocab, total, p=p)
    docs = np.repeat(np.arange(n_docs), lens)
    keys_sorted, rank = token_keys(vocab)
    r = rank[toks]
    # (term rank, doc) pairs -> unique with counts
    code = r * n_docs + docs
    uniq, cnt = np.unique(code, return_counts=True)
    post_rank = uniq // n_docs
    post_doc = (uniq % n_docs).astype(np.uint32)
    post_tf = cnt.astype(np.uint32)
    present = np.unique(post_rank)
    dense = np.full(vocab, -1, dtype=np.int64)
    dense[present] = np.arange(len(present))
    dr = dense[post_rank]
    term_start = np.zeros(len(present) + 1, dtype=np.uint64)
    np.add.at(term_start, dr + 1, 1)
    term_start = np.cumsum(term_start).astype(np.uint64)
    doc_payload = np.stack([(np.arange(n_docs) // 64) >> 16, (np.arange(n_docs) // 64) & 0xffff,
                            np.arange(n_docs) % 64 + 1], axis=1).astype(np.uint16)
    token_to_term = np.full(vocab, -1, dtype=np.int64)
    token_to_term[:] = dense[rank]
    return dict(
        n_docs=n_docs, doc_len=lens.astype(np.uint32), doc_payload=doc_payload,
        term_key=keys_sorted[present], term_start=term_start, post_doc=post_doc, post_tf=post_tf,
        token_to_term=token_to_term, vocab=vocab)


def make_queries(corpus, nq, n_terms, seed=1, zipf=None):
    """Distinct tokens per query drawn like document tokens; returned as ascending term ranks
    (CSR).  Tokens absent from the index are kept as rank >= n_terms (ignored by search)."""
    rng = np.random.default_rng(seed)
    vocab = corpus["vocab"]
    n_idx_terms = len(corpus["term_key"])
    terms, off = [], [0]
    if zipf is not None:
        p = 1.0 / np.arange(1, vocab + 1) ** zipf
        p /= p.sum()
    for _ in range(nq):
        if zipf is None:
            toks = rng.choice(vocab, size=min(n_terms, vocab), replace=False)
        else:
            toks = np.unique(rng.choice(vocab, size=n_terms * 3, p=p))[:n_terms]
        t = corpus["token_to_term"][toks]
        t = np.where(t < 0, n_idx_terms + toks, t)  # unknown token -> out-of-range rank
        t = np.unique(t)
        terms.extend(t.tolist())
        off.append(len(terms))
    return np.array(terms, dtype=np.uint32), np.array(off, dtype=np.uint32)


def _from_draws(n_docs, vocab, doc, tok, tf_of, lens, seed):
    """postings of (document, token) draws: duplicates merged, tf_of(post_doc, n distinct terms of the document) -> tf; the
    same dict as make_corpus with `lens` as the document lengths"""
    keys_sorted, rank = token_keys(vocab)
    code = np.unique(rank[tok] * n_docs + doc)
    post_rank = code // n_docs
    post_doc = (code % n_docs).astype(np.uint32)
    m = np.bincount(post_doc, minlength=n_docs)
    post_tf = tf_of(post_doc, m[post_doc]).astype(np.uint32)
    present = np.unique(post_rank)
    dense = np.full(vocab, -1, dtype=np.int64)
    dense[present] = np.arange(len(present))
    term_start = np.zeros(len(present) + 1, dtype=np.uint64)
    np.add.at(term_start, dense[post_rank] + 1, 1)
    rng = np.random.default_rng(seed)
    return dict(
        n_docs=n_docs, doc_len=np.asarray(lens, dtype=np.uint32),
        doc_payload=rng.integers(0, 65536, (n_docs, 3)).astype(np.uint16),
        term_key=keys_sorted[present], term_start=np.cumsum(term_start).astype(np.uint64), post_doc=post_doc, post_tf=post_tf,
        token_to_term=dense[rank], vocab=vocab)


def make_long_corpus(n_docs, vocab, seed=0, wide_tf=False):
    """Every fieldnorm code 1..255 (about n_docs / 255 documents each, lengths up to 2^32 - 1).  A document of length L holds
    m <= min(L, 30) distinct terms; tf <= 127 (the byte planes of the index stay in use) or, wide_tf, log-uniform in
    [1, L // m] (tf beyond a byte, beyond 16 bits, up to 2^32 / 30).  The term frequencies of a document sum to at most L."""
    import orc

    L = orc.lib()
    lo = np.array([L.orc_fieldnorm_to_length(f) for f in range(256)], dtype=np.int64)
    hi = np.r_[lo[1:] - 1, 2 ** 32 - 1]
    rng = np.random.default_rng(seed)
    code = np.r_[np.arange(1, 256), rng.integers(1, 256, max(0, n_docs - 255))][rng.permutation(n_docs)]
    lens = lo[code] + (rng.random(n_docs) * (hi[code] - lo[code] + 1)).astype(np.int64)
    lens = np.minimum(lens, hi[code])
    m = np.minimum(lens, rng.integers(1, 31, n_docs))
    doc = np.repeat(np.arange(n_docs), m)
    tok = rng.integers(0, vocab, len(doc))
    cap = lens // np.maximum(m, 1)

    def tf_of(pd, _):
        c = cap[pd]
        if not wide_tf:
            return rng.integers(1, np.minimum(c, 127) + 1)
        return np.minimum(c, np.exp(rng.random(len(pd)) * np.log(c.astype(np.float64) + 1.0)).astype(np.int64) + 1)

    return _from_draws(n_docs, vocab, doc, tok, tf_of, lens, seed + 1)


def make_short_corpus(n_docs, vocab, seed=0, n_huge=40):
    """Short documents against a large mean: lengths 1..3 (one posting of tf 1 per token) but for n_huge documents of 10^6 ..
    2^32 - 1 tokens (up to 30 terms each, wide tf).  S1 = k1 (1 - b + b len / avgdl) is tiny for nearly every posting at b > 0."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, n_docs).astype(np.int64)
    huge = rng.choice(n_docs, n_huge, replace=False)
    lens[huge] = np.exp(rng.uniform(np.log(1e6), np.log(2.0 ** 32 - 1), n_huge)).astype(np.int64)
    m = np.minimum(lens, 30)
    doc = np.repeat(np.arange(n_docs), m)
    tok = rng.integers(0, vocab, len(doc))
    cap = lens // m

    def tf_of(pd, _):
        c = cap[pd]
        tf = np.minimum(c, np.exp(rng.random(len(pd)) * np.log(c.astype(np.float64) + 1.0)).astype(np.int64) + 1)
        return np.where(lens[pd] <= 3, 1, tf)

    # (a short document whose draws collided has fewer distinct terms than tokens: its length stays as drawn)
    return _from_draws(n_docs, vocab, doc, tok, tf_of, lens, seed + 1)


def make_tie_corpus(n_docs, vocab, seed=0, n_head=3, p_head=0.7):
    """Masses of equal scores at b = 0 (S1 = k1 for every document): tf 1 or 2 (2 with probability 1/20), n_head head terms
    (tokens 0 .. n_head - 1) in a fraction p_head of the documents each, 2..8 draws from the other tokens per document; lengths
    the sum of tf plus a lognormal rest (they matter only at b > 0)."""
    rng = np.random.default_rng(seed)
    hd = [np.flatnonzero(rng.random(n_docs) < p_head) for _ in range(n_head)]
    n_tail = rng.integers(2, 9, n_docs)
    doc = np.r_[np.concatenate(hd), np.repeat(np.arange(n_docs), n_tail)]
    tok = np.r_[np.concatenate([np.full(len(h), i) for i, h in enumerate(hd)]), rng.integers(n_head, vocab, int(n_tail.sum()))]
    c = _from_draws(n_docs, vocab, doc, tok, lambda pd, _: np.where(rng.random(len(pd)) < 0.05, 2, 1), np.zeros(n_docs, np.int64),
                    seed + 1)
    lens = np.bincount(c["post_doc"], weights=c["post_tf"], minlength=n_docs).astype(np.int64)
    lens += np.rint(rng.lognormal(np.log(20.0), 0.8, n_docs)).astype(np.int64)
    c["doc_len"] = lens.astype(np.uint32)
    return c
