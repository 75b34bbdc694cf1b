"""Synthetic growing (unsealed) segments for tests/test_gpu_growing.py and tools/growing_cost.py: CSR arrays in the form
vbm25_growing_search and vbm25_growing_upload take."""
import numpy as np


def _key_order(keys):
    """argsort of 16-byte keys in memcmp order"""
    k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 16)
    hi = k[:, :8].copy().view(">u8").ravel()
    lo = k[:, 8:].copy().view(">u8").ravel()
    return np.lexsort((lo, hi))


def make_growing(term_key, n_grow, seed, mean_elems=12, n_unknown=50, deleted=0.1, pool=None, pool_p=0.3,
                 fieldnorm_hi=200):
    """n_grow documents over the sealed keys plus `n_unknown` keys the sealed segment lacks: elements in ascending key order, tf 1..5,
    random fieldnorms (0 .. fieldnorm_hi - 1) and payloads; `pool` (term ids) are drawn with probability pool_p per element slot, so queries over them match."""
    rng = np.random.default_rng(seed)
    term_key = np.asarray(term_key, dtype=np.uint8).reshape(-1, 16)
    n_terms = len(term_key)
    extra = rng.integers(1, 256, (n_unknown, 16), dtype=np.uint8)
    extra[:, 0] = 0xFE  # (beyond every key of the corpora here)
    universe = np.concatenate([term_key, extra])
    order = _key_order(universe)
    rank = np.empty(len(universe), np.int64)
    rank[order] = np.arange(len(universe))
    lens = np.maximum(1, rng.poisson(mean_elems, n_grow))
    total = int(lens.sum())
    doc = np.repeat(np.arange(n_grow), lens)
    pick = rng.integers(0, len(universe), total)
    if pool is not None and len(pool):
        use = rng.random(total) < pool_p
        pick[use] = np.asarray(pool)[rng.integers(0, len(pool), int(use.sum()))]
    code = np.unique(doc.astype(np.int64) * len(universe) + rank[pick])
    d = code // len(universe)
    u = order[code % len(universe)]
    start = np.zeros(n_grow + 1, np.uint64)
    np.add.at(start, d + 1, 1)
    start = np.cumsum(start).astype(np.uint64)
    return dict(g_start=start, g_key=universe[u].reshape(-1), g_tf=rng.integers(1, 6, len(u)).astype(np.uint32),
                g_fieldnorm=rng.integers(0, fieldnorm_hi, n_grow).astype(np.uint8),
                g_payload=rng.integers(0, 65535, (n_grow, 3)).astype(np.uint16),
                g_deleted=(rng.random(n_grow) < deleted).astype(np.uint8) if deleted is not None else None), \
        np.where(u < n_terms, u, 0xFFFFFFFF).astype(np.uint32)
