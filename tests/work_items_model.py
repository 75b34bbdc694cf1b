"""The planner of every search route but the window route in plain integers, and the hand-made indexes of
tests/test_gpu_work_items.py.  No GPU, no call into the library: tests/test_work_items_model.py states what the GPU tests need of it.

A query is cut into c work items, document ranges [n_docs * i // c, n_docs * (i + 1) // c).  plan(...) restates who decides c:
  * the general route (plan_kernel and its host mirror at the end of plan_route): chunk = max(ceil(sparse postings of the batch /
    target items), min chunk), c = (postings + chunk // 2) // chunk, at least 1, at most n_docs; a dense query gets min(dense_c, n_docs);
    a query without postings gets no item;
  * the plan-free and the one-launch route (every query sparse, 1 .. 16 indexed terms, none without postings): every query the same
    g = (largest query's postings + chunk // 2) // chunk with chunk = min chunk (a quarter of it up to 8 queries), at most
    max((target + nq // 2) // nq, 1), at least 1, at most min(64, n_docs).
The window route makes its items of 2^16-document windows and is not modelled here (tests/test_gpu_win_boundaries.py)."""
import numpy as np

PLAN_WG = 1024
LISTS_PER_ITEM = 8            # scan_range_kernel / scan_dense_kernel: one list per wave; scan_many_kernel at k > 256: 1
REG_K = 256
R_TARGET_ITEMS, R_MIN_CHUNK = 1024, 16384
TARGET_ITEMS, MIN_CHUNK = 1536, 8192
D_TARGET_ITEMS = 12288
GENERAL, ONE_LAUNCH, PLAN_FREE, WINDOW = 0, 1, 2, 3

DEFAULTS = dict(dense_x1000=100, dense=1, fused=1, dense_items=D_TARGET_ITEMS, range_items=R_TARGET_ITEMS, range_min_chunk=R_MIN_CHUNK,
                fused_items=128, arith=1, win=1)


def csr(queries):
    """a list of term-id lists -> (terms uint32, offsets uint32)"""
    off = np.cumsum([0] + [len(q) for q in queries]).astype(np.uint32)
    terms = np.array([t for q in queries for t in q], dtype=np.uint32)
    return terms, off


def item_ranges(n_docs, c):
    return [(n_docs * i // c, n_docs * (i + 1) // c) for i in range(c)]


def plan(n_docs, df, queries, k, **tune):
    """df[t]: postings of term t (ids >= len(df) are unknown terms).  Returns a dict: route, c (items per query), total, chunk, g,
    dense_c, dense (flags), raw_c (c before the n_docs clamp; raw_g on the g routes), classes (general-route items of the sparse,
    dense and many-term kernel).  tune: the switches the GPU test sets (win must be 0: the window route is not modelled)."""
    t = dict(DEFAULTS)
    t.update(tune)
    assert 1 <= k <= 1024
    nq, n_terms = len(queries), len(df)
    use_range = k <= REG_K
    use_dense = use_range and t["dense"] != 0
    target = max(256, t["range_items"]) if use_range else TARGET_ITEMS
    min_chunk = max(128, t["range_min_chunk"]) if use_range else MIN_CHUNK
    valid = [sum(1 for x in q if x < n_terms) for q in queries]
    postings = [sum(int(df[x]) for x in q if x < n_terms) for q in queries]
    dense = [p * 1000 >= max(0, t["dense_x1000"]) * n_docs for p in postings]
    many = any(dense) or not use_range or any(v > 16 for v in valid)
    n_dense = sum(1 for p, d in zip(postings, dense) if d and p)
    has_dense = use_dense and any(d and v <= 16 for d, v in zip(dense, valid))
    range_mt = max([v for v, d in zip(valid, dense) if not d and v <= 16] + [0]) if use_range else 0
    out = dict(route=GENERAL, g=0, raw_g=0, dense=dense, postings=postings, valid=valid)
    if use_range and nq and not many and not has_dense and range_mt and all(postings):
        assert t["win"] == 0, "the window route is not modelled: pass win=0"
        chunk = max(min_chunk // 4, 1) if nq <= 8 else min_chunk
        raw_g = (max(postings) + chunk // 2) // chunk
        g = min(raw_g, max((target + nq // 2) // nq, 1))
        g = min(max(g, 1), min(64, n_docs))
        if t["fused"] and nq * g <= t["fused_items"]:
            out.update(route=ONE_LAUNCH, g=g, raw_g=raw_g)
        elif t["arith"]:
            out.update(route=PLAN_FREE, g=g, raw_g=raw_g)
    dense_c = 0
    if has_dense:
        dense_c = max(1, (max(256, t["dense_items"]) + n_dense // 2) // max(n_dense, 1))
        if t["dense_items"] == D_TARGET_ITEMS:
            dense_c = min(dense_c, max(max(1, 4096 // max(n_dense, 1)), n_docs >> 16))
    sparse = sum(p for p, d in zip(postings, dense) if not (dense_c and d))
    chunk = max((sparse + target - 1) // target, min_chunk)
    c, raw_c = [], []
    for p, d in zip(postings, dense):
        if p == 0:
            raw = 0
        elif dense_c and d:
            raw = dense_c
        else:
            raw = max((p + chunk // 2) // chunk, 1)
        raw_c.append(raw)
        c.append(min(raw, n_docs))
    if out["route"] != GENERAL:
        c = [out["g"]] * nq
    classes = [0, 0, 0]
    if out["route"] == GENERAL:
        for ci, v, d in zip(c, valid, dense):
            classes[2 if v > 16 else 1 if d else 0] += ci
    out.update(c=c, raw_c=raw_c, total=sum(c), chunk=chunk, dense_c=dense_c, classes=classes, has_dense=has_dense)
    return out


def plan_threads(nq):
    """plan_kernel: the queries q0 .. q1 of each of its 1024 threads"""
    per = (nq + PLAN_WG - 1) // PLAN_WG
    return per, [(min(nq, t * per), min(nq, t * per + per)) for t in range(PLAN_WG)]


# --------------------------------------------------------------------------------------------------------------------------------
# posting lists and their blocks
# --------------------------------------------------------------------------------------------------------------------------------
def keys(n):
    out = np.zeros((n, 16), dtype=np.uint8)
    for i in range(n):
        s = b"t%04d" % i
        out[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return out


def build_args(n_docs, lists, doc_len):
    """the arguments of vb.Segment.build after (k1, b); a document's payload is its id"""
    term_start = np.cumsum([0] + [len(d) for d, _ in lists]).astype(np.uint64)
    post_doc = np.concatenate([np.asarray(d, dtype=np.uint32) for d, _ in lists])
    post_tf = np.concatenate([np.asarray(f, dtype=np.uint32) for _, f in lists])
    payload = np.zeros((n_docs, 3), dtype=np.uint16)
    payload[:, :2] = np.arange(n_docs, dtype="<u4").view("<u2").reshape(n_docs, 2)
    return np.asarray(doc_len, dtype=np.uint32), payload, keys(len(lists)), term_start, post_doc, post_tf


def blocks(docs):
    """a list's blocks of 128 postings (the last one, if shorter, is the byte-packed tail): (min_doc, max_doc, n)"""
    docs = np.asarray(docs)
    return [(int(docs[i]), int(docs[min(i + 128, len(docs)) - 1]), min(128, len(docs) - i)) for i in range(0, len(docs), 128)]


def boundary_kinds(docs, b):
    """how the item boundary b (a doc_hi and the next doc_lo) falls into one list"""
    kinds = set()
    for lo, hi, n in blocks(docs):
        if lo < b <= hi:
            kinds.add("in_full" if n == 128 else "in_tail")
        if b == lo:
            kinds.add("on_min")
        if b == hi + 1:
            kinds.add("past_max")
    return kinds


def items_terms(lists, query, n_docs, c):
    """per item of the query: the set of its terms with a posting in the item's range"""
    out = []
    for lo, hi in item_ranges(n_docs, c):
        out.append({t for t in query if np.any((np.asarray(lists[t][0]) >= lo) & (np.asarray(lists[t][0]) < hi))})
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# B: the index of designed item cuts
# --------------------------------------------------------------------------------------------------------------------------------
B_DOCS, B_CUT = 6000, 8
B_EDGES = [B_DOCS * i // B_CUT for i in range(1, B_CUT)]   # 750, 1500, ..., 5250
T_W, T_S, T_L, T_H, T_F0 = 0, 1, 2, 3, 4                   # the wide list, the spikes, the low and the high list, 18 fillers
B_FILL = 18
B_K = 32


def _pick(rng, lo, hi, n, must=(), never=()):
    """n ascending documents of [lo, hi) with `must` among them and none of `never`"""
    pool = np.setdiff1d(np.arange(lo, hi), np.r_[np.asarray(must, dtype=np.int64), np.asarray(never, dtype=np.int64)])
    got = np.r_[np.asarray(must, dtype=np.int64), rng.choice(pool, n - len(must), replace=False)]
    return np.sort(got)


def cut_index(spikes="both"):
    """-> (n_docs, lists, doc_len).  The wide list W is laid over the eight ranges of 750 documents so that the seven inner boundaries
    fall: 750 inside a full block; 1500 on a block's first document; 2250 one past a block's last document (2250 itself absent);
    3000 inside a full block and itself in the list; 3750 both (2249 + 1500 = 3749 ends a block, 3750 begins the next); 4500 inside a
    full block; 5250 inside the byte-packed tail.  L lies in [0, 2250) and H in [3750, 6000): queried together, the items are one
    term's or, between them, empty; L ends on 2249 and H begins on 3750.
    The spikes -- term S, tf 200, and a length of one -- are the documents e - 1 and e of every inner boundary e ("both": every doc_lo
    and every doc_hi - 1, which are also every doc_hi and every doc_lo - 1 but for the ends of the index), or only the documents e
    ("lo") or only e - 1 ("hi"): then the other side of each boundary is an ordinary document.  Document 0 and the last one are
    spikes always."""
    rng = np.random.default_rng(11)
    E = B_EDGES
    step = B_DOCS // B_CUT
    # W: postings per range, so that the running count at each boundary is 64, 256, 384, 454, 640, 740, 940 (of 1010)
    seg = [
        _pick(rng, 0, E[0], 64, must=[0, E[0] - 1]),
        _pick(rng, E[0], E[1], 192, must=[E[0], E[1] - 1]),
        _pick(rng, E[1], E[2], 128, must=[E[1], E[2] - 1]),
        _pick(rng, E[2], E[3], 70, must=[E[3] - 1], never=[E[2]]),
        _pick(rng, E[3], E[4], 186, must=[E[3], E[4] - 1]),
        _pick(rng, E[4], E[5], 100, must=[E[4], E[5] - 1]),
        _pick(rng, E[5], E[6], 200, must=[E[5], E[6] - 1]),
        _pick(rng, E[6], B_DOCS, 70, must=[E[6], B_DOCS - 1]),
    ]
    w = np.concatenate(seg)
    assert len(w) == 1010 and np.all(np.diff(w) > 0)
    edge_docs = sorted({0, B_DOCS - 1} | {e - 1 for e in E if spikes in ("both", "hi")} | {e for e in E if spikes in ("both", "lo")})
    s = np.array(edge_docs)
    low = _pick(rng, 0, 3 * step, 500, must=[0, E[0] - 1, E[0], E[1] - 1, E[1], E[2] - 1])
    high = _pick(rng, 5 * step, B_DOCS, 520, must=[E[4], E[5] - 1, E[5], E[6] - 1, E[6], B_DOCS - 1])
    lists = [(w, rng.integers(1, 4, len(w))), (s, np.full(len(s), 200))]
    for d in (low, high):  # (S is not in their query: their own postings make the spikes)
        lists.append((d, np.where(np.isin(d, s), 200, rng.integers(1, 4, len(d)))))
    # fillers: 13 long ones and 5 short ones -- with W and S a 15-term and a 20-term query of about 8 x 8192 postings
    for i in range(B_FILL):
        n = 4660 if i < 13 else 1200
        d = np.sort(rng.choice(B_DOCS, n, replace=False))
        lists.append((d, rng.integers(1, 4, n)))
    doc_len = rng.integers(60, 300, B_DOCS)
    doc_len[s] = 1
    return B_DOCS, lists, doc_len


Q_WIDE = [T_W, T_S]
Q_SPLIT = [T_L, T_H]
Q_15 = [T_W, T_S] + [T_F0 + i for i in range(13)]
Q_20 = [T_W, T_S] + [T_F0 + i for i in range(B_FILL)]


def cut_cases():
    """name -> (queries, k, tuning, expected route, kernel class of the items: 0 sparse / 1 dense / 2 many-term / None).  Every case cuts
    each query into a multiple of eight items, so that 750, 1500, ... are boundaries in all of them; "-one" is the same route uncut."""
    two = [Q_WIDE, Q_SPLIT]
    general = dict(fused=0, win=0, arith=0, dense_x1000=10**9)
    free = dict(fused=0, win=0, dense_x1000=10**9)
    one = dict(fused=1, win=0, dense_x1000=10**9, fused_items=4096)
    return {
        "general": (two, B_K, dict(general, range_min_chunk=128, range_items=256), GENERAL, 0),
        "general-grid1": (two, B_K, dict(general, range_min_chunk=128, range_items=256, range_grid=1), GENERAL, 0),
        "general-one": (two, B_K, dict(general), GENERAL, 0),
        "plan-free": (two, B_K, dict(free, range_min_chunk=512, range_items=256), PLAN_FREE, None),
        "plan-free-finest": (two, B_K, dict(free, range_min_chunk=128, range_items=256), PLAN_FREE, None),
        "plan-free-grid1": (two, B_K, dict(free, range_min_chunk=128, range_items=256, range_grid=1), PLAN_FREE, None),
        "plan-free-one": (two, B_K, dict(free), PLAN_FREE, None),
        "one-launch": (two, B_K, dict(one, range_min_chunk=512, range_items=256), ONE_LAUNCH, None),
        "one-launch-finest": (two, B_K, dict(one, range_min_chunk=128, range_items=256), ONE_LAUNCH, None),
        "one-launch-one": (two, B_K, dict(one), ONE_LAUNCH, None),
        "dense-8": (two * 16, B_K, dict(fused=0, win=0, dense_x1000=0, dense_items=256), GENERAL, 1),
        "dense-128": (two, B_K, dict(fused=0, win=0, dense_x1000=0, dense_items=256), GENERAL, 1),
        "dense-128-grid1": (two, B_K, dict(fused=0, win=0, dense_x1000=0, dense_items=256, dense_grid=1), GENERAL, 1),
        "dense-default": (two, B_K, dict(fused=0, win=0, dense_x1000=0), GENERAL, 1),
        "dense-one": (two * 128, B_K, dict(fused=0, win=0, dense_x1000=0, dense_items=256), GENERAL, 1),
        "many-term": ([Q_20], B_K, dict(general, range_min_chunk=8192, range_items=256), GENERAL, 2),
        "many-term-finest": ([Q_20], B_K, dict(general, range_min_chunk=264, range_items=1024), GENERAL, 2),
        "many-term-one": ([Q_20], B_K, dict(general, range_min_chunk=1 << 20), GENERAL, 2),
        "k300": ([Q_15, Q_20], 300, dict(), GENERAL, None),
    }


# --------------------------------------------------------------------------------------------------------------------------------
# C: the merge -- every document one term, one tf, one length (two tfs for the second score level)
# --------------------------------------------------------------------------------------------------------------------------------
def flat_index(n_docs, high=(), docs=None):
    """one term in every document (or in `docs` only), tf 1 (tf 3 in the documents of `high`), every length 10: one score bit pattern
    (two with `high`), so the order of the hits is by document alone -- the documents of `high` ascending, then the others ascending"""
    docs = np.arange(n_docs) if docs is None else np.asarray(docs, dtype=np.int64)
    tf = np.where(np.isin(docs, np.asarray(high, dtype=np.int64)), 3, 1).astype(np.uint32)
    return n_docs, [(docs, tf)], np.full(n_docs, 10)


def flat_expected(n_docs, k, high=(), docs=None):
    high = sorted(int(x) for x in high)
    rest = [int(d) for d in (range(n_docs) if docs is None else docs) if int(d) not in set(high)]
    return (high + rest)[:k]


MERGE_TUNE = dict(fused=0, win=0, arith=0, dense_x1000=10**9, range_min_chunk=128, range_items=256)


def merge_form(cnt, surv, k):
    """merge_kernel's path through a query's lists, from what debug_lists returns: (form, round in which the 65th survivor came or
    None, rounds of 16 lists, survivors)"""
    if k > REG_K:
        return "lds", None, None, int(np.sum(surv))
    rounds = (len(cnt) + 15) // 16
    run, over = 0, None
    for r in range(rounds):
        run += int(np.sum(surv[16 * r:16 * r + 16]))
        if over is None and run > 64:
            over = r
    return ("ranked" if over is None else "register"), over, rounds, run


# --------------------------------------------------------------------------------------------------------------------------------
# D: the clamps -- every term in every document of a tiny index
# --------------------------------------------------------------------------------------------------------------------------------
def tiny_index(n_docs, n_terms=300):
    rng = np.random.default_rng(n_docs)
    lists = [(np.arange(n_docs), rng.integers(1, 5, n_docs)) for _ in range(n_terms)]
    return n_docs, lists, rng.integers(5, 40, n_docs)


# --------------------------------------------------------------------------------------------------------------------------------
# A: query sets beyond plan_kernel's 1024 threads
# --------------------------------------------------------------------------------------------------------------------------------
def big_queries(nq, n_terms, seed, holes=True):
    """nq queries of 1 .. 4 known terms.  holes: queries without postings -- empty, or of unknown terms only -- on the first and on the
    last slot of a thread's queries q0 .. q1 (one thread empty first and unknown last, one the other way round, one with its first
    two slots both without postings), and one 20-term query, which sends the batch over the general route.  Without holes every
    query has postings (the plan-free, one-launch and window routes need that)."""
    rng = np.random.default_rng(seed)
    queries = [sorted(int(x) for x in rng.choice(n_terms, rng.integers(1, 5), replace=False)) for _ in range(nq)]
    if holes:
        per, threads = plan_threads(nq)
        full = [t for t in range(PLAN_WG) if threads[t][1] - threads[t][0] == per]
        unknown = [n_terms + 3, n_terms + 70]
        a, b, c = full[1], full[len(full) // 2], full[-1]
        for t, first, last in ((a, [], unknown), (b, unknown, [])):
            q0, q1 = threads[t]
            queries[q0] = list(first)
            queries[q1 - 1] = list(last)   # (one query a thread: its only slot is first and last, and takes `last`)
        q0, q1 = threads[c]
        queries[q0] = []
        queries[min(q0 + 1, nq - 1)] = list(unknown)
        queries[nq // 5] = sorted(int(x) for x in rng.choice(n_terms, 20, replace=False))
    return queries


def hole_slots(queries, n_terms):
    """(position in its thread's q0 .. q1: "first" / "last" / "middle", kind: "empty" / "unknown") of every query without postings"""
    per, threads = plan_threads(len(queries))
    out = set()
    for q0, q1 in threads:
        for q in range(q0, q1):
            if not any(x < n_terms for x in queries[q]):
                pos = "first" if q == q0 else "last" if q == q1 - 1 else "middle"
                out.add((pos, "empty" if not queries[q] else "unknown"))
                if q1 - q0 == 1:
                    out.add(("last", "empty" if not queries[q] else "unknown"))
    return out
