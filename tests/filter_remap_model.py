"""A numpy restatement of vbm25_filter_remap, independent of the device code: the filter of a compacted index is, per bitmap, the old
sealed bitmap's bits of the kept sealed documents followed by the old growing bitmap's bits of the live growing documents, packed
as a filter packs (bit d % 64 of word d / 64, least significant first).  remap_words is that concatenation; remap_by_relabel
permutes through a relabel array (vbm25_index_maintain's, maintain_model.maintain's) instead; remap_word_scheme restates the
device kernel's word-level scheme (keep words, popcount scan, compress, OR at a bit offset) in Python integers."""
import numpy as np

NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1


def pack_bits(bits):
    """bool [F, n] -> uint64 [F, ceil(n / 64)]"""
    bits = np.asarray(bits, bool)
    f, n = bits.shape
    padded = np.zeros((f, 64 * ((n + 63) // 64)), bool)
    padded[:, :n] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little").view("<u8")).reshape(f, (n + 63) // 64)


def unpack_bits(words, n):
    """uint64 [F, ceil(n / 64)] -> bool [F, n]"""
    words = np.ascontiguousarray(words, "<u8").reshape(len(words), -1)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool)[:, :n]


def _flags(deleted, n):
    return np.zeros(n, bool) if deleted is None else np.asarray(deleted).astype(bool)


def remap_bits(bits_sealed, sealed_deleted=None, bits_growing=None, growing_deleted=None):
    """bool [F, N], bool [N] / None, bool [F, G] / None, flags [G] / None -> bool [F, kept + live]"""
    bits_sealed = np.asarray(bits_sealed, bool)
    out = bits_sealed[:, ~_flags(sealed_deleted, bits_sealed.shape[1])]
    if bits_growing is not None:
        bits_growing = np.asarray(bits_growing, bool)
        out = np.concatenate([out, bits_growing[:, ~_flags(growing_deleted, bits_growing.shape[1])]], axis=1)
    return out


def remap_words(bits_sealed, sealed_deleted=None, bits_growing=None, growing_deleted=None):
    return pack_bits(remap_bits(bits_sealed, sealed_deleted, bits_growing, growing_deleted))


def remap_by_relabel(bits_sealed, bits_growing, relabel, n_new):
    """the same through a relabel array: old sealed ids, then growing indexes -> new id or NONE"""
    old = np.asarray(bits_sealed, bool)
    if bits_growing is not None:
        old = np.concatenate([old, np.asarray(bits_growing, bool)], axis=1)
    relabel = np.asarray(relabel, np.int64)
    assert len(relabel) == old.shape[1]
    kept = relabel != NONE
    new = np.zeros((len(old), n_new), bool)
    new[:, relabel[kept]] = old[:, kept]
    return pack_bits(new)


def compress64(x, m):
    """the bits of x under mask m moved to the low end, in order (Hacker's Delight 7-4: six move masks from m alone)"""
    mk = (~m << 1) & M64
    x &= m
    for i in range(6):
        mp = mk ^ ((mk << 1) & M64)
        for s in (2, 4, 8, 16, 32):
            mp ^= (mp << s) & M64
        mv = mp & m
        m = (m ^ mv) | (mv >> (1 << i))
        t = x & mv
        x = (x ^ t) | (t >> (1 << i))
        mk &= ~mp & M64
    return x


def remap_word_scheme(words_sealed, n_docs, sealed_deleted, words_growing, n_grow, growing_deleted):
    """uint64 [F, W] (+ [F, GW]) -> uint64 [F, ceil(n_new / 64)] the way the kernel does it, one input word at a time"""
    F = len(words_sealed)
    keep, src = [], []
    for words, n, deleted in ((words_sealed, n_docs, sealed_deleted), (words_growing, n_grow, growing_deleted)):
        if not n:
            continue
        dw = pack_bits(_flags(deleted, n)[None])[0]
        for w in range((n + 63) // 64):
            k = ~int(dw[w]) & M64
            if w + 1 == (n + 63) // 64 and n % 64:
                k &= (1 << (n % 64)) - 1  # the tail word's keep bits masked
            keep.append(k)
            src.append([int(words[f][w]) for f in range(F)])
    base = np.r_[0, np.cumsum([bin(k).count("1") for k in keep])].astype(np.int64)
    n_new = int(base[-1])
    out = [[0] * ((n_new + 63) // 64) for _ in range(F)]
    for w, k in enumerate(keep):
        if not k:
            continue
        ow, sh = int(base[w]) >> 6, int(base[w]) & 63
        for f in range(F):
            c = compress64(src[w][f], k)
            assert c < (1 << bin(k).count("1"))
            if not c:
                continue
            out[f][ow] |= (c << sh) & M64
            if sh and (c >> (64 - sh)):  # (sh == 0: the word takes all 64 bits)
                out[f][ow + 1] |= c >> (64 - sh)
    return np.array(out, np.uint64).reshape(F, (n_new + 63) // 64)


def deletion_patterns(n, rng):
    """name -> bool [n] (True = deleted): the shapes of tests/test_gpu_filter_remap.py"""
    p = {"none": np.zeros(n, bool)}
    p["all_but_first"] = np.arange(n) != 0
    p["all_but_last"] = np.arange(n) != n - 1
    p["every_other"] = np.arange(n) % 2 == 1
    r = np.zeros(n, bool)  # a range that empties at least three whole words (where the corpus has that many)
    r[n // 3: n // 3 + max(4 * 64, n // 5)] = True
    p["range"] = r
    for rate in (0.01, 0.5, 0.99):
        p[f"random_{rate}"] = rng.random(n) < rate
    return p
