// bigk_lane.h -- the per-entry functions of the sparse k > 1024 path (bigk.hip).  __host__ __device__, and plain C++ as well: the
// kernels of bigk.hip are loops over these, and tests/native/fuzz_bigk.cpp compiles the same text with g++ under AddressSanitizer and
// drives a select and a tile rank with them as a workgroup does, against std::sort / std::nth_element.
//
//   the order    a candidate is (key, doc): key = the bits of its f64 score (never 0: zeros are no hits), doc its document.  "a beats
//                b": key descending, then doc ascending.  The documents of one query are distinct, so the order is strict and every
//                select, sort and rank has one outcome whatever the arrival order.
//   the composite  that order as one 96-bit unsigned number, larger = better: the key's 64 bits, then the 32 bits of ~doc.  The
//                select reads it as 12 digits of 8 bits, most significant first (levels 0 .. 7 the key, 8 .. 11 the inverted doc).
//   digit / same_prefix / keeps   a candidate's digit at a level, whether its first `level` digits are the boundary's, and whether
//                its first `levels` digits are >= the boundary's (it survives)
//   walk_digits  one level of the select: from the histogram of the candidates that share the boundary's prefix, the boundary
//                digit, the candidates above it and whether the bucket holds exactly the missing count (the select stops)
//   count_beating   in a tile sorted best first, the entries that beat (key, doc): a bisection.  An entry's final rank is its index
//                in its own tile plus this count over every other tile of its query (the merge-by-rank idiom of live.hip).
//   item_windows the host's item cut: windows per work item
#ifndef VBM25_BIGK_LANE_H
#define VBM25_BIGK_LANE_H

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BGK_HD __host__ __device__ __forceinline__
#else
#define BGK_HD inline __attribute__((always_inline))
#endif

namespace vbm25 {
namespace bgk {

constexpr uint32_t WINDOW = 8192;          // documents of a window: 64 KB of f64 accumulators + 1 KB of touched bits in LDS
constexpr uint32_t WINDOW_WORDS = WINDOW / 64;
constexpr uint32_t SCAN_THREADS = 512;     // bigk_scan_kernel: 8 waves
constexpr uint32_t TERM_TABLE = 1024;      // entries of the LDS term table (MAX_TERMS): 16 KB
constexpr uint32_t TILE = 4096;            // entries a workgroup sorts in LDS: 48 KB
constexpr uint32_t LEVELS = 12;            // digits of the composite
constexpr uint32_t BINS = 256;
constexpr uint32_t MAX_TILES = 16;         // k <= 65535
constexpr uint64_t WORST_KEY = 0ull;       // loses against every candidate (a candidate's key is not 0): the padding of a sort
constexpr uint32_t WORST_DOC = 0xffffffffu;

BGK_HD bool beats(uint64_t a_key, uint32_t a_doc, uint64_t b_key, uint32_t b_doc) {
    return a_key > b_key || (a_key == b_key && a_doc < b_doc);
}

BGK_HD uint32_t digit(uint64_t key, uint32_t doc, uint32_t level) {
    return level < 8u ? uint32_t(key >> (56u - 8u * level)) & 255u : ((~doc) >> (24u - 8u * (level - 8u))) & 255u;
}

// the first `level` digits of (key, doc) are those of the boundary (b_key, b_doc); digits of the boundary below `level` are not read
BGK_HD bool same_prefix(uint64_t key, uint32_t doc, uint64_t b_key, uint32_t b_doc, uint32_t level) {
    if (level == 0u) return true;
    if (level < 8u) return (key >> (64u - 8u * level)) == (b_key >> (64u - 8u * level));
    if (key != b_key) return false;
    if (level == 8u) return true;
    const uint32_t s = 32u - 8u * (level - 8u);
    return ((~doc) >> s) == ((~b_doc) >> s);
}

// the first `levels` (1 .. 12) digits of (key, doc) are >= the boundary's
BGK_HD bool keeps(uint64_t key, uint32_t doc, uint64_t b_key, uint32_t b_doc, uint32_t levels) {
    if (levels <= 8u) return (key >> (64u - 8u * levels)) >= (b_key >> (64u - 8u * levels));
    if (key != b_key) return key > b_key;
    const uint32_t s = 32u - 8u * (levels - 8u);
    return ((~doc) >> s) >= ((~b_doc) >> s);
}

// the boundary with digit `d` written at `level` (the digits below stay whatever they were: nobody reads them)
BGK_HD void set_digit(uint64_t &b_key, uint32_t &b_doc, uint32_t level, uint32_t d) {
    if (level < 8u) {
        const uint32_t s = 56u - 8u * level;
        b_key = (b_key & ~(255ull << s)) | (uint64_t(d) << s);
    } else {
        const uint32_t s = 24u - 8u * (level - 8u);
        const uint32_t inv = ((~b_doc) & ~(255u << s)) | (d << s);
        b_doc = ~inv;
    }
}

// One level of the select.  hist: the digits at this level of the candidates that share the boundary's prefix; need (>= 1, <= their
// number): how many of them survive.  Returns the boundary digit; need becomes the survivors wanted from the boundary bucket and
// `exact` whether the bucket holds exactly that many (every one of them survives: the select stops).
BGK_HD uint32_t walk_digits(const uint32_t *hist, uint32_t &need, bool &exact) {
    uint32_t above = 0, d = BINS - 1u;
    for (;; --d) {
        if (above + hist[d] >= need || d == 0u) break;
        above += hist[d];
    }
    need -= above;
    exact = hist[d] == need;
    return d;
}

// tile[0 .. n) sorted best first (keys and docs apart): how many of its entries beat (key, doc)
BGK_HD uint32_t count_beating(const uint64_t *keys, const uint32_t *docs, uint32_t n, uint64_t key, uint32_t doc) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (beats(keys[mid], docs[mid], key, doc)) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// The host's item cut.  A work item is `wpi` consecutive windows of one query: the wanted cut (0: as many items as `target` in all,
// over n_q queries), doubled until the batch's items fit `cap`.
BGK_HD uint32_t item_windows(uint32_t n_win, uint32_t n_q, uint32_t wanted, uint32_t target, uint64_t cap) {
    if (n_win == 0u || n_q == 0u) return 1u;
    uint32_t wpi = wanted;
    if (wpi == 0u) {
        const uint32_t per_q = target / n_q ? target / n_q : 1u;
        wpi = (n_win + per_q - 1u) / per_q;
    }
    if (wpi == 0u) wpi = 1u;
    if (wpi > n_win) wpi = n_win;
    while (wpi < n_win && uint64_t(n_q) * ((n_win + wpi - 1u) / wpi) > cap) wpi = wpi * 2u > n_win ? n_win : wpi * 2u;
    return wpi;
}

}  // namespace bgk
}  // namespace vbm25

#endif
