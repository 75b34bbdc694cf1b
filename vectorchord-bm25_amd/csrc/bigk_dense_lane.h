// bigk_dense_lane.h -- the per-lane functions of the dense half of the k > 1024 route (bigk_dense.h, launched by bigk.hip): an MSD radix
// select of a query's k-th entry whose histograms are made by scanning postings, not a stored list.  __host__ __device__, and plain
// C++ as well: tests/native/fuzz_bigk_dense.cpp compiles the same text with g++ under AddressSanitizer and drives histogram -> walk ->
// next interval with it as the kernels do, against std::nth_element.
//
//   the composite  bigk_lane.h's order ("key descending, doc ascending") as one 96-bit unsigned number, larger = better: the key's 64
//                bits, then the 32 bits of ~doc; carried as unsigned __int128.
//   State        a query's search: the closed interval [lo, top] of the composite that holds its k-th entry, `above` = the entries
//                better than top (always < k), the shift that cuts the interval into at most BINS bins, the level, and settled.
//   bin_of       an entry's bin: (top - c) >> shift, bin 0 the best; whatever lies further down is clipped into the last bin.
//   level 0      top = (K_ub, doc 0) with K_ub the bits of the sum of the query's s0 (no score exceeds it) and shift = 44 + 32: bin
//                i < BINS - 1 holds the keys with (K_ub - key) >> 44 == i -- 1/256 of an octave, 16 octaves below the bound -- and the
//                clip bin everything lower.
//   later levels the boundary bin becomes the interval and its shift follows from its size: 12 bits a level.  An ordinary level-0 bin
//                is 2^76 wide: 76 -> 64 -> 52 -> 40 -> 28 -> 16 -> 4 -> 0 bits, eight levels in all; the clip bin is below 2^95 (a
//                positive f64's key has no sign bit): 95 -> 83 -> ... -> 11 -> 0, NINE levels in all (MAX_LEVELS).  An interval of
//                one value holds at most one entry (a query's documents are distinct), so the last level always settles.
//   walk / walk_grouped   the first bin from the top at which the running count reaches `need`
//   decide       a level's outcome from the histogram's walk: everything fits the capacity -- settled with lo = 0; the boundary bin
//                fits on top of `above` and the bins before it -- settled with lo at the bin's lower edge; otherwise `above` takes the
//                bins before it and the bin is the next interval.
#ifndef VBM25_BIGK_DENSE_LANE_H
#define VBM25_BIGK_DENSE_LANE_H

#include <cstdint>

#include "bigk_lane.h"

namespace vbm25 {
namespace bgd {

typedef unsigned __int128 u128;

constexpr uint32_t DIGIT = 12;
constexpr uint32_t BINS = 1u << DIGIT;       // 16 KB of LDS
constexpr uint32_t CLIP = BINS - 1u;
constexpr uint32_t L0_SHIFT = 44u + 32u;     // level 0: 2^44 of the key a bin
constexpr uint32_t MAX_LEVELS = 9;
constexpr uint32_t WALK_GROUP = 16;          // bins a thread of the walk sums
constexpr uint32_t WALK_THREADS = BINS / WALK_GROUP;
constexpr uint64_t KUB_ALL = 0x7ff0000000000000ull;  // the bound of a query whose s0 the host does not trust: above every finite score

struct State {
    uint64_t lo_key, top_key;
    uint32_t lo_inv, top_inv;
    uint32_t shift, above, level, settled;
};

BGK_HD u128 composite(uint64_t key, uint32_t doc) { return (u128(key) << 32) | u128(uint32_t(~doc)); }
BGK_HD u128 lo_of(const State &s) { return (u128(s.lo_key) << 32) | s.lo_inv; }
BGK_HD u128 top_of(const State &s) { return (u128(s.top_key) << 32) | s.top_inv; }
BGK_HD void set_lo(State &s, u128 v) { s.lo_key = uint64_t(v >> 32), s.lo_inv = uint32_t(v); }
BGK_HD void set_top(State &s, u128 v) { s.top_key = uint64_t(v >> 32), s.top_inv = uint32_t(v); }

BGK_HD uint32_t bit_length(u128 v) {
    const uint64_t hi = uint64_t(v >> 64), lo = uint64_t(v);
    if (hi) return 128u - uint32_t(__builtin_clzll(hi));
    return lo ? 64u - uint32_t(__builtin_clzll(lo)) : 0u;
}

// the shift that cuts an interval of `span` + 1 values into at most BINS bins
BGK_HD uint32_t shift_for(u128 span) {
    const uint32_t bl = bit_length(span);
    return bl > DIGIT ? bl - DIGIT : 0u;
}

BGK_HD State level0(uint64_t k_ub) {
    State s{};
    s.top_key = k_ub;
    s.top_inv = 0xffffffffu;
    s.shift = L0_SHIFT;
    return s;
}

BGK_HD bool inside(u128 c, u128 lo, u128 top) { return c >= lo && c <= top; }

// c <= top
BGK_HD uint32_t bin_of(u128 c, u128 top, uint32_t shift) {
    const u128 d = (top - c) >> shift;
    return d < u128(CLIP) ? uint32_t(d) : CLIP;
}

// the lower edge of bin d of the state's interval (the last bin, and the clip bin of level 0, reach down to lo)
BGK_HD u128 bin_lo(const State &s, uint32_t d) {
    const u128 lo = lo_of(s), top = top_of(s), span = u128(d + 1u) << s.shift;
    return d == CLIP || span > top - lo ? lo : top - span + 1u;
}
BGK_HD u128 bin_top(const State &s, uint32_t d) { return top_of(s) - (u128(d) << s.shift); }

// the first d in [0, n) with h[0] + .. + h[d] >= need (n when none); before = h[0] + .. + h[d - 1]
BGK_HD uint32_t walk(const uint32_t *h, uint32_t n, uint64_t need, uint64_t &before) {
    uint32_t d = 0;
    before = 0;
    for (; d < n; ++d) {
        if (before + h[d] >= need) break;
        before += h[d];
    }
    return d;
}

// the same over BINS bins with gsum[g] the sum of bins [g WALK_GROUP, (g + 1) WALK_GROUP): the groups first, then inside one
BGK_HD uint32_t walk_grouped(const uint32_t *hist, const uint32_t *gsum, uint64_t need, uint64_t &before) {
    const uint32_t g = walk(gsum, WALK_THREADS, need, before);
    if (g == WALK_THREADS) return BINS;
    uint64_t in = 0;
    const uint32_t d = walk(hist + g * WALK_GROUP, WALK_GROUP, need - before, in);
    before += in;
    return g * WALK_GROUP + d;
}

// A level's outcome.  total: the entries the scan counted in the interval; d, before: walk's answer for need = k - above; hd = hist[d]
// (d < BINS).  Returns whether the level-0 boundary was the clip bin.
BGK_HD bool decide(State &s, uint32_t k, uint32_t cap, uint64_t total, uint32_t d, uint64_t before, uint32_t hd) {
    if (s.level == 0u && total <= cap) {  // everything is a candidate (lo = 0)
        s.settled = 1u;
        return false;
    }
    if (d >= BINS) {  // (fewer than k in all: level 0 and total < k <= cap, taken above)
        s.settled = 1u;
        return false;
    }
    const bool clip = s.level == 0u && d == CLIP;
    const u128 nlo = bin_lo(s, d);
    if (uint64_t(s.above) + before + hd <= cap) {
        set_lo(s, nlo);
        s.settled = 1u;
        return clip;
    }
    const u128 ntop = bin_top(s, d);
    set_top(s, ntop);
    set_lo(s, nlo);
    s.above += uint32_t(before);
    s.shift = shift_for(ntop - nlo);
    ++s.level;
    return clip;
}

}  // namespace bgd
}  // namespace vbm25

#endif
