// rerank_lane.h -- the per-lane and per-entry functions of the top-k selection over `<&>` scores (rerank.hip).  __host__ __device__,
// and plain C++ as well: the kernels of rerank.hip are loops over these, and tests/native/fuzz_rerank.cpp compiles the same text with
// g++ under AddressSanitizer and drives a buffer with them as a workgroup does, against std::stable_sort.
//
//   score_key / key_score   a double's bits as an unsigned integer that orders as the double does (the sign bit flipped for positive
//                values, every bit for negative ones) and back.  Scores here are sums of non-negative terms -- the idf is
//                ln((N + 1) / (df + 0.5)) with df <= N -- so the plain bits would order already; the sign-aware form costs two
//                instructions and holds for whatever tables an index was made from.  A NaN has no place in the order and no index
//                produces one.
//   better       the whole order of the result: score descending, then pos ascending.  Positions within one query are distinct, so
//                any two entries of a query compare unequal and every sort, cut and merge has one outcome whatever the arrival order.
//   WORST        loses against every entry a kernel can make (a pos is below 2^31): the threshold before the first cut, the padding
//                of a sort
//   buffer_entries   the entries of the selection buffer for k and the tuning multiple: a power of two (the bitonic network's size),
//                at least 2k, at least one round of the workgroup's offers, at most MAX_BUFFER
//   offer_slot   the buffer index of a wave's lane among the lanes that offer: the wave's base (one atomic add of the offer count)
//                plus the lane's rank in the ballot.  A slot >= the buffer's size is not written: the lane keeps its entry, the
//                workgroup cuts, the lane offers again (a wave can offer 64 entries to a buffer with fewer free slots).
//   sort_entries the power of two a sort of n live entries runs over
//   bitonic_pair / bitonic_best_first   the compare-exchange schedule: for size = 2, 4 .. n, for stride = size / 2 .. 1, exchange t of
//                n / 2 works on the pair (i, i + stride) and leaves the better entry at i when bitonic_best_first(i, size)
//   exchange     one compare-exchange on two entries
#ifndef VBM25_RERANK_LANE_H
#define VBM25_RERANK_LANE_H

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RRK_HD __host__ __device__ __forceinline__
#else
#define RRK_HD inline __attribute__((always_inline))
#endif

namespace vbm25 {
namespace rrk {

constexpr uint32_t MAX_K = 1024;         // the limit of the search's general path
constexpr uint32_t ROUND = 256;          // the offers of one round: one a thread of the workgroup
constexpr uint32_t MAX_BUFFER = 4096;    // entries: 48 KB of LDS
constexpr uint32_t MIN_MULTIPLE = 2, MAX_MULTIPLE = 8;

struct Entry {
    uint64_t key;  // score_key of the score
    uint32_t pos;  // the candidate's index within its query's list
};

constexpr uint64_t WORST_KEY = 0ull;
constexpr uint32_t WORST_POS = 0xffffffffu;
constexpr Entry WORST{WORST_KEY, WORST_POS};

RRK_HD uint64_t score_key(uint64_t bits) { return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull; }
RRK_HD uint64_t key_score(uint64_t key) { return (key >> 63) ? key & 0x7fffffffffffffffull : ~key; }

RRK_HD bool better(uint64_t a_key, uint32_t a_pos, uint64_t b_key, uint32_t b_pos) { return a_key > b_key || (a_key == b_key && a_pos < b_pos); }
RRK_HD bool better(const Entry &a, const Entry &b) { return better(a.key, a.pos, b.key, b.pos); }

RRK_HD uint32_t pow2_ceil(uint32_t n) {
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

RRK_HD uint32_t buffer_entries(uint32_t k, uint32_t multiple) {
    const uint32_t m = multiple < MIN_MULTIPLE ? MIN_MULTIPLE : multiple > MAX_MULTIPLE ? MAX_MULTIPLE : multiple;
    const uint32_t want = pow2_ceil(k * m < ROUND ? ROUND : k * m);
    return want > MAX_BUFFER ? MAX_BUFFER : want;  // (k <= 1024: never under 2k)
}

RRK_HD uint32_t rank_in(uint64_t ballot, uint32_t lane) {
    uint64_t below = ballot & ((1ull << lane) - 1ull);
    uint32_t n = 0;
    for (; below; below &= below - 1ull) ++n;
    return n;
}
// the device counts the bits in one instruction; `rank` is rank_in(ballot, lane) either way
RRK_HD uint32_t offer_slot(uint32_t base, uint32_t rank) { return base + rank; }

RRK_HD uint32_t sort_entries(uint32_t n_live) { return pow2_ceil(n_live < 2u ? 2u : n_live); }

RRK_HD void bitonic_pair(uint32_t t, uint32_t stride, uint32_t &i, uint32_t &j) {
    i = 2u * t - (t & (stride - 1u));
    j = i + stride;
}
RRK_HD bool bitonic_best_first(uint32_t i, uint32_t size) { return (i & size) == 0u; }

RRK_HD void exchange(uint64_t &a_key, uint32_t &a_pos, uint64_t &b_key, uint32_t &b_pos, bool best_first) {
    // best_first: a must not lose to b; else b must not lose to a
    const bool swap = best_first ? better(b_key, b_pos, a_key, a_pos) : better(a_key, a_pos, b_key, b_pos);
    if (swap) {
        const uint64_t k = a_key;
        const uint32_t p = a_pos;
        a_key = b_key;
        a_pos = b_pos;
        b_key = k;
        b_pos = p;
    }
}

}  // namespace rrk
}  // namespace vbm25

#endif
