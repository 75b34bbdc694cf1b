// dense_list_lane.h -- the per-lane functions of scan_dense_kernel's SURVIVOR LIST (256 < k <= 1024: one list of exactly re-scored
// documents per workgroup in LDS, scan_dense.h).  __host__ __device__, and plain C++ as well: the kernel's append and cut are loops over
// these, and tests/native/fuzz_dense_big.cpp compiles the same text with g++ under AddressSanitizer and drives a buffer with them as
// the eight waves do, against std::partial_sort.
//
//   entry        (key, doc): key = the bits of the document's exact f64 score.  Scores are positive, so the bits order as the scores
//                do; the order of the result is rrk::better -- key descending, then doc ascending (rerank_lane.h).
//   CAP          entries of the buffer: 2 x 1024, 24 KB.  After a cut at most k <= 1024 are live, so at least 1024 appends fit before
//                the next one.
//   keeps        an entry the threshold does not strictly beat stays (equal scores stay: the doc order decides among them at the cut)
//   fits         a lane's slot is rrk::offer_slot: the wave's base (one atomic add of the count on the cursor) plus the lane's rank in
//                the ballot.  fits(slot) is false past the buffer: nothing is written, the item is given up.
//   sort_entries the power of two (>= 16: eight waves of at least one pair) a sort of n live entries runs over; [n_live, that) is padded
//                with PAD, which loses against every entry
//   wave_pairs / stage_local / wave_pair   wave w of the eight owns the pairs [w n / 16, (w + 1) n / 16) of a stage of the bitonic
//                network (rrk::bitonic_pair: n / 2 pairs a stage).  While the stride is at most n / 16 those pairs lie inside the
//                wave's own n / 8 entries -- the stage needs no workgroup barrier, only the wave's own order.
//   cut_count    live entries behind a cut: the first k
#ifndef VBM25_DENSE_LIST_LANE_H
#define VBM25_DENSE_LIST_LANE_H

#include "rerank_lane.h"

namespace vbm25 {
namespace dlist {

constexpr uint32_t MAX_K = 1024;
constexpr uint32_t CAP = 2 * MAX_K;
constexpr uint32_t WAVES = 8;
constexpr uint64_t PAD_KEY = 0ull;
constexpr uint32_t PAD_DOC = 0xffffffffu;

RRK_HD bool keeps(uint64_t key, uint64_t theta) { return key != PAD_KEY && key >= theta; }

RRK_HD bool fits(uint32_t slot) { return slot < CAP; }

RRK_HD uint32_t sort_entries(uint32_t n_live) { return rrk::pow2_ceil(n_live < 2u * WAVES ? 2u * WAVES : n_live); }

RRK_HD uint32_t wave_pairs(uint32_t n) { return n / (2u * WAVES); }
RRK_HD bool stage_local(uint32_t stride, uint32_t n) { return stride <= wave_pairs(n); }
// pair p (< wave_pairs(n)) of wave w in the stage (size, stride): the entries i < j and whether the better one belongs at i
RRK_HD void wave_pair(uint32_t w, uint32_t p, uint32_t n, uint32_t size, uint32_t stride, uint32_t &i, uint32_t &j, bool &best_first) {
    rrk::bitonic_pair(w * wave_pairs(n) + p, stride, i, j);
    best_first = rrk::bitonic_best_first(i, size);
}

RRK_HD uint32_t cut_count(uint32_t n_live, uint32_t k) { return n_live < k ? n_live : k; }

}  // namespace dlist
}  // namespace vbm25

#endif
