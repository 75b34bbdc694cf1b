// forward_lane.h -- the per-lane functions of the forward index built from a sealed index (forward.hip): which sort a document's run of
// postings takes, and the compare-exchange schedule of that sort.  __host__ __device__, and plain C++ as well: the kernels of
// forward.hip are loops over these, and tests/native/fuzz_forward.cpp compiles the same text with g++ under AddressSanitizer and
// drives a model wave and a model workgroup with them, against std::sort.
//
//   run_class      a run of `len` postings under the two class bounds: RUN_WAVE (one wave, one element a lane, in registers),
//                  RUN_GROUP (one workgroup, in LDS) or RUN_LONG (the segmented radix sort).  A bound of 0 turns its class off.
//   padded_len     the bitonic network's size for a run: the least power of two >= len (and >= 2).  The elements behind the run
//                  are padding with the key PAD_TERM, which no term has and which sorts last.
//   slot_of        where a posting goes: its document's start plus the value its atomic add on the document's cursor returned
//   the network    stages k = 2, 4 .. P, in each the steps j = k / 2, k / 4 .. 1 (next_step walks them).  In step (k, j) element i
//                  meets element i ^ j; the lower of the two keeps the smaller key exactly when bit k of i is clear.
//       lane form  (a wave, element i in lane i): cx_partner is the lane to read, cx_take replaces the lane's own (key, value) by
//                  the partner's when the step gives it the partner's
//       pair form  (a workgroup, thread t owns pair t of P / 2): pair_low is the pair's lower element, pair_ascending its direction,
//                  pair_swaps whether the two trade places
//   Keys inside a run are distinct (a document holds a term once), so the sorted run does not depend on the order it arrived in;
//   equal keys -- the padding -- never trade places in either form.
#ifndef VBM25_FORWARD_LANE_H
#define VBM25_FORWARD_LANE_H

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FWD_HD __host__ __device__ __forceinline__
#else
#define FWD_HD inline __attribute__((always_inline))
#endif

namespace vbm25 {
namespace fwd {

constexpr uint32_t FWD_WAVE_MAX = 64;     // the wave class: one lane a posting
constexpr uint32_t FWD_GROUP_MAX = 2048;  // the workgroup class: 8 bytes of LDS a posting, 16 KiB a workgroup
constexpr uint32_t PAD_TERM = 0xffffffffu;

enum RunClass : uint32_t { RUN_WAVE = 0, RUN_GROUP = 1, RUN_LONG = 2 };

FWD_HD uint32_t run_class(uint64_t len, uint32_t wave_max, uint32_t group_max) {
    return len <= wave_max ? RUN_WAVE : len <= group_max ? RUN_GROUP : RUN_LONG;
}

FWD_HD uint32_t padded_len(uint32_t len) {
    uint32_t p = 2;
    while (p < len) p <<= 1;
    return p;
}

FWD_HD uint64_t slot_of(uint64_t doc_start, uint32_t cursor_before) { return doc_start + cursor_before; }

// the step behind (k, j); (k, j) = (2, 1) is the first, the network of P elements is over when k > P
FWD_HD void next_step(uint32_t &k, uint32_t &j) {
    j >>= 1;
    if (j == 0) {
        k <<= 1;
        j = k >> 1;
    }
}

FWD_HD uint32_t cx_partner(uint32_t i, uint32_t j) { return i ^ j; }
// element i keeps the smaller key of its pair: it is the pair's lower element in an ascending stretch, or the upper in a descending one
FWD_HD bool cx_keeps_min(uint32_t i, uint32_t k, uint32_t j) { return ((i & k) == 0) == ((i & j) == 0); }
FWD_HD void cx_take(uint32_t i, uint32_t k, uint32_t j, uint32_t &key, uint32_t &val, uint32_t pkey, uint32_t pval) {
    const bool take = cx_keeps_min(i, k, j) ? pkey < key : pkey > key;
    if (take) {
        key = pkey;
        val = pval;
    }
}

// pair t of step j: the element with bit j clear whose other bits are t's
FWD_HD uint32_t pair_low(uint32_t t, uint32_t j) { return ((t & ~(j - 1u)) << 1) | (t & (j - 1u)); }
FWD_HD bool pair_ascending(uint32_t low, uint32_t k) { return (low & k) == 0; }
FWD_HD bool pair_swaps(uint32_t key_low, uint32_t key_high, bool ascending) { return ascending ? key_low > key_high : key_low < key_high; }

}  // namespace fwd
}  // namespace vbm25

#endif
