// rerank_shared.h -- what rerank.hip (the scorer handle) and reranker.hip (the reranker ring) have in common: the arguments of the
// fused score-and-select kernels, the plan of a batch's units, and the launch.  The kernels live in rerank.hip; both callers select
// through them from the same plan.  HIP-only, not part of the ABI.
#ifndef VBM25_RERANK_SHARED_H
#define VBM25_RERANK_SHARED_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "evaluate_shared.h"
#include "rerank_lane.h"

namespace vbm25 {
namespace rrk {

// a cand_doc entry that names no document (a ctid the payload directory lacks): the entry is not eligible, its pos still counts
constexpr uint32_t NO_DOC = 0xFFFFFFFFu;

// What a unit reads once at its start (the first three) and where its result goes (the rest): fetched from the staged block where
// they are used, so that these pointers do not sit in scalar registers through the scoring loop (with all of them as kernel
// arguments the compiler spilled eleven SGPRs)
struct TopkOut {
    const uint32_t *unit_start;        // nq + 1: query q owns units unit_start[q] .. unit_start[q + 1], at least one
    const uint32_t *q_off;             // = ScoreArgs::q_off
    const unsigned long long *q_cand;  // = ScoreArgs::q_cand
    const uint32_t *scr_start;         // nq: the first part list of a query of several units
    unsigned long long *scr_key;       // part lists: k entries each, best first
    uint32_t *scr_pos, *scr_cnt;
    vbm25_rank *ranks;
    uint32_t *n_ranks;
};

struct TopkArgs {
    evl::ScoreArgs s;             // (item_start and scores unused)
    const uint32_t *multi_q;      // n_multi: the queries of several units
    const TopkOut *out;
    uint32_t n_units, n_multi, k, buf, part;
    // the handle's deletion bitmap as the call found it (NULL: nobody deleted from the handle): a candidate whose document's bit is
    // set is not eligible, as a NO_DOC entry is not
    const unsigned long long *dead;
};

// The units of a batch: a scan of the parts per query, at least one a query; the queries of several parts get part lists.  They
// depend on the candidate counts only.
struct UnitPlan {
    uint32_t n_units = 0, n_multi = 0, n_lists = 0;
};
inline uint32_t parts_of(const uint64_t *q_cand, uint32_t n_docs, uint32_t part, uint32_t q) {
    const uint64_t n = q_cand ? q_cand[q + 1] - q_cand[q] : n_docs;
    return uint32_t(std::max<uint64_t>(1, (n + part - 1) / part));
}
inline UnitPlan count_units(const uint64_t *q_cand, uint32_t n_docs, uint32_t part, uint32_t nq) {
    UnitPlan u;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t p = parts_of(q_cand, n_docs, part, q);
        u.n_units += p;
        if (p > 1) ++u.n_multi, u.n_lists += p;
    }
    return u;
}
// unit_start and scr_start: nq + 1 entries each; multi_q: n_multi
inline void fill_units(const uint64_t *q_cand, uint32_t n_docs, uint32_t part, uint32_t nq, uint32_t *unit_start, uint32_t *scr_start,
                       uint32_t *multi_q) {
    unit_start[0] = 0;
    uint32_t m = 0, l = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t p = parts_of(q_cand, n_docs, part, q);
        unit_start[q + 1] = unit_start[q] + p;
        scr_start[q] = l;
        if (p > 1) multi_q[m++] = q, l += p;
    }
    scr_start[nq] = l;
}
// the bytes of n_lists part lists of k entries: keys, positions, counts
inline size_t part_list_bytes(uint64_t n_lists, uint32_t k) { return size_t(12ull * n_lists * k + 4ull * n_lists); }

// rerank_part and rerank_buf of vbm25_tuning_set as they stand
uint32_t rerank_part_now();
uint32_t rerank_buf_now();
// rerank_part_kernel, then rerank_merge_kernel when a.n_multi != 0, on `stream`; the grids capped by eval_grid as read now
hipError_t launch_topk(const TopkArgs &a, hipStream_t stream);

}  // namespace rrk
}  // namespace vbm25

#endif
