// live_shared.h -- what live.hip (the kernels that keep the rerank stack up with a live table) offers reranker.hip
// (vbm25_reranker_sync): the sort of a small delta of ctids in LDS, the merge by rank of a sorted delta into the sorted directory
// keys, and the live_sort_max switch between that sort and the radix sort.  The per-lane functions are tid_lane.h's.  HIP-only, not
// part of the ABI.
#ifndef VBM25_LIVE_SHARED_H
#define VBM25_LIVE_SHARED_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tid_lane.h"

namespace vbm25 {
namespace live {

// the most rows one workgroup sorts in LDS (32 KB of words); live_sort_max of vbm25_tuning_set is at most this
constexpr uint32_t LIVE_SORT_CAP = 1u << tid::LIVE_SORT_LOG2;
// live_sort_max as it stands: a delta of up to this many rows takes live_sort_kernel, a larger one the radix sort (0: always the radix sort)
uint32_t live_sort_max_now();

// payload: m x 3 uint16_t, the ctids of documents first_doc .. first_doc + m (1 <= m <= LIVE_SORT_CAP) -> keys[m] ascending with
// docs[m] beside them, equal keys in ascending document order.  One workgroup.
hipError_t launch_live_sort(const uint16_t *payload, uint32_t m, uint32_t first_doc, unsigned long long *keys, uint32_t *docs, hipStream_t stream);

struct MergeArgs {
    const unsigned long long *keys;  // the n_old sorted keys, their documents and the directory over them
    const uint32_t *docs;
    unsigned long long n_old;
    const unsigned long long *dir;
    uint32_t n_dir, stride;
    const unsigned long long *delta_keys;  // the n_delta sorted keys of the new documents (every one above every old document)
    const uint32_t *delta_docs;
    unsigned long long n_delta;
    unsigned long long *out_keys;  // n_old + n_delta
    uint32_t *out_docs;
};
// one lane an entry, old or new, each to its rank (tid_lane.h: live_rank_old, live_rank_delta); the grid capped by eval_grid
hipError_t launch_live_merge(const MergeArgs &a, hipStream_t stream);

}  // namespace live
}  // namespace vbm25

#endif
