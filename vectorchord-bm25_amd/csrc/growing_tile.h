// growing_tile.h -- where a term's postings of one tile of the growing segment lie.  Shared by growing.h (k <= 1024, search.hip) and
// growing_bigk.h (k > 1024, bigk.hip).
#ifndef VBM25_GROWING_TILE_H
#define VBM25_GROWING_TILE_H

#include <hip/hip_runtime.h>

#include "device_types.h"

namespace vbm25 {

// postings of term t with g in tile j
__device__ __forceinline__ uint2 grow_tile_range(const DevGrowing &G, uint32_t t, uint32_t j) {
    const uint32_t ti = G.tab_idx[t];
    if (ti != NONE32) return make_uint2(G.tab[ti + j], G.tab[ti + j + 1]);
    const uint32_t a = G.term_start[t], b = G.term_start[t + 1];
    auto lower = [&](uint32_t lo, uint32_t hi, uint64_t g) {
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (uint64_t(G.post_g[mid]) < g) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const uint32_t lo = j == 0 ? a : lower(a, b, uint64_t(j) * GT);
    const uint32_t hi = j + 1 >= G.n_tiles ? b : lower(lo, b, uint64_t(j + 1) * GT);
    return make_uint2(lo, hi);
}

}  // namespace vbm25

#endif
