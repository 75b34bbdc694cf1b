// growing_build.h -- vbm25_growing_upload on the device: the CSR of the growing documents -> the inverted form growing.h describes.
// Included by growing.hip only (non-template kernels: one definition).
#ifndef VBM25_GROWING_BUILD_H
#define VBM25_GROWING_BUILD_H

#include "device_types.h"

namespace vbm25 {

// 16-byte token keys compare as memcmp: two big-endian 64-bit words
__device__ __forceinline__ int key_cmp(const ulonglong2 a, const ulonglong2 b) {
    const unsigned long long a0 = __builtin_bswap64(a.x), b0 = __builtin_bswap64(b.x);
    if (a0 != b0) return a0 < b0 ? -1 : 1;
    const unsigned long long a1 = __builtin_bswap64(a.y), b1 = __builtin_bswap64(b.y);
    return a1 < b1 ? -1 : a1 > b1 ? 1 : 0;
}

// upload 1: per element of a live document the sort key (term id << 32 | g), ~0 for a key the sealed segment lacks or a deleted
// document; the value is the element's tf.  `n_valid` counts the postings.
__global__ void __launch_bounds__(256) grow_map_kernel(const ulonglong2 *term_key, uint32_t n_terms, uint32_t n_grow,
                                                       const uint64_t *start, const ulonglong2 *g_key, const uint32_t *g_tf,
                                                       const uint8_t *deleted, unsigned long long *keys, uint32_t *vals,
                                                       uint32_t *n_valid) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_grow) return;
    const uint64_t e0 = start[g] - start[0], e1 = start[g + 1] - start[0];
    const bool live = !(deleted && deleted[g]);
    uint32_t found = 0;
    for (uint64_t e = e0; e < e1; ++e) {
        unsigned long long key = ~0ull;
        if (live) {
            const ulonglong2 x = g_key[e];
            uint32_t lo = 0, hi = n_terms;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (key_cmp(term_key[mid], x) < 0) lo = mid + 1; else hi = mid;
            }
            if (lo < n_terms && key_cmp(term_key[lo], x) == 0) {
                key = (unsigned long long)lo << 32 | g;
                ++found;
            }
        }
        keys[e] = key;
        vals[e] = g_tf[e];
    }
    if (found) atomicAdd(n_valid, found);
}

// upload 2: the sorted postings -> (g, c) and the term starts.  c exactly as the host's Cache::evaluate (-ffp-contract=off).
__global__ void __launch_bounds__(256) grow_post_kernel(const unsigned long long *keys, const uint32_t *tf, uint32_t n_post,
                                                        uint32_t n_terms, const double *s0, const double *s1, const uint8_t *fieldnorm,
                                                        uint32_t *post_g, double *post_c, uint32_t *term_start) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_post) return;
    const unsigned long long key = keys[i];
    const uint32_t t = uint32_t(key >> 32), g = uint32_t(key);
    const double f = (double)tf[i];
    post_g[i] = g;
    post_c[i] = (f * s0[t]) / (f + s1[fieldnorm[g]]);  // Cache::evaluate, bm25.rs:355-358
    const uint32_t tp = i ? uint32_t(keys[i - 1] >> 32) : 0u;
    for (uint32_t u = i ? tp + 1 : 0u; u <= t; ++u) term_start[u] = i;  // (the terms without postings before t start here too)
    if (i + 1 == n_post)
        for (uint32_t u = t + 1; u <= n_terms; ++u) term_start[u] = n_post;
}

// upload 3: the tile tables of the terms with at least n_tiles postings
__global__ void __launch_bounds__(256) grow_tab_kernel(const unsigned long long *keys, uint32_t n_post, DevGrowing G, uint32_t *tab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_post) return;
    const uint32_t t = uint32_t(keys[i] >> 32);
    const uint32_t ti = G.tab_idx[t];
    if (ti == NONE32) return;
    const uint32_t p0 = G.term_start[t], p1 = G.term_start[t + 1];
    const uint32_t j = G.post_g[i] / GT;
    const uint32_t jp = i == p0 ? 0u : G.post_g[i - 1] / GT + 1u;
    for (uint32_t u = jp; u <= j; ++u) tab[ti + u] = i;
    if (i + 1 == p1)
        for (uint32_t u = j + 1; u <= G.n_tiles; ++u) tab[ti + u] = p1;
}

}  // namespace vbm25

#endif
