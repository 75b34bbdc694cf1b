// growing_append.h -- the growing segment changed in place: vbm25_device_growing_append and vbm25_device_growing_delete.
// Included by growing.hip only (non-template kernels: one definition); key_cmp is growing_build.h's.
//
// The layout stays growing.h's (term-major post_g / post_c, term_start, tab_idx / tab, payload), so no search kernel knows about
// an append.  An append is a merge on the device.  The delta's elements become sorted (term << 32 | g) keys exactly as an upload's
// do, with g offset by the old n_grow.  Every g of the delta exceeds every old g, so delta posting j of term t belongs at the end
// of t's old list: its insertion point in the old array is ins[j] = term_start[t + 1], ins is ascending, and
//     delta posting j  -> ins[j] + j                          (the j delta postings before it are all inserted at or before it)
//     old posting i    -> i + #{j : ins[j] <= i}              (a binary search over the DELTA's insertion points, not the vocabulary)
//     term_start'[t]   =  term_start[t] + #{j : t_j < t}
// All of it is written into the segment's spare arrays, which the host swaps in when everything has succeeded.  The tile tables are
// rebuilt for the new n_tiles by upload's rule (grow_tab_kernel's entries, found by a search of post_g per table entry).
//
// A delete zeroes the c of the deleted documents' postings.  Live postings are positive (idf = ln((N + 1) / (df + 0.5)) > 0), so such
// a document sums to exactly 0.0: growing_scan_kernel admits only s > thr >= 0 and the k > 1024 path takes a zero key as no hit.
#ifndef VBM25_GROWING_APPEND_H
#define VBM25_GROWING_APPEND_H

#include "growing_build.h"

namespace vbm25 {

constexpr uint32_t GA_ITEMS = 4;  // old postings per thread of grow_append_move_kernel

// append 1: grow_map_kernel for a delta whose document i is growing document g0 + i.  One thread per ELEMENT (its document found
// by a search of start), so the usual delta of one document is mapped by a wave, not by a lane.
__global__ void __launch_bounds__(256) grow_append_map_kernel(const ulonglong2 *term_key, uint32_t n_terms, uint32_t n_delta, uint32_t g0,
                                                              const uint64_t *start, uint32_t n_el, const ulonglong2 *g_key,
                                                              const uint32_t *g_tf, const uint8_t *deleted, unsigned long long *keys,
                                                              uint32_t *vals, uint32_t *n_valid) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    bool found = false;
    if (e < n_el) {
        const uint64_t pos = start[0] + e;
        uint32_t d = 0, hi = n_delta;  // the last document with start[d] <= pos (the empty ones before it start there too)
        while (hi - d > 1) {
            const uint32_t mid = (d + hi) >> 1;
            if (start[mid] <= pos) d = mid; else hi = mid;
        }
        unsigned long long key = ~0ull;
        if (!(deleted && deleted[d])) {
            const ulonglong2 x = g_key[e];
            uint32_t lo = 0, th = n_terms;
            while (lo < th) {
                const uint32_t mid = (lo + th) >> 1;
                if (key_cmp(term_key[mid], x) < 0) lo = mid + 1; else th = mid;
            }
            if (lo < n_terms && key_cmp(term_key[lo], x) == 0) {
                key = (unsigned long long)lo << 32 | (g0 + d);
                found = true;
            }
        }
        keys[e] = key;
        vals[e] = g_tf[e];
    }
    const unsigned long long m = __ballot(found);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(n_valid, (uint32_t)__popcll(m));
}

// append 2: term_start'[t] for t = 0 .. n_terms: the old start plus the delta postings of the terms before t
__global__ void __launch_bounds__(256) grow_append_starts_kernel(const unsigned long long *keys, uint32_t n_delta_post, uint32_t n_terms,
                                                                 const uint32_t *term_start, uint32_t *new_start) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_terms) return;
    const unsigned long long first = (unsigned long long)t << 32;
    uint32_t lo = 0, hi = n_delta_post;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < first) lo = mid + 1; else hi = mid;
    }
    new_start[t] = term_start[t] + lo;
}

// append 3: the delta's postings behind their term's old ones, c exactly as grow_post_kernel computes it; ins[j] for the move
__global__ void __launch_bounds__(256) grow_append_post_kernel(const unsigned long long *keys, const uint32_t *tf, uint32_t n_delta_post,
                                                               uint32_t g0, const double *s0, const double *s1, const uint8_t *fieldnorm,
                                                               const uint32_t *term_start, uint32_t *ins, uint32_t *out_g, double *out_c) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_delta_post) return;
    const unsigned long long key = keys[j];
    const uint32_t t = uint32_t(key >> 32), g = uint32_t(key);
    const double f = (double)tf[j];
    const uint32_t at = term_start[t + 1];
    ins[j] = at;
    out_g[at + j] = g;
    out_c[at + j] = (f * s0[t]) / (f + s1[fieldnorm[g - g0]]);  // Cache::evaluate, bm25.rs:355-358
}

// append 4: the old postings move up by the number of delta postings inserted at or before them.  A workgroup's GA_ITEMS x 256
// consecutive postings bracket the search once (uniform loads); a posting then searches the few insertion points inside its block.
__global__ void __launch_bounds__(256) grow_append_move_kernel(const uint32_t *post_g, const double *post_c, uint32_t n_old,
                                                               const uint32_t *ins, uint32_t n_ins, uint32_t *out_g, double *out_c) {
    auto upper = [&](uint32_t lo, uint32_t hi, uint32_t i) {  // #{j : ins[j] <= i} given that it lies in [lo, hi]
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (ins[mid] <= i) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const uint32_t b0 = blockIdx.x * (256u * GA_ITEMS);  // (the grid covers n_old: b0 < n_old)
    const uint32_t b1 = min(n_old - b0, 256u * GA_ITEMS) - 1u + b0;
    const uint32_t lo_b = upper(0, n_ins, b0), hi_b = upper(lo_b, n_ins, b1);
#pragma unroll
    for (uint32_t r = 0; r < GA_ITEMS; ++r) {
        const uint32_t i = b0 + r * 256u + threadIdx.x;
        if (i < n_old) {
            const uint32_t p = i + upper(lo_b, hi_b, i);
            out_g[p] = post_g[i];
            out_c[p] = post_c[i];
        }
    }
}

// append 5: upload's rule for the tabled terms (at least n_tiles postings, n_tiles > 1) as the number of table entries per term,
// flags[n_terms] = 0: the exclusive sum over n_terms + 1 entries gives every table's first entry and, last, the total.  (Upload's
// NONE32 cap cannot bind: a tabled term has n_tiles >= 2 postings per n_tiles + 1 entries and there are fewer than 2^31 postings,
// so fewer than 3 x 2^30 entries.)
__global__ void __launch_bounds__(256) grow_append_flag_kernel(const uint32_t *new_start, uint32_t n_terms, uint32_t n_tiles,
                                                               uint32_t *flags) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_terms) return;
    flags[t] = t < n_terms && n_tiles > 1 && new_start[t + 1] - new_start[t] >= n_tiles ? n_tiles + 1u : 0u;
}

// append 6: tab_idx of every term, and per table its term
__global__ void __launch_bounds__(256) grow_append_tabidx_kernel(const uint32_t *flags, const uint32_t *offs, uint32_t n_terms,
                                                                 uint32_t n_tiles, uint32_t *tab_idx, uint32_t *tab_term) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_terms) return;
    const bool tabled = flags[t] != 0;
    tab_idx[t] = tabled ? offs[t] : NONE32;
    if (tabled) tab_term[offs[t] / (n_tiles + 1u)] = t;
}

// append 7: table entry e = (table e / (n_tiles + 1), tile boundary u = e % (n_tiles + 1)): the term's first posting with g >= u GT
__global__ void __launch_bounds__(256) grow_append_tab_kernel(const uint32_t *tab_term, uint32_t n_tab, uint32_t n_tiles,
                                                              const uint32_t *new_start, const uint32_t *post_g, uint32_t *tab) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_tab) return;
    const uint32_t t = tab_term[e / (n_tiles + 1u)], u = e % (n_tiles + 1u);
    const uint64_t g = uint64_t(u) * GT;
    uint32_t lo = new_start[t], hi = new_start[t + 1];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (uint64_t(post_g[mid]) < g) lo = mid + 1; else hi = mid;
    }
    tab[e] = lo;
}

// delete 1: the indices -> a bitmap of n_grow bits (zeroed by the caller; the indices were checked on the host)
__global__ void __launch_bounds__(256) grow_delete_bits_kernel(const uint32_t *g, uint32_t n, uint32_t *bits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicOr(&bits[g[i] >> 5], 1u << (g[i] & 31u));
}

// delete 2: one pass over the postings; those of a deleted document score nothing from now on
__global__ void __launch_bounds__(256) grow_delete_kernel(const uint32_t *post_g, uint32_t n_post, const uint32_t *bits, double *post_c) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_post) return;
    const uint32_t g = post_g[i];
    if ((bits[g >> 5] >> (g & 31u)) & 1u) post_c[i] = 0.0;
}

}  // namespace vbm25

#endif
