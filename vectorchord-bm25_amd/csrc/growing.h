// growing.h -- the growing (unsealed) segment at query time: the scan and the merge (the upload kernels: growing_build.h).
// Included by search.hip only (non-template kernels among them: one definition).
//
// search.rs:83-135 scores every unsealed document (a VectorTuple: elements of ascending key) with the SEALED segment's statistics
// before the WAND loop.  The upload turns the documents into an inverted form: per sealed term id the postings (g, c) of the growing
// documents that hold the term, g ascending, c = Cache::evaluate(fieldnorm[g], tf) precomputed (bm25.rs:355-358).  A query's score of
// document g is then the sum of the c of its terms in ascending term-id order -- which is ascending key order, the element order the
// host sums in -- starting from 0.0.  Deleted documents and keys the sealed segment lacks have no postings.
//
// k <= 1024: growing_scan_kernel, one workgroup per (query, run of tiles of GT documents).  A tile's accumulators live in LDS; the
// query's terms are applied in ascending order with a barrier between terms (the first touch of a document stores, later touches
// add: 0.0 + c == c), then every wave offers the touched documents of its quarter of the tile to a RegTopK (ties by g ascending).
// growing_merge_kernel merges a query's lists and then the sealed records with them (sealed first on equal scores).
// k > 1024: a dense accumulator over the growing documents per query, a stable descending radix sort, growing_final_kernel.
//
// Filtered batches (vbm25_filter_set_growing): query q with selector s takes growing bitmap s, one bit per growing document g.  In
// growing_scan_kernel<KM, true> a lane's uint32 word of the bitmap covers exactly the 32 documents of its bits[] word, so a rejected
// document is dropped where the touched documents are extracted (never read from acc, never offered); a tile whose bitmap words are
// all zero is skipped by the whole workgroup before any posting is read.  k > 1024: bigk_mask_kernel zeroes the rejected scores.
#ifndef VBM25_GROWING_H
#define VBM25_GROWING_H

#include "device_types.h"
#include "topk_reg.h"

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

// the records of one query: the sealed list S (ns) and the growing list (gs, gg; ng, best first) merged as vbm25_merge_hits merges
// them -- a growing hit goes before a sealed one only with a higher score.  Every entry is placed by its rank (binary search in the
// other list): the threads of the caller write disjoint records, out may not alias S.
__device__ __forceinline__ void grow_rank_merge(const vbm25_hit *S, uint32_t ns, const double *gs, const uint32_t *gg, uint32_t ng,
                                                uint32_t k, const uint16_t *payload, vbm25_hit *out, uint32_t *n_out, uint32_t tid,
                                                uint32_t nthr) {
    for (uint32_t i = tid; i < ns; i += nthr) {
        const double s = S[i].score;
        uint32_t lo = 0, hi = ng;  // growing hits that score higher
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (gs[mid] > s) lo = mid + 1; else hi = mid;
        }
        const uint32_t pos = i + lo;
        if (pos < k) {
            const unsigned long long *src = reinterpret_cast<const unsigned long long *>(S + i);
            unsigned long long *dst = reinterpret_cast<unsigned long long *>(out + pos);
            dst[0] = src[0];
            dst[1] = src[1];
            dst[2] = src[2];
        }
    }
    for (uint32_t j = tid; j < ng; j += nthr) {
        const double s = gs[j];
        uint32_t lo = 0, hi = ns;  // sealed hits that score at least as high
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (S[mid].score >= s) lo = mid + 1; else hi = mid;
        }
        const uint32_t pos = j + lo;
        if (pos < k) {
            const uint32_t g = gg[j];
            const uint16_t *pl = payload + 3ull * g;
            unsigned long long *dst = reinterpret_cast<unsigned long long *>(out + pos);
            dst[0] = __double_as_longlong(s);
            dst[1] = (unsigned long long)(0xffffffffu - g) | (unsigned long long)pl[0] << 32 | (unsigned long long)pl[1] << 48;
            dst[2] = (unsigned long long)pl[2];
        }
    }
    if (tid == 0) *n_out = min(k, ns + ng);
}

// FILT: the batch has a document filter with growing bitmaps (see the top of this file)
template <int KM, bool FILT>
__global__ void __launch_bounds__(GWG) growing_scan_kernel(DevGrowing G, GrowArgs a) {
    constexpr int RK = KM / 64;
    __shared__ double acc[GT];
    __shared__ uint32_t bits[GT / 32];
    __shared__ uint32_t s_t[MAX_TERMS], s_lo[MAX_TERMS], s_cum[MAX_TERMS + 1];
    __shared__ uint32_t s_nt;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = blockIdx.x / a.gq, w = blockIdx.x % a.gq;
    const uint32_t k = a.k;
    const uint32_t j0 = uint32_t(uint64_t(w) * G.n_tiles / a.gq), j1 = uint32_t(uint64_t(w + 1) * G.n_tiles / a.gq);
    // a growing document must beat the sealed k-th score: on equal scores the sealed hit wins
    const uint32_t ns = a.sealed_cnt[q];
    const double thr = ns >= k ? a.sealed[size_t(q) * k + k - 1].score : 0.0;
    if (tid == 0) s_nt = 0;
    for (uint32_t i = tid; i < GT / 32; i += GWG) bits[i] = 0;
    __syncthreads();
    {   // the query's indexed terms: ids are strictly ascending, so those below n_terms are a prefix
        const uint32_t q0 = a.q_off[q], q1 = a.q_off[q + 1];
        for (uint32_t r = tid; r < q1 - q0 && r < (uint32_t)MAX_TERMS; r += GWG) {
            const uint32_t t = a.term_ids[q0 + r];
            if (t < G.n_terms) {
                s_t[r] = t;
                atomicAdd(&s_nt, 1u);
            }
        }
    }
    __syncthreads();
    const uint32_t nt = s_nt;
    const uint32_t *fw = nullptr;  // the query's growing bitmap (FILT), NULL: none
    if constexpr (FILT) {
        const uint32_t s = a.filt_sel[q];
        if (s != NONE32) fw = a.filt_words + size_t(s) * a.filt_stride;
    }
    RegTopK<RK> top;
    top.init();
    for (uint32_t j = j0; j < j1 && nt; ++j) {
        const uint32_t tile_lo = j * GT;
        uint32_t keep = ~0u;  // the bitmap word of this thread's bits[] word (the documents tile_lo + 32 tid ..)
        if constexpr (FILT) {
            if (fw) {
                const uint32_t fi = j * (GT / 32u) + tid;
                keep = fi < a.filt_stride ? fw[fi] : 0u;
            }
            // no document of the tile may be returned: the whole workgroup skips it (a barrier: uniform)
            if (!__syncthreads_or(keep != 0u)) continue;
        }
        __syncthreads();  // (the last tile's reads of s_cum and acc are done)
        for (uint32_t r = tid; r < nt; r += GWG) {
            const uint2 rg = grow_tile_range(G, s_t[r], j);
            s_lo[r] = rg.x;
            s_cum[r + 1] = rg.y - rg.x;  // (counts: the prefix sum follows)
        }
        __syncthreads();
        if (wave == 0) {
            uint32_t carry = 0;
            for (uint32_t base = 0; base < nt; base += 64) {
                const uint32_t r = base + lane;
                uint32_t v = r < nt ? s_cum[r + 1] : 0u;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t u = __shfl_up(v, o);
                    if (lane >= (uint32_t)o) v += u;
                }
                if (r < nt) s_cum[r + 1] = carry + v;
                carry += __shfl(v, 63);
            }
            if (lane == 0) s_cum[0] = 0;
        }
        __syncthreads();
        const uint32_t P = s_cum[nt];
        if (P == 0) continue;
        auto term_of = [&](uint32_t i) {  // last r with s_cum[r] <= i
            uint32_t lo = 0, hi = nt;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_cum[mid] <= i) lo = mid; else hi = mid;
            }
            return lo;
        };
        // postings in chunks of GWG (loads of all the chunk's terms in flight at once), applied term by term
        for (uint32_t base = 0; base < P; base += GWG) {
            const uint32_t i = base + tid;
            const bool mine = i < P;
            uint32_t r = 0, l = 0;
            double c = 0.0;
            if (mine) {
                r = term_of(i);
                const uint32_t p = s_lo[r] + (i - s_cum[r]);
                l = G.post_g[p] - tile_lo;
                c = G.post_c[p];
            }
            const uint32_t r_first = term_of(base), r_last = term_of(min(base + GWG, P) - 1u);
            for (uint32_t rr = r_first; rr <= r_last; ++rr) {
                if (mine && r == rr) {
                    const uint32_t bit = 1u << (l & 31u);
                    const uint32_t old = atomicOr(&bits[l >> 5], bit);
                    if (old & bit) acc[l] += c;
                    else acc[l] = c;
                }
                __syncthreads();
            }
        }
        // the touched documents of this wave's quarter of the tile (one bitmap word per lane), cleared for the next tile
        {
            const uint32_t wi = wave * 64u + lane;
            uint32_t word = bits[wi];
            bits[wi] = 0;
            if constexpr (FILT) word &= keep;  // (wi == tid)
            while (__ballot(word != 0)) {
                bool has = word != 0;
                uint32_t d = 0;
                double s = 0.0;
                if (has) {
                    const uint32_t b = (uint32_t)__builtin_ctz(word);
                    word &= word - 1u;
                    const uint32_t ll = wi * 32u + b;
                    s = acc[ll];
                    d = tile_lo + ll;
                    has = s > thr;
                }
                top.offer(has, s, d, k, lane);
            }
        }
    }
    const uint32_t L = (q * a.gq + w) * 4u + wave;
#pragma unroll
    for (int rr = 0; rr < RK; ++rr) {
        const uint32_t e = rr * 64u + lane;
        if (e < top.cnt) {
            a.ls[size_t(L) * k + e] = top.score[rr];
            a.lg[size_t(L) * k + e] = top.doc[rr];
        }
    }
    if (lane == 0) a.lc[L] = top.cnt;
}

// one wave per query: the query's 4 gq lists -> its growing top-k, then merged with the sealed records into the batch's records
template <int KM>
__global__ void __launch_bounds__(64) growing_merge_kernel(DevGrowing G, GrowArgs a) {
    constexpr int RK = KM / 64;
    __shared__ double fs[KM];
    __shared__ uint32_t fg[KM];
    const uint32_t q = blockIdx.x, lane = threadIdx.x, k = a.k;
    RegTopK<RK> top;
    top.init();
    for (uint32_t L = q * a.gq * 4u; L < (q + 1) * a.gq * 4u; ++L) {
        const uint32_t cnt = a.lc[L];
        for (uint32_t base = 0; base < cnt; base += 64) {
            const uint32_t e = base + lane;
            const bool has = e < cnt;
            const double s = has ? a.ls[size_t(L) * k + e] : 0.0;
            const uint32_t d = has ? a.lg[size_t(L) * k + e] : 0u;
            top.offer(has, s, d, k, lane);
        }
    }
#pragma unroll
    for (int rr = 0; rr < RK; ++rr) {
        const uint32_t e = rr * 64u + lane;
        if (e < top.cnt) {
            fs[e] = top.score[rr];
            fg[e] = top.doc[rr];
        }
    }
    __syncthreads();
    grow_rank_merge(a.sealed + size_t(q) * k, a.sealed_cnt[q], fs, fg, top.cnt, k, G.payload, a.hits + size_t(q) * k, a.n_hits + q,
                    lane, 64);
}

// k > 1024: acc[g] += c for the postings [p0, p0 + n) of one term (a document has one posting per term: the adds never collide)
__global__ void __launch_bounds__(256) grow_accum_kernel(const uint32_t *post_g, const double *post_c, uint32_t p0, uint32_t n,
                                                         double *acc) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t g = post_g[p0 + i];
        acc[g] = acc[g] + post_c[p0 + i];
    }
}

// k > 1024: the sorted (score bits, g) of one query (zero keys: no hit) merged with its sealed records
__global__ void __launch_bounds__(256) growing_final_kernel(const vbm25_hit *sealed, const uint32_t *sealed_cnt,
                                                            const unsigned long long *keys, const uint32_t *docs, uint32_t n_avail,
                                                            uint32_t k, const uint16_t *payload, vbm25_hit *hits, uint32_t *n_hits) {
    uint32_t lo = 0, hi = min(n_avail, k);  // the non-zero keys are a prefix
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] != 0) lo = mid + 1; else hi = mid;
    }
    grow_rank_merge(sealed, *sealed_cnt, reinterpret_cast<const double *>(keys), docs, lo, k, payload, hits, n_hits,
                    blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

}  // namespace vbm25

#endif
