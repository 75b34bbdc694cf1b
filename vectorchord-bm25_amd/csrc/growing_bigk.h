// growing_bigk.h -- the growing (unsealed) segment at k > 1024, batched: the two kernels of its own.  bigk.hip alone includes and
// launches them, between them bigk_select_kernel and bigk_sort_kernel of that unit on the growing candidate segments (a second
// descriptor array and cursor block: the same kernels, nothing copied).  The records are byte for byte those of the per-query branch
// of growing_enqueue (search.hip: an accumulator per growing document, a launch per term, a stable radix sort, growing_final_kernel),
// which stays behind the switch bigk_grow = 0 as the comparison.  Per chunk of queries, whatever they hold:
//   growing_bigk_scan_kernel   work item = (query, run of tiles of GT growing documents), one workgroup, computed from the workgroup's
//                          number (gbk::item_tiles: no item list).  growing_scan_kernel's loop (growing.h): a tile's f64
//                          accumulators and its touched bitmap in LDS, the postings of the tile loaded a workgroup-wide chunk at a
//                          time across terms and applied term by term with a barrier between terms -- the first touch stores, later
//                          touches add, so a document's sum is formed in query order from its first term's c exactly as
//                          grow_accum_kernel's per-term launches form it from 0.0 (0.0 + c == c).  The query's terms come up with
//                          its descriptor at every run: those with a growing posting, in query order (a k > 1024 batch keeps its
//                          queries on the host only; a term without a growing posting adds nothing).  The LDS term table holds
//                          gbk::TERM_PASS terms and is refilled in passes, in order, for a query of more.  A tile whose filter
//                          words are all zero, or in which no term has a posting, is skipped by the whole workgroup before any
//                          posting is read.  The sweep makes no top-k offers: a thread a bitmap word, every touched document's
//                          filter bit applied, a zero sum dropped, and -- when the query's sealed list is full -- a sum not above
//                          the sealed k-th score dropped too (exact: grow_rank_merge places such an entry at position >= k, on equal
//                          scores the sealed hit wins).  What is left is appended as (score bits, g) to the query's candidate
//                          segment: one atomic add a wave and round on the query's cursor, ballot ranks.  The sweep clears the
//                          bitmap words it reads: no tile-sized wipe between tiles.
//   bigk_select_kernel, bigk_sort_kernel (bigk.hip)   at most k survivors of "key descending, g ascending" -- the stable descending
//                          sort over an iota of the per-query branch -- in tiles of 4096 sorted best first
//   growing_bigk_merge_kernel  grid (k in 256s, queries of the chunk): thread i places growing survivor i and sealed record i by
//                          rank (growing_bigk_lane.h) and writes the records below k in grow_rank_merge's layout.  The sealed
//                          records are read from the copy growing_enqueue makes: the output never aliases its input.
#ifndef VBM25_GROWING_BIGK_H
#define VBM25_GROWING_BIGK_H

#include <hip/hip_runtime.h>

#include "host_objects.h"
#include "growing_tile.h"
#include "bigk_lane.h"
#include "growing_bigk_lane.h"

namespace vbm25 {

struct GrowBigkArgs {
    const BigkQuery *qd;              // per query of the batch (descriptor q = query q): its terms and its candidate segment
    const uint32_t *terms;            // the queries' indexed terms that have a growing posting, in query order
    uint32_t *cursor;                 // per query: candidates appended
    uint32_t *stats;                  // [0] candidates appended, [1] candidates pruned by the sealed threshold
    uint64_t *cand_key;
    uint32_t *cand_doc;
    const uint32_t *filt_words;       // NULL: no filter; growing bitmap s = filt_stride uint32 words (GrowArgs' layout)
    const uint32_t *filt_sel;
    uint32_t filt_stride;
    const vbm25_hit *sealed;          // the sealed records of the run (a copy: nq x k) and their counts
    const uint32_t *sealed_cnt;
    const uint32_t *surv_cnt;         // per query: survivors of the select
    const uint64_t *surv_key;         // per query of the chunk: surv_stride entries, tiles sorted best first
    const uint32_t *surv_doc;
    uint32_t k, surv_stride;
    vbm25_hit *hits;                  // the batch's records: the merged result
    uint32_t *n_hits;
    uint32_t *error_flag;
};

static_assert(sizeof(vbm25_hit) == 24, "a record is three 8-byte words, the score first");
static_assert(GT / 32u == GWG, "the sweep: a thread a bitmap word");

__global__ void __launch_bounds__(GWG) growing_bigk_scan_kernel(DevGrowing G, GrowBigkArgs a, uint32_t q0, uint32_t ipq) {
    using ull = unsigned long long;
    __shared__ double acc[GT];
    __shared__ uint32_t bits[GT / 32];
    __shared__ uint32_t s_lo[gbk::TERM_PASS], s_cum[gbk::TERM_PASS + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = q0 + blockIdx.x / ipq, w = blockIdx.x % ipq;
    const BigkQuery qd = a.qd[q];
    if (qd.cand_cap == 0u) return;  // (the whole workgroup: no term of the query has a growing posting)
    uint32_t j0, j1;
    gbk::item_tiles(w, ipq, G.n_tiles, j0, j1);
    const uint32_t k = a.k;
    // a growing document must beat the sealed k-th score: on equal scores the sealed hit wins
    const bool full = a.sealed_cnt[q] >= k;
    const double thr = full ? a.sealed[size_t(q) * k + k - 1u].score : 0.0;
    const uint32_t t0 = qd.term_lo, nt_all = qd.term_hi - qd.term_lo;
    bits[tid] = 0;
    const uint32_t *fw = nullptr;  // the query's growing bitmap, NULL: none
    if (a.filt_words) {
        const uint32_t s = a.filt_sel[q];
        if (s != NONE32) fw = a.filt_words + size_t(s) * a.filt_stride;
    }
    uint64_t *ckey = a.cand_key + qd.cand_base;
    uint32_t *cdoc = a.cand_doc + qd.cand_base;
    uint32_t n_app = 0, n_prune = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t tile_lo = j * GT;
        uint32_t keep = ~0u;  // the filter's word of this thread's bits[] word (the documents tile_lo + 32 tid ..)
        if (a.filt_words) {
            if (fw) {
                const uint32_t fi = j * (GT / 32u) + tid;
                keep = fi < a.filt_stride ? fw[fi] : 0u;
            }
            // no document of the tile may be returned: the whole workgroup skips it (a barrier: uniform)
            if (!__syncthreads_or(keep != 0u)) continue;
        }
        bool any = false;  // some term has a posting in the tile (uniform)
        for (uint32_t tb = 0; tb < nt_all; tb += gbk::TERM_PASS) {  // the term table, pass after pass in query order
            const uint32_t nt = min(gbk::TERM_PASS, nt_all - tb);
            __syncthreads();  // (the reads of s_lo and s_cum of the pass before, bits[] zero at the first tile)
            for (uint32_t r = tid; r < nt; r += GWG) {
                const uint32_t t = a.terms[t0 + tb + r];
                const uint2 rg = t < G.n_terms ? grow_tile_range(G, t, j) : make_uint2(0u, 0u);
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
            any = true;
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
                    if (mine && r == rr && l < GT) {  // (l < GT: by grow_tile_range)
                        const uint32_t bit = 1u << (l & 31u);
                        const uint32_t old = atomicOr(&bits[l >> 5], bit);
                        if (old & bit) acc[l] += c;
                        else acc[l] = c;
                    }
                    __syncthreads();
                }
            }
        }
        if (!any) continue;
        // sweep: the touched documents of this thread's bitmap word, cleared for the next tile
        uint32_t word = bits[tid];
        bits[tid] = 0;
        word &= keep;
        while (__ballot(word != 0u)) {
            ull key = 0;
            uint32_t g = 0;
            if (word) {
                const uint32_t b = (uint32_t)__builtin_ctz(word);
                word &= word - 1u;
                const uint32_t ll = tid * 32u + b;
                const double s = acc[ll];
                key = (ull)__double_as_longlong(s);
                g = tile_lo + ll;
                if (key != 0ull && full && !(s > thr)) {
                    key = 0;
                    ++n_prune;
                }
            }
            const ull m = __ballot(key != 0ull);
            if (m) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(a.cursor + q, (uint32_t)__popcll(m));
                base = __shfl(base, 0);
                const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (key != 0ull) {
                    if (slot < qd.cand_cap) {
                        ckey[slot] = key;
                        cdoc[slot] = g;
                        ++n_app;
                    } else {
                        atomicOr(a.error_flag, 8u);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        n_app += __shfl_xor(n_app, o);
        n_prune += __shfl_xor(n_prune, o);
    }
    if (lane == 0 && n_app) atomicAdd(&a.stats[0], n_app);
    if (lane == 0 && n_prune) atomicAdd(&a.stats[1], n_prune);
}

// grid (k in 256s, queries of the chunk)
__global__ void __launch_bounds__(256) growing_bigk_merge_kernel(DevGrowing G, GrowBigkArgs a, uint32_t q0) {
    using ull = unsigned long long;
    const uint32_t q = q0 + blockIdx.y, k = a.k;
    const uint32_t ns = min(a.sealed_cnt[q], k), ng = min(a.surv_cnt[q], k);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint64_t *keys = a.surv_key + size_t(blockIdx.y) * a.surv_stride;
    const uint32_t *docs = a.surv_doc + size_t(blockIdx.y) * a.surv_stride;
    const vbm25_hit *S = a.sealed + size_t(q) * k;
    const double *Ss = reinterpret_cast<const double *>(S);
    vbm25_hit *out = a.hits + size_t(q) * k;
    if (i == 0) a.n_hits[q] = min(k, ns + ng);
    if (i < ns) {
        const uint32_t pos = gbk::sealed_pos(keys, ng, Ss, 3u, i);
        if (pos < k) {
            const ull *src = reinterpret_cast<const ull *>(S + i);
            ull *dst = reinterpret_cast<ull *>(out + pos);
            dst[0] = src[0];
            dst[1] = src[1];
            dst[2] = src[2];
        }
    }
    if (i < ng) {
        const uint32_t pos = gbk::growing_pos(keys, docs, ng, i, Ss, 3u, ns);
        if (pos < k) {
            const uint32_t g = docs[i];
            const uint16_t *pl = G.payload + 3ull * g;
            ull *dst = reinterpret_cast<ull *>(out + pos);
            dst[0] = keys[i];
            dst[1] = (ull)(0xffffffffu - g) | (ull)pl[0] << 32 | (ull)pl[1] << 48;
            dst[2] = (ull)pl[2];
        }
    }
}

}  // namespace vbm25

#endif
