// bigk_dense.h -- the kernels of the dense half of the k > 1024 route; bigk.hip alone includes and launches them.  A dense query (its
// document frequencies sum to more than bigk_cand_max) cannot list every touched document, so its scan finds a threshold first: an
// MSD radix select over the composite (key, ~doc) whose histograms are made by scanning the postings (bigk_dense_lane.h has the
// interval arithmetic and the walk).  Per chunk of dense queries the host enqueues, unconditionally and without waiting,
//   bigk_dense_init_kernel         a thread a query: the level-0 state from the upper bound K_ub of its scores
//   MAX_LEVELS times
//     bigk_dense_scan_kernel<false>  the histogram scan: work item = (query, run of 8192-document windows), one workgroup of 8 waves.
//                                  The accumulation is bigk_scan_kernel's -- direct-addressed f64 in LDS, the terms in query order
//                                  with a workgroup barrier behind every term, a block that straddles a cut decoded on both sides --
//                                  so the keys are bit for bit the per-query path's.  The sweep reads and clears a touched document's
//                                  sum, applies the filter's bit, drops zeros and counts the entry's bin inside the query's interval
//                                  in an LDS histogram of 4096 bins; the item flushes it with one global atomic per non-zero bin.  An
//                                  item of a settled query returns after loading its item and the query's state.
//     bigk_dense_walk_kernel       a workgroup a query: the histogram walked from the top, cleared for the next level, the state
//                                  stepped (bgd::decide).  A settled query's workgroup returns at once.
//   bigk_dense_scan_kernel<true>   the emit scan: the same accumulation; the sweep appends (key, doc) of every entry >= the query's lo
//                                  to its candidate segment as bigk_scan_kernel does (one atomic on the cursor per wave and round,
//                                  ballot ranks, error flag 8 past the capacity).  By construction at most the capacity arrive, and
//                                  at least k when the query has k non-zero documents.
// and then bigk_select_kernel / bigk_sort_kernel / bigk_rank_emit_kernel on the segments, unchanged.
#ifndef VBM25_BIGK_DENSE_H
#define VBM25_BIGK_DENSE_H

#include <hip/hip_runtime.h>

#include "host_objects.h"
#include "decode.h"
#include "block_fetch.h"
#include "bigk_lane.h"
#include "bigk_dense_lane.h"

namespace vbm25 {

struct BigkDenseArgs {
    const BigkQuery *qd;
    const BigkItem *items;
    const uint32_t *terms;
    uint32_t *cursor;
    uint64_t *cand_key;
    uint32_t *cand_doc;
    const unsigned long long *filt_words;  // NULL: no filter
    const uint32_t *filt_sel;
    uint32_t filt_stride;
    uint32_t k;
    uint32_t d0;             // the descriptor index of the first dense query: query s has state[s - d0]
    bgd::State *state;
    uint32_t *hist;          // BINS words per query of the chunk, zero between levels
    uint32_t *stats;         // [0] the highest level any query needed, plus one; [1] queries whose level-0 boundary was the clip bin
    uint32_t *error_flag;
};

namespace bgd {
constexpr uint32_t SCAN_WAVES = bgk::SCAN_THREADS / 64;
constexpr uint32_t SWEEP_WORDS = bgk::WINDOW_WORDS / SCAN_WAVES;  // bitmap words a wave sweeps: one a lane of its first lanes
static_assert(SWEEP_WORDS >= 1 && SWEEP_WORDS <= 64, "a wave reads its bitmap words one a lane");
static_assert(WALK_GROUP == 16, "the walk loads a thread's bins as four uint4");
}  // namespace bgd

// a thread a dense query: K_ub = the bits of the sum of its terms' s0, in f64 and in query order.  Every posting's score is below its
// term's s0 and rounding is monotone, so no document's key exceeds it.  (An s0 that is not positive: the bound above every score.)
__global__ void __launch_bounds__(256) bigk_dense_init_kernel(DevIndex ix, BigkDenseArgs a, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BigkQuery qd = a.qd[a.d0 + i];
    double sum = 0.0;
    bool ok = true;
    for (uint32_t p = qd.term_lo; p < qd.term_hi; ++p) {
        const double s0 = ix.term_s0[a.terms[p]];
        ok = ok && s0 > 0.0;
        sum = sum + s0;
    }
    const uint64_t bits = (uint64_t)__double_as_longlong(sum);
    a.state[i] = bgd::level0(ok && bits < bgd::KUB_ALL ? bits : bgd::KUB_ALL);
}

template <bool EMIT>
__global__ void __launch_bounds__(bgk::SCAN_THREADS) bigk_dense_scan_kernel(DevIndex ix, BigkDenseArgs a, uint32_t item0, uint32_t chunk_s0) {
    using ull = unsigned long long;
    __shared__ double s_acc[bgk::WINDOW];
    __shared__ ull s_bits[bgk::WINDOW_WORDS];
    __shared__ uint32_t s_jlo[bgk::TERM_TABLE], s_jhi[bgk::TERM_TABLE];
    __shared__ double s_s0[bgk::TERM_TABLE];
    __shared__ uint32_t s_hist[EMIT ? 1u : bgd::BINS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const BigkItem it = a.items[item0 + blockIdx.x];
    const bgd::State st = a.state[it.s - a.d0];
    if (EMIT != (st.settled != 0u)) {  // (the whole workgroup) a settled query has no more levels; the emit finds every query settled
        if (EMIT && tid == 0) atomicOr(a.error_flag, 8u);
        return;
    }
    const BigkQuery qd = a.qd[it.s];
    const uint32_t nt = qd.term_hi - qd.term_lo;
    if (nt > bgk::TERM_TABLE) {  // (set_queries refuses such a query)
        if (tid == 0) atomicOr(a.error_flag, 8u);
        return;
    }
    const bgd::u128 lo = bgd::lo_of(st), top = bgd::top_of(st);
    const uint32_t doc_lo = it.win_lo * bgk::WINDOW;
    const uint32_t doc_hi = (uint32_t)min((ull)it.win_hi * bgk::WINDOW, (ull)ix.n_docs);
    for (uint32_t i = tid; i < bgk::WINDOW; i += bgk::SCAN_THREADS) s_acc[i] = 0.0;
    for (uint32_t i = tid; i < bgk::WINDOW_WORDS; i += bgk::SCAN_THREADS) s_bits[i] = 0ull;
    if (!EMIT)
        for (uint32_t i = tid; i < bgd::BINS; i += bgk::SCAN_THREADS) s_hist[i] = 0u;
    // the term table: per term the blocks that can hold a document of the item, and s0
    for (uint32_t p = tid; p < nt; p += bgk::SCAN_THREADS) {
        const uint32_t t = a.terms[qd.term_lo + p];
        const uint32_t j0 = ix.term_first_block[t], j1 = ix.term_first_block[t + 1];
        uint32_t l = j0, h = j1;
        while (l < h) {  // first block whose last id is >= doc_lo
            const uint32_t mid = (l + h) >> 1;
            if (ix.blk_max_doc[mid] >= doc_lo) h = mid;
            else l = mid + 1u;
        }
        const uint32_t jlo = l;
        h = j1;
        while (l < h) {  // first block whose first id is >= doc_hi
            const uint32_t mid = (l + h) >> 1;
            if (ix.blk_min_doc[mid] >= doc_hi) h = mid;
            else l = mid + 1u;
        }
        s_jlo[p] = jlo;
        s_jhi[p] = l;
        s_s0[p] = ix.term_s0[t];
    }
    __syncthreads();
    const ull *filt = nullptr;
    if (a.filt_words) {
        const uint32_t sel = a.filt_sel[qd.q];
        if (sel != UINT32_MAX) filt = a.filt_words + size_t(sel) * a.filt_stride;
    }
    uint64_t *ckey = a.cand_key + qd.cand_base;
    uint32_t *cdoc = a.cand_doc + qd.cand_base;
    for (uint32_t w = it.win_lo; w < it.win_hi; ++w) {
        const uint32_t w0 = w * bgk::WINDOW;
        if (w0 >= doc_hi) break;
        const uint32_t w1 = min(w0 + bgk::WINDOW, doc_hi);
        for (uint32_t p = 0; p < nt; ++p) {
            const uint32_t jlo = s_jlo[p], jhi = s_jhi[p];
            if (jlo >= jhi) continue;  // (the whole workgroup: the term has no posting in the item)
            const double s0 = s_s0[p];
            const uint32_t js = wave_lower_bound(ix.blk_max_doc, jlo, jhi, w0, lane);
            for (uint32_t j = js + wave; j < jhi && ix.blk_min_doc[j] < w1; j += bgd::SCAN_WAVES) {
                const uint4 bm = ix.blk_meta[j];
                const uint32_t n = bm.w & 0xff, md = (bm.w >> 8) & 0xff, mt = (bm.w >> 16) & 0xff;
                const uint8_t *body = ix.blob + 8ull * bm.z;
                uint32_t d0, d1, f0, f1;
                decode_doc_ids(body, md, n, bm.x, lane, d0, d1);
                decode_fields(body + ((payload_bytes(md, n) + 7u) & ~7u), mt, n, lane, f0, f1);
                const uchar2 fn = reinterpret_cast<const uchar2 *>(ix.post_fn + 128ull * j)[lane];
                if (2 * lane < n && d0 >= w0 && d0 < w1) {
                    const double tf = (double)f0;
                    const uint32_t r = d0 - w0;
                    s_acc[r] = s_acc[r] + (tf * s0) / (tf + ix.s1[fn.x]);  // Cache::evaluate, bm25.rs:355-358
                    atomicOr(&s_bits[r >> 6], 1ull << (r & 63u));
                }
                if (2 * lane + 1 < n && d1 >= w0 && d1 < w1) {
                    const double tf = (double)f1;
                    const uint32_t r = d1 - w0;
                    s_acc[r] = s_acc[r] + (tf * s0) / (tf + ix.s1[fn.y]);
                    atomicOr(&s_bits[r >> 6], 1ull << (r & 63u));
                }
            }
            __syncthreads();  // the next term's adds see this term's sums
        }
        // sweep: every wave its own words of the bitmap
        const uint32_t wbase = wave * bgd::SWEEP_WORDS;
        const ull mine = lane < bgd::SWEEP_WORDS ? s_bits[wbase + lane] : 0ull;
        ull nz = __ballot(mine != 0ull);
        while (nz) {
            const uint32_t l = (uint32_t)__ffsll((long long)nz) - 1u;
            nz &= nz - 1ull;
            const uint32_t wi = wbase + l;
            const ull word = s_bits[wi];
            const uint32_t doc = w0 + wi * 64u + lane;
            ull key = 0;
            if ((word >> lane) & 1ull) {
                key = (ull)__double_as_longlong(s_acc[wi * 64u + lane]);
                s_acc[wi * 64u + lane] = 0.0;
            }
            if (filt && !((filt[(w0 >> 6) + wi] >> lane) & 1ull)) key = 0;  // (bigk_mask_kernel's word and bit)
            if (!EMIT) {
                if (key != 0ull) {
                    bgd::u128 c = bgd::composite(key, doc);
                    if (st.level == 0u && c > top) {  // (cannot be: no score exceeds the sum of the s0)
                        atomicOr(a.error_flag, 8u);
                        c = top;
                    }
                    if (bgd::inside(c, lo, top)) atomicAdd(&s_hist[bgd::bin_of(c, top, st.shift)], 1u);
                }
            } else {
                if (key != 0ull && bgd::composite(key, doc) < lo) key = 0;
                const ull m = __ballot(key != 0ull);
                if (m) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(a.cursor + it.s, (uint32_t)__popcll(m));
                    base = __shfl(base, 0);
                    const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (key != 0ull) {
                        if (slot < qd.cand_cap) {
                            ckey[slot] = key;
                            cdoc[slot] = doc;
                        } else {
                            atomicOr(a.error_flag, 8u);
                        }
                    }
                }
            }
            if (lane == 0) s_bits[wi] = 0ull;
        }
        __syncthreads();  // the next window's adds find zeros
    }
    if (!EMIT) {  // (behind the last window's barrier) one global atomic per non-zero bin
        uint32_t *gh = a.hist + size_t(it.s - chunk_s0) * bgd::BINS;
        for (uint32_t i = tid; i < bgd::BINS; i += bgk::SCAN_THREADS) {
            const uint32_t c = s_hist[i];
            if (c) atomicAdd(&gh[i], c);
        }
    }
}

// grid: the chunk's queries.  Thread t sums bins [16 t, 16 t + 16) and clears them; thread 0 walks the group sums, then one group.
__global__ void __launch_bounds__(bgd::WALK_THREADS) bigk_dense_walk_kernel(BigkDenseArgs a, uint32_t chunk_s0) {
    __shared__ uint32_t s_h[bgd::BINS], s_g[bgd::WALK_THREADS];
    const uint32_t tid = threadIdx.x, s = chunk_s0 + blockIdx.x;
    bgd::State st = a.state[s - a.d0];
    if (st.settled) return;  // (the whole workgroup; nothing was counted: the histogram is zero)
    uint4 *gh = reinterpret_cast<uint4 *>(a.hist + size_t(blockIdx.x) * bgd::BINS) + 4u * tid;
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint4 v = gh[i];
        gh[i] = make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4 *>(&s_h[bgd::WALK_GROUP * tid + 4u * i]) = v;
        sum += v.x + v.y + v.z + v.w;
    }
    s_g[tid] = sum;
    __syncthreads();
    if (tid != 0) return;
    uint64_t total = 0, before = 0;
    for (uint32_t g = 0; g < bgd::WALK_THREADS; ++g) total += s_g[g];
    const uint32_t d = bgd::walk_grouped(s_h, s_g, uint64_t(a.k - st.above), before);
    atomicMax(&a.stats[0], st.level + 1u);
    if (bgd::decide(st, a.k, a.qd[s].cand_cap, total, d, before, d < bgd::BINS ? s_h[d] : 0u)) atomicAdd(&a.stats[1], 1u);
    a.state[s - a.d0] = st;
}

}  // namespace vbm25

#endif
