// plan.h -- plan_kernel (queries -> doc-range work items).
// Included by search.hip only (a non-template kernel: one definition).
#ifndef VBM25_PLAN_H
#define VBM25_PLAN_H

#include "device_types.h"
#include "decode.h"

namespace vbm25 {

// ---------------------------------------------------------------------------
// Planner
// ---------------------------------------------------------------------------
// Block-wide inclusive scan of one u64 per thread (PLAN_WG threads): wave scans + one LDS hop.
__device__ __forceinline__ unsigned long long plan_incl_scan(unsigned long long v, unsigned long long *s_wave,
                                                             unsigned long long &total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(v, o);
        if ((int)lane >= o) v += y;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (uint32_t w = 0; w < PLAN_WG / 64; ++w) {
        const unsigned long long x = s_wave[w];
        if (w < wave) before += x;
        all += x;
    }
    __syncthreads();
    total = all;
    return v + before;
}

// dense_c != 0: every dense query (q_dense) is cut into dense_c items of equal document counts -- the dense-window kernel's
// work per item goes with its windows, not with its postings -- and does not count towards the other queries' chunk size.
__global__ void __launch_bounds__(PLAN_WG) plan_kernel(DevIndex ix, DevBatch bt, uint32_t max_items,
                                                       uint32_t target_items, uint32_t min_chunk, uint32_t dense_c) {
    __shared__ unsigned long long s_wave[PLAN_WG / 64];
    __shared__ uint32_t s_bucket[PLAN_BUCKETS];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < (uint32_t)PLAN_BUCKETS; i += PLAN_WG) s_bucket[i] = 0;
    const uint32_t per = (bt.nq + PLAN_WG - 1) / PLAN_WG;
    const uint32_t q0 = min(bt.nq, tid * per), q1 = min(bt.nq, q0 + per);
    // per-launch state of the scan kernels (saves two memset launches per step)
    for (uint32_t i = tid; i < bt.nq; i += PLAN_WG) bt.theta[i] = 0;
    for (uint32_t i = tid; i < max_items; i += PLAN_WG) {
        bt.item_failed[i] = 0;
        bt.item_order[i] = i;  // (every slot defined even when the item count overflows: error_flag 2)
    }
    __syncthreads();
    if (bt.lpi > 1)  // lists a kernel does not write must read as empty
        for (uint32_t i = tid; i < max_items * bt.lpi; i += PLAN_WG) bt.res_cnt[i] = 0;
    if (tid == 0) {
        bt.work_ctr[0] = 0;
        bt.work_ctr[1] = 0;
        *bt.fail_any = 0;
    }

    auto postings_of = [&](uint32_t q) {
        unsigned long long t = 0;
        for (uint32_t p = bt.q_off[q]; p < bt.q_off[q + 1]; ++p) {
            uint32_t term = bt.term_ids[p];
            if (term < ix.n_terms) t += ix.term_df[term];
        }
        return t;
    };
    // a thread usually owns one query (nq <= PLAN_WG): its posting count is read once and kept -- every
    // evaluation is a chain of three dependent global loads, which is what a small batch's plan costs
    const bool one = q1 - q0 == 1;
    const unsigned long long own_postings = one ? postings_of(q0) : 0ull;
    auto is_dense = [&](uint32_t q) { return dense_c != 0 && bt.q_dense[q] != 0; };
    unsigned long long local = one && !is_dense(q0) ? own_postings : 0ull;
    if (!one)
        for (uint32_t q = q0; q < q1; ++q)
            if (!is_dense(q)) local += postings_of(q);
    unsigned long long total = 0;
    plan_incl_scan(local, s_wave, total);
    unsigned long long chunk = (total + target_items - 1) / target_items;
    if (chunk < min_chunk) chunk = min_chunk;
    auto chunks_of = [&](uint32_t q) -> uint32_t {
        unsigned long long t = one ? own_postings : postings_of(q);
        if (t == 0) return 0u;
        if (is_dense(q)) return min(dense_c, ix.n_docs);
        // nearest, not ceil: a batch of similar queries gets the same count for all of them, i.e. the
        // item count lands on the target (a multiple of the resident waves) instead of ~8 % above it
        unsigned long long c = (t + chunk / 2) / chunk;
        if (c == 0) c = 1;
        if (c > ix.n_docs) c = ix.n_docs;
        return (uint32_t)c;
    };
    unsigned long long cnt = 0;
    for (uint32_t q = q0; q < q1; ++q) cnt += chunks_of(q);
    unsigned long long run = 0;
    const unsigned long long incl = plan_incl_scan(cnt, s_wave, run);
    if (tid == 0) {
        *bt.n_items = (uint32_t)min(run, (unsigned long long)max_items);
        if (run > max_items) atomicOr(bt.error_flag, 2u);
        bt.q_item_base[bt.nq] = (uint32_t)min(run, (unsigned long long)max_items);
    }
    uint32_t base = (uint32_t)(incl - cnt);
    // The persistent scan kernels draw items through item_order: longest first (the last items drawn decide when the
    // launch ends).  A counting sort over buckets of the items' postings: exponent and three mantissa bits.
    auto bucket_of = [&](unsigned long long postings, uint32_t c) -> uint32_t {
        const unsigned long long w = postings / (c ? c : 1u) + 1ull;
        const uint32_t e = 63u - (uint32_t)__builtin_clzll(w);
        const uint32_t sub = e >= 3u ? (uint32_t)(w >> (e - 3u)) & 7u : 0u;
        return min(8u * e + sub, (uint32_t)PLAN_BUCKETS - 1u);
    };
    for (uint32_t q = q0; q < q1; ++q) {
        const uint32_t c = chunks_of(q);
        if (c) atomicAdd(&s_bucket[bucket_of(one ? own_postings : postings_of(q), c)], c);
    }
    __syncthreads();
    {   // first position of every bucket, from the largest bucket down (PLAN_BUCKETS <= PLAN_WG: one bucket per thread)
        const uint32_t bkt = (uint32_t)PLAN_BUCKETS - 1u - tid;
        const unsigned long long v = tid < (uint32_t)PLAN_BUCKETS ? s_bucket[bkt] : 0u;
        unsigned long long all = 0;
        const unsigned long long in = plan_incl_scan(v, s_wave, all);
        if (tid < (uint32_t)PLAN_BUCKETS) s_bucket[bkt] = (uint32_t)(in - v);
    }
    __syncthreads();
    for (uint32_t q = q0; q < q1; ++q) {
        const uint32_t c = chunks_of(q);
        uint32_t nterms = 0;
        for (uint32_t p = bt.q_off[q]; p < bt.q_off[q + 1]; ++p) nterms += bt.term_ids[p] < ix.n_terms;
        if (bt.q_dense[q]) nterms |= ITEM_DENSE;
        bt.q_item_base[q] = min(base, max_items);
        const uint32_t pos = c ? atomicAdd(&s_bucket[bucket_of(one ? own_postings : postings_of(q), c)], c) : 0u;
        for (uint32_t i = 0; i < c && base + i < max_items; ++i) {
            Item it;
            it.q = q;
            it.doc_lo = (uint32_t)((unsigned long long)ix.n_docs * i / c);
            it.doc_hi = (uint32_t)((unsigned long long)ix.n_docs * (i + 1) / c);
            it.m = nterms;
            bt.items[base + i] = it;
            if (pos + i < max_items) bt.item_order[pos + i] = base + i;
        }
        base += c;
    }
}

}  // namespace vbm25

#endif
