// maintain.hip -- VACUUM's compaction on the device (vbm25_index_maintain): an index, a bitmap of deleted sealed documents and a
// growing segment become ONE new sealed segment in HBM, crates/bm25/src/maintain.rs:27-298 of the reference (decode every block, drop
// and relabel the deleted documents, append the live growing documents, flush again: io.rs:187-197, flush.rs:40-158).  The result is
// the vbm25_device_segment build_device_core (flush.hip) makes of the mappings maintain.rs would write; the sealed postings never leave
// the device and are never sorted:
//   relabel     keep bits per 64-document word, popcount, exclusive scan: new id = base[w] + popcount(kept bits below)
//   count       one wave per sealed block: decode the ids, ballot the kept postings -> kept postings per block; +1 to the length of
//               every kept document (maintain.rs:344-362: a sealed document's new length is its number of postings)
//   vocabulary  growing keys binary-searched among the sealed keys (memcmp order = two big-endian u64); the unknown ones sorted and
//               de-duplicated; the two sorted lists merged by rank; per merged token: sealed kept + growing postings, tokens left
//               with none dropped, u64 exclusive scan -> term_start
//   scatter     one wave per sealed block again: decode ids and tfs, every kept (new id, tf) straight to its final slot (the relabel is
//               monotone and blocks are in (token, document) order, so a block's kept postings stay in order); the growing mappings
//               radix-sorted by (token rank, new id) and placed after their token's sealed postings (growing ids exceed every sealed id)
//   encode      build_device_core with the lengths, payloads and postings already in HBM
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "decode.h"

namespace {

using namespace vbm25;
using ull = unsigned long long;

// phase times of the last call on this thread (tools/maintain_cost.py): relabel, count, vocabulary, scatter, encode
thread_local double g_phase_ms[5];
// every byte the call copied over the host link, the encode's copies included (tools/vacuum_device_cost.py): [0] host -> device
// (deletion words, the growing arrays, the term keys; the new vocabulary's starts and first blocks), [1] device -> host (scalars,
// the new vocabulary's keys, starts and block boundaries, the relabel table when asked for)
thread_local double g_link_bytes[2];

// ---------------------------------------------------------------------------
// relabel
// ---------------------------------------------------------------------------
// keep word w = NOT deleted word w, the bits at or beyond n_docs cleared; cnt[w] = its popcount
__global__ void __launch_bounds__(256) mt_keep_kernel(uint32_t n_words, uint32_t n_docs, const ull *deleted, ull *keep, uint32_t *cnt) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += gridDim.x * blockDim.x) {
        ull k = deleted ? ~deleted[w] : ~0ull;
        if (w + 1 == n_words && (n_docs & 63u)) k &= (1ull << (n_docs & 63u)) - 1ull;
        keep[w] = k;
        cnt[w] = (uint32_t)__popcll(k);
    }
}

__device__ __forceinline__ uint32_t mt_new_id(const ull *keep, const uint32_t *base, uint32_t d, bool &kept) {
    const ull w = keep[d >> 6];
    const uint32_t s = d & 63u;
    kept = (w >> s) & 1ull;
    return base[d >> 6] + (uint32_t)__popcll(w & ((1ull << s) - 1ull));
}

struct SealedArgs {
    uint32_t n_docs, n_terms, n_blocks;
    const uint4 *blk_meta;            // (min_doc, max_doc, off8, n | meta_doc << 8 | meta_tf << 16 | ...)
    const uint8_t *blob;
    const uint32_t *term_first_block;  // n_terms + 1
    const ull *keep;                   // per 64 old ids
    const uint32_t *base;              // exclusive scan of the keep words' popcounts
    uint32_t *len;                     // per new id
    uint32_t *kept_blk;                // per block: kept postings
    const ull *blk_base;               // exclusive scan of kept_blk
    const ull *sbase;                  // per sealed term: final slot of its first kept posting - blk_base[its first block]
    uint32_t *post_doc, *post_tf;      // the output mappings
};

// The kept postings of block j among lanes' postings 2 lane, 2 lane + 1 (the ids of lanes past the block's end are not looked at:
// decode_doc_ids leaves them arbitrary).  Every lane of the wave must be here: decode_doc_ids' DPP scan reads them all.
__device__ __forceinline__ void mt_block_ids(const SealedArgs &a, uint32_t j, uint32_t lane, uint4 &m, uint32_t &i0, uint32_t &i1, bool &k0,
                                             bool &k1) {
    m = a.blk_meta[j];
    const uint32_t n = m.w & 0xffu, md = (m.w >> 8) & 0xffu;
    uint32_t d0, d1;
    decode_doc_ids(a.blob + 8ull * m.z, md, n, m.x, lane, d0, d1);
    k0 = k1 = false;
    i0 = i1 = 0;
    if (2 * lane < n && d0 < a.n_docs) i0 = mt_new_id(a.keep, a.base, d0, k0);
    if (2 * lane + 1 < n && d1 < a.n_docs) i1 = mt_new_id(a.keep, a.base, d1, k1);
}

// count: one wave per block.  A document holds at most one posting per token, so its count never reaches 2^32: the reference's
// saturating_add(1) never saturates and a plain atomic add is the same.
__global__ void __launch_bounds__(256) mt_count_kernel(SealedArgs a) {
    const uint32_t lane = threadIdx.x & 63, j = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (j >= a.n_blocks) return;  // (whole waves)
    uint4 m;
    uint32_t i0, i1;
    bool k0, k1;
    mt_block_ids(a, j, lane, m, i0, i1, k0, k1);
    if (k0) atomicAdd(&a.len[i0], 1u);
    if (k1) atomicAdd(&a.len[i1], 1u);
    const ull b0 = __ballot(k0), b1 = __ballot(k1);
    if (lane == 0) a.kept_blk[j] = (uint32_t)(__popcll(b0) + __popcll(b1));
}

// scatter: one wave per block; kept posting i goes to sbase[t] + blk_base[j] + (kept postings of the block before i)
__global__ void __launch_bounds__(256) mt_scatter_kernel(SealedArgs a) {
    const uint32_t lane = threadIdx.x & 63, j = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (j >= a.n_blocks) return;
    uint4 m;
    uint32_t i0, i1;
    bool k0, k1;
    mt_block_ids(a, j, lane, m, i0, i1, k0, k1);
    const ull b0 = __ballot(k0), b1 = __ballot(k1);
    if (!(b0 | b1)) return;
    const uint32_t n = m.w & 0xffu, md = (m.w >> 8) & 0xffu, mt = (m.w >> 16) & 0xffu;
    uint32_t f0, f1;
    decode_fields(a.blob + 8ull * m.z + ((payload_bytes(md, n) + 7u) & ~7u), mt, n, lane, f0, f1);
    uint32_t lo = 0, hi = a.n_terms;  // the term of block j
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.term_first_block[mid] <= j) lo = mid; else hi = mid;
    }
    const ull below = (1ull << lane) - 1ull;
    const ull at = a.sbase[lo] + a.blk_base[j] + (ull)(__popcll(b0 & below) + __popcll(b1 & below));
    if (k0) {
        a.post_doc[at] = i0;
        a.post_tf[at] = f0;
    }
    if (k1) {
        a.post_doc[at + (k0 ? 1u : 0u)] = i1;
        a.post_tf[at + (k0 ? 1u : 0u)] = f1;
    }
}

// payloads of the kept sealed documents at their new ids; the relabel table (optional)
__global__ void __launch_bounds__(256) mt_sealed_docs_kernel(uint32_t n_docs, const ull *keep, const uint32_t *base, const uint16_t *payload,
                                                             uint16_t *new_payload, uint32_t *relabel) {
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += gridDim.x * blockDim.x) {
        bool kept;
        const uint32_t id = mt_new_id(keep, base, d, kept);
        if (kept) {
            new_payload[3ull * id + 0] = payload[3ull * d + 0];
            new_payload[3ull * id + 1] = payload[3ull * d + 1];
            new_payload[3ull * id + 2] = payload[3ull * d + 2];
        }
        if (relabel) relabel[d] = kept ? id : 0xffffffffu;
    }
}

// ---------------------------------------------------------------------------
// vocabulary
// ---------------------------------------------------------------------------
// 16-byte keys -> (big-endian high half, big-endian low half): memcmp order is the order of the pairs
__global__ void __launch_bounds__(256) mt_key_split_kernel(uint64_t n, const ulonglong2 *key, ull *hi, ull *lo) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const ulonglong2 k = key[i];
        hi[i] = __builtin_bswap64(k.x);
        lo[i] = __builtin_bswap64(k.y);
    }
}

__device__ __forceinline__ bool mt_key_less(ull ah, ull al, ull bh, ull bl) { return ah < bh || (ah == bh && al < bl); }
// entries of the ascending list (hi, lo)[0 .. n) below (qh, ql)
__device__ __forceinline__ uint32_t mt_lower_bound(const ull *hi, const ull *lo, uint32_t n, ull qh, ull ql) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (mt_key_less(hi[m], lo[m], qh, ql)) a = m + 1; else b = m;
    }
    return a;
}

// tf 0 among the elements of a device CSR (Document::checked_new, vector.rs:56-64): the smallest document that holds one
// One thread per element, no grid cap and no stride (fewer than 2^31 elements: at most 2^23 workgroups).
__global__ void __launch_bounds__(256) mt_tf_zero_kernel(uint64_t n_el, uint32_t n_grow, const uint64_t *start, const uint32_t *tf, uint32_t *first) {
    const uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (e >= n_el || tf[e] != 0) return;
    uint32_t lo = 0, hi = n_grow;  // start[lo] <= e < start[hi]: the last such lo is e's document (empty documents lie below it)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= e) lo = mid; else hi = mid;
    }
    atomicMin(first, lo);
}

struct GrowArgs {
    uint32_t n_grow, n_terms, n_sealed_kept;
    const uint64_t *start;            // n_grow + 1, from 0
    const ull *key_hi, *key_lo;       // per element
    const uint32_t *tf;               // per element
    const uint8_t *deleted;           // per document, or NULL
    const uint16_t *payload;          // per document x 3
    const uint32_t *gnew;             // exclusive scan of the live documents
    const uint32_t *gel;              // exclusive scan of the live documents' elements
    const ull *skey_hi, *skey_lo;     // the sealed keys
    uint32_t *ext;                    // per element: sealed term t, or n_terms + new key number
    uint32_t *unk, *n_unk;            // elements whose key the sealed segment lacks
    const uint32_t *rank_of_ext;      // n_terms + new keys: merged rank
    ull *map_key;                     // per live element: rank << 32 | new id
    uint32_t *map_tf, *gcnt;          // ... its tf; growing postings per merged rank
    uint32_t *len;                    // per new id
    uint16_t *new_payload;
    uint32_t *relabel;                // + n_sealed, or NULL
};

__global__ void __launch_bounds__(256) mt_grow_live_kernel(uint32_t n_grow, const uint64_t *start, const uint8_t *deleted, uint32_t *live,
                                                           uint32_t *live_el) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_grow; g += gridDim.x * blockDim.x) {
        const bool l = !(deleted && deleted[g]);
        live[g] = l ? 1u : 0u;
        live_el[g] = l ? (uint32_t)(start[g + 1] - start[g]) : 0u;
    }
}

// one thread per live growing document: its keys looked up among the sealed keys
__global__ void __launch_bounds__(256) mt_grow_lookup_kernel(GrowArgs a) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < a.n_grow; g += gridDim.x * blockDim.x) {
        if (a.deleted && a.deleted[g]) continue;
        for (uint64_t e = a.start[g]; e < a.start[g + 1]; ++e) {
            const ull qh = a.key_hi[e], ql = a.key_lo[e];
            const uint32_t t = mt_lower_bound(a.skey_hi, a.skey_lo, a.n_terms, qh, ql);
            if (t < a.n_terms && a.skey_hi[t] == qh && a.skey_lo[t] == ql) {
                a.ext[e] = t;
            } else {
                a.unk[atomicAdd(a.n_unk, 1u)] = (uint32_t)e;
            }
        }
    }
}

__global__ void __launch_bounds__(256) mt_gather_u64_kernel(uint32_t n, const uint32_t *idx, const ull *src, ull *dst) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[idx[i]];
}
// the unknown elements in key order: first of its key -> 1
__global__ void __launch_bounds__(256) mt_unique_flag_kernel(uint32_t n, const uint32_t *idx, const ull *hi, const ull *lo, uint32_t *flag) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        flag[i] = (i == 0 || hi[idx[i]] != hi[idx[i - 1]] || lo[idx[i]] != lo[idx[i - 1]]) ? 1u : 0u;
}
// uid = inclusive scan - 1: the new key's number; its key written once
__global__ void __launch_bounds__(256) mt_unique_write_kernel(uint32_t n, uint32_t n_terms, const uint32_t *idx, const uint32_t *flag,
                                                              const uint32_t *incl, const ull *hi, const ull *lo, ull *nkey_hi, ull *nkey_lo,
                                                              uint32_t *ext) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t e = idx[i], u = incl[i] - 1u;
        ext[e] = n_terms + u;
        if (flag[i]) {
            nkey_hi[u] = hi[e];
            nkey_lo[u] = lo[e];
        }
    }
}

// merged rank of sealed term t: t + new keys below it; of new key u: u + sealed keys below it
__global__ void __launch_bounds__(256) mt_merge_kernel(uint32_t n_terms, uint32_t n_new, const ull *skey_hi, const ull *skey_lo,
                                                       const ull *nkey_hi, const ull *nkey_lo, uint32_t *rank_of_ext, uint32_t *ext_of_rank,
                                                       ulonglong2 *mkey) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_terms + n_new; x += gridDim.x * blockDim.x) {
        ull h, l;
        uint32_t r;
        if (x < n_terms) {
            h = skey_hi[x];
            l = skey_lo[x];
            r = x + mt_lower_bound(nkey_hi, nkey_lo, n_new, h, l);
        } else {
            h = nkey_hi[x - n_terms];
            l = nkey_lo[x - n_terms];
            r = (x - n_terms) + mt_lower_bound(skey_hi, skey_lo, n_terms, h, l);
        }
        rank_of_ext[x] = r;
        ext_of_rank[r] = x;
        mkey[r] = make_ulonglong2(__builtin_bswap64(h), __builtin_bswap64(l));  // (back to bytes)
    }
}

// one thread per growing document: its mappings, length, payload and relabel entry
__global__ void __launch_bounds__(256) mt_grow_map_kernel(GrowArgs a) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < a.n_grow; g += gridDim.x * blockDim.x) {
        const bool live = !(a.deleted && a.deleted[g]);
        const uint32_t id = a.n_sealed_kept + a.gnew[g];
        if (a.relabel) a.relabel[g] = live ? id : 0xffffffffu;
        if (!live) continue;
        ull length = 0;  // Document::length, vector.rs:77-83: saturating
        uint32_t slot = a.gel[g];
        for (uint64_t e = a.start[g]; e < a.start[g + 1]; ++e, ++slot) {
            const uint32_t r = a.rank_of_ext[a.ext[e]], tf = a.tf[e];
            a.map_key[slot] = (ull)r << 32 | id;
            a.map_tf[slot] = tf;
            atomicAdd(&a.gcnt[r], 1u);
            length += tf;
            if (length > 0xffffffffull) length = 0xffffffffull;
        }
        a.len[id] = (uint32_t)length;
        a.new_payload[3ull * id + 0] = a.payload[3ull * g + 0];
        a.new_payload[3ull * id + 1] = a.payload[3ull * g + 1];
        a.new_payload[3ull * id + 2] = a.payload[3ull * g + 2];
    }
}

// per merged rank: sealed kept postings + growing postings; non-empty flag
__global__ void __launch_bounds__(256) mt_term_count_kernel(uint32_t n_merged, uint32_t n_terms, const uint32_t *ext_of_rank,
                                                            const uint32_t *term_first_block, const ull *blk_base, const uint32_t *gcnt,
                                                            ull *skept, ull *total, uint32_t *nonempty) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_merged; r += gridDim.x * blockDim.x) {
        const uint32_t x = ext_of_rank[r];
        const ull s = x < n_terms ? blk_base[term_first_block[x + 1]] - blk_base[term_first_block[x]] : 0ull;
        skept[r] = s;
        total[r] = s + gcnt[r];
        nonempty[r] = (s + gcnt[r]) ? 1u : 0u;
    }
}

// the final vocabulary (tokens with postings left) and term_start; the sealed and growing slot bases
__global__ void __launch_bounds__(256) mt_finalize_kernel(uint32_t n_merged, uint32_t n_terms, const uint32_t *ext_of_rank,
                                                          const uint32_t *term_first_block, const ull *blk_base, const ull *ts_m,
                                                          const ull *skept, const ull *total, const uint32_t *fid, const uint32_t *gscan,
                                                          const ulonglong2 *mkey, ulonglong2 *key_f, ull *ts_f, ull *sbase, ull *gbase) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r <= n_merged; r += gridDim.x * blockDim.x) {
        if (r == n_merged) {
            ts_f[fid[r]] = ts_m[r];
            continue;
        }
        if (total[r]) {
            key_f[fid[r]] = mkey[r];
            ts_f[fid[r]] = ts_m[r];
        }
        gbase[r] = ts_m[r] + skept[r] - gscan[r];
        const uint32_t x = ext_of_rank[r];
        if (x < n_terms) sbase[x] = ts_m[r] - blk_base[term_first_block[x]];  // (modulo 2^64: blk_base[j] is added back)
    }
}

// the sorted growing mappings after their token's sealed postings
__global__ void __launch_bounds__(256) mt_grow_scatter_kernel(uint32_t n, const ull *key, const uint32_t *tf, const ull *gbase, uint32_t *post_doc,
                                                              uint32_t *post_tf) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const ull k = key[i];
        const ull at = gbase[k >> 32] + i;
        post_doc[at] = (uint32_t)k;
        post_tf[at] = tf[i];
    }
}

uint32_t grid_of(uint64_t n) { return grid_for(n, 256, 4096); }

// The result of compacting everything away: no documents, no tokens, no blocks (as an index over an empty table)
int empty_segment(const MaintainSource &s, std::unique_ptr<vbm25_device_segment> &out) {
    auto ds = std::make_unique<vbm25_device_segment>();
    ds->device = s.device;
    ds->k1 = s.k1;
    ds->b = s.b;
    ds->term_first_block.assign(1, 0);
    for (HbmArray *h : {&ds->d_term_df, &ds->d_term_wand_fn, &ds->d_term_wand_tf, &ds->d_blk_min, &ds->d_blk_max, &ds->d_blk_n,
                        &ds->d_blk_wand_fn, &ds->d_blk_wand_tf, &ds->d_blk_meta_doc, &ds->d_blk_meta_tf, &ds->d_blob, &ds->d_doc_fieldnorm,
                        &ds->d_doc_payload})
        HIP_TRY(h->alloc(0));
    HIP_TRY(ds->d_term_first_block.alloc(4));
    HIP_TRY(ds->d_blk_off8.alloc(4));
    HIP_TRY(hipMemset(ds->d_term_first_block.p, 0, 4));
    HIP_TRY(hipMemset(ds->d_blk_off8.p, 0, 4));
    HIP_TRY(hipDeviceSynchronize());
    out = std::move(ds);
    return VBM25_OK;
}

}  // namespace

namespace vbm25 {

int maintain_device(const MaintainSource &s, const MaintainInput &in, uint32_t *relabel, vbm25_device_segment **out) {
    using clock = std::chrono::steady_clock;
    for (double &x : g_phase_ms) x = 0.0;
    for (double &x : g_link_bytes) x = 0.0;
    const uint32_t N = s.n_docs, T = s.n_terms, B = s.n_blocks, W = (N + 63u) / 64u;
    const vbm25_device_vacuum *dev = in.dev;
    const uint64_t *sealed_deleted = dev ? nullptr : in.sealed_deleted;
    const vbm25_growing_desc *growing = dev ? nullptr : in.growing;
    // arguments (all on the host, before the device is touched)
    if (dev && dev->device != s.device)
        return set_error(VBM25_ERR_INVALID, "the compaction inputs are on device %d, the index on device %d", dev->device, s.device);
    if (dev && dev->n_sealed != N)
        return set_error(VBM25_ERR_INVALID, "the compaction inputs are of %u sealed documents, the index holds %u", dev->n_sealed, N);
    if (sealed_deleted && (N & 63u) && (sealed_deleted[W - 1] >> (N & 63u)))
        return set_error(VBM25_ERR_INVALID, "sealed_deleted has bits at or beyond n_docs = %u", N);
    const uint32_t G = dev ? dev->n_grow : growing ? growing->n_docs : 0u;
    uint64_t e_first = 0, n_el = dev ? dev->n_elements : 0;
    if (G && !dev) {
        const vbm25_growing_desc *d = growing;
        if (!d->start || !d->payload) return set_error(VBM25_ERR_INVALID, "growing arrays missing");
        for (uint32_t g = 0; g < G; ++g)
            if (d->start[g + 1] < d->start[g]) return set_error(VBM25_ERR_INVALID, "start not monotone at growing document %u", g);
        if (d->start[G] > d->n_elements)
            return set_error(VBM25_ERR_INVALID, "start reaches element %llu of %llu", (unsigned long long)d->start[G],
                             (unsigned long long)d->n_elements);
        e_first = d->start[0];
        n_el = d->start[G] - e_first;
        if (n_el && (!d->key || !d->tf)) return set_error(VBM25_ERR_INVALID, "growing arrays missing");
        if (n_el >= (1ull << 31)) return set_error(VBM25_ERR_UNSUPPORTED, "%llu growing elements: the device path takes fewer than 2^31",
                                                   (unsigned long long)n_el);
        for (uint32_t g = 0; g < G; ++g)  // Document::checked_new, vector.rs:56-64
            for (uint64_t e = d->start[g]; e < d->start[g + 1]; ++e) {
                if (d->tf[e] == 0) return set_error(VBM25_ERR_INVALID, "growing document %u: tf 0", g);
                if (e > d->start[g] && std::memcmp(d->key + 16ull * (e - 1), d->key + 16ull * e, 16) >= 0)
                    return set_error(VBM25_ERR_INVALID, "growing document %u: keys must be strictly ascending", g);
            }
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return set_error(VBM25_ERR_DEVICE, "no HIP device: maintain has no CPU entry point");
    HIP_TRY(hipSetDevice(s.device));
    if (dev && n_el) {  // the host loop's tf check on the handle's planes (its keys were checked when the handle was made)
        HbmArray d_first;
        uint32_t first = 0xffffffffu;
        HIP_TRY(d_first.alloc(4));
        HIP_TRY(hipMemset(d_first.p, 0xff, 4));
        mt_tf_zero_kernel<<<(uint32_t)((n_el + 255) / 256), 256>>>(n_el, G, dev->d_start.as<uint64_t>(), dev->d_tf.as<uint32_t>(), d_first.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&first, d_first.p, 4, hipMemcpyDeviceToHost));
        g_link_bytes[1] += 4;
        if (first != 0xffffffffu) return set_error(VBM25_ERR_INVALID, "growing document %u: tf 0", first);
    }
    auto t0 = clock::now();
    auto lap = [&](int phase) -> hipError_t {
        const hipError_t e = hipDeviceSynchronize();
        const auto t1 = clock::now();
        g_phase_ms[phase] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return e;
    };

    // relabel
    HbmArray d_del, d_keep, d_cnt, d_base, tmp;
    HIP_TRY(d_keep.alloc(8ull * W));
    HIP_TRY(d_cnt.alloc(4ull * (W + 1ull)));
    HIP_TRY(d_base.alloc(4ull * (W + 1ull)));
    uint32_t K = 0;
    if (W) {
        const ull *del_words = dev ? dev->d_sealed_deleted.as<ull>() : nullptr;  // (the handle's words: read in place)
        if (sealed_deleted) {
            HIP_TRY(d_del.alloc(8ull * W));
            HIP_TRY(hipMemcpy(d_del.p, sealed_deleted, 8ull * W, hipMemcpyHostToDevice));
            g_link_bytes[0] += 8.0 * W;
            del_words = d_del.as<ull>();
        }
        HIP_TRY(hipMemset(d_cnt.as<uint32_t>() + W, 0, 4));
        mt_keep_kernel<<<grid_of(W), 256>>>(W, N, del_words, d_keep.as<ull>(), d_cnt.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, d_cnt.as<uint32_t>(), d_base.as<uint32_t>(), (int)(W + 1)); }));
        HIP_TRY(hipMemcpy(&K, d_base.as<uint32_t>() + W, 4, hipMemcpyDeviceToHost));
        g_link_bytes[1] += 4;
        d_del.release();
    }
    HIP_TRY(lap(0));

    // count (lengths of the kept sealed documents, kept postings per block)
    HbmArray d_len, d_pay, d_kept_blk, d_blk_base;
    HIP_TRY(d_len.alloc(4ull * (uint64_t(N) + G)));
    HIP_TRY(d_pay.alloc(6ull * (uint64_t(N) + G)));
    HIP_TRY(d_kept_blk.alloc(4ull * (B + 1ull)));
    HIP_TRY(d_blk_base.alloc(8ull * (B + 1ull)));
    HIP_TRY(hipMemset(d_len.p, 0, 4ull * (uint64_t(N) + G)));
    HIP_TRY(hipMemset(d_kept_blk.p, 0, 4ull * (B + 1ull)));
    SealedArgs sa{};
    sa.n_docs = N;
    sa.n_terms = T;
    sa.n_blocks = B;
    sa.blk_meta = s.blk_meta;
    sa.blob = s.blob;
    sa.term_first_block = s.term_first_block;
    sa.keep = d_keep.as<ull>();
    sa.base = d_base.as<uint32_t>();
    sa.len = d_len.as<uint32_t>();
    sa.kept_blk = d_kept_blk.as<uint32_t>();
    sa.blk_base = d_blk_base.as<ull>();
    if (B) {
        mt_count_kernel<<<(B + 3) / 4, 256>>>(sa);
        HIP_TRY(hipGetLastError());
    }
    {
        hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *> wide(d_kept_blk.as<uint32_t>(), WidenU32());
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, wide, d_blk_base.as<ull>(), (int)(B + 1)); }));
    }
    HIP_TRY(lap(1));

    // vocabulary
    HbmArray d_skey, d_shi, d_slo, d_start, d_gkey, d_ghi, d_glo, d_gtf, d_gdel, d_gpay, d_live, d_live_el, d_gnew, d_gel, d_ext, d_unk, d_nunk;
    HIP_TRY(d_skey.alloc(16ull * T));
    HIP_TRY(d_shi.alloc(8ull * T));
    HIP_TRY(d_slo.alloc(8ull * T));
    if (T) {
        HIP_TRY(hipMemcpy(d_skey.p, s.term_key, 16ull * T, hipMemcpyHostToDevice));
        g_link_bytes[0] += 16.0 * T;
        mt_key_split_kernel<<<grid_of(T), 256>>>(T, d_skey.as<ulonglong2>(), d_shi.as<ull>(), d_slo.as<ull>());
        HIP_TRY(hipGetLastError());
    }
    d_skey.release();
    uint32_t Gk = 0, n_gel = 0, U = 0;
    HIP_TRY(d_gnew.alloc(4ull * (G + 1ull)));
    HIP_TRY(d_gel.alloc(4ull * (G + 1ull)));
    HIP_TRY(d_ext.alloc(4ull * n_el));
    HIP_TRY(d_unk.alloc(4ull * n_el));
    HIP_TRY(d_nunk.alloc(4));
    HIP_TRY(hipMemset(d_nunk.p, 0, 4));
    GrowArgs ga{};
    if (G) {
        // the growing arrays: the handle's planes where they are (only read: nothing of the handle is freed or written), or the host
        // arrays' copies in buffers of the call
        const uint64_t *g_start = nullptr;
        const ulonglong2 *g_key = nullptr;
        const uint32_t *g_tf = nullptr;
        const uint8_t *g_del = nullptr;
        const uint16_t *g_pay = nullptr;
        HIP_TRY(d_ghi.alloc(8ull * n_el));
        HIP_TRY(d_glo.alloc(8ull * n_el));
        HIP_TRY(d_live.alloc(4ull * (G + 1ull)));
        HIP_TRY(d_live_el.alloc(4ull * (G + 1ull)));
        if (dev) {
            g_start = dev->d_start.as<uint64_t>();
            g_key = dev->d_key.as<ulonglong2>();
            g_tf = dev->d_tf.as<uint32_t>();
            g_del = dev->d_deleted.as<uint8_t>();
            g_pay = dev->d_payload.as<uint16_t>();
        } else {
            std::vector<uint64_t> start(size_t(G) + 1);
            for (uint32_t g = 0; g <= G; ++g) start[g] = growing->start[g] - e_first;
            HIP_TRY(d_start.alloc(8ull * (G + 1ull)));
            HIP_TRY(hipMemcpy(d_start.p, start.data(), 8ull * (G + 1ull), hipMemcpyHostToDevice));
            HIP_TRY(d_gkey.alloc(16ull * n_el));
            HIP_TRY(d_gtf.alloc(4ull * n_el));
            HIP_TRY(d_gpay.alloc(6ull * G));
            if (n_el) {
                HIP_TRY(hipMemcpy(d_gkey.p, growing->key + 16ull * e_first, 16ull * n_el, hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(d_gtf.p, growing->tf + e_first, 4ull * n_el, hipMemcpyHostToDevice));
            }
            if (growing->deleted) {
                HIP_TRY(d_gdel.alloc(G));
                HIP_TRY(hipMemcpy(d_gdel.p, growing->deleted, G, hipMemcpyHostToDevice));
                g_del = d_gdel.as<uint8_t>();
            }
            HIP_TRY(hipMemcpy(d_gpay.p, growing->payload, 6ull * G, hipMemcpyHostToDevice));
            g_link_bytes[0] += 8.0 * (G + 1.0) + 20.0 * n_el + 6.0 * G + (growing->deleted ? G : 0);
            g_start = d_start.as<uint64_t>();
            g_key = d_gkey.as<ulonglong2>();
            g_tf = d_gtf.as<uint32_t>();
            g_pay = d_gpay.as<uint16_t>();
        }
        if (n_el) {
            mt_key_split_kernel<<<grid_of(n_el), 256>>>(n_el, g_key, d_ghi.as<ull>(), d_glo.as<ull>());
            HIP_TRY(hipGetLastError());
        }
        d_gkey.release();  // (after the split on the null stream: hipFree waits for it)
        HIP_TRY(hipMemset(d_live.as<uint32_t>() + G, 0, 4));
        HIP_TRY(hipMemset(d_live_el.as<uint32_t>() + G, 0, 4));
        mt_grow_live_kernel<<<grid_of(G), 256>>>(G, g_start, g_del, d_live.as<uint32_t>(), d_live_el.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, d_live.as<uint32_t>(), d_gnew.as<uint32_t>(), (int)(G + 1)); }));
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, d_live_el.as<uint32_t>(), d_gel.as<uint32_t>(), (int)(G + 1)); }));
        HIP_TRY(hipMemcpy(&Gk, d_gnew.as<uint32_t>() + G, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&n_gel, d_gel.as<uint32_t>() + G, 4, hipMemcpyDeviceToHost));
        g_link_bytes[1] += 8;
        ga.n_grow = G;
        ga.n_terms = T;
        ga.n_sealed_kept = K;
        ga.start = g_start;
        ga.key_hi = d_ghi.as<ull>();
        ga.key_lo = d_glo.as<ull>();
        ga.tf = g_tf;
        ga.deleted = g_del;
        ga.payload = g_pay;
        ga.gnew = d_gnew.as<uint32_t>();
        ga.gel = d_gel.as<uint32_t>();
        ga.skey_hi = d_shi.as<ull>();
        ga.skey_lo = d_slo.as<ull>();
        ga.ext = d_ext.as<uint32_t>();
        ga.unk = d_unk.as<uint32_t>();
        ga.n_unk = d_nunk.as<uint32_t>();
        if (n_el) {
            mt_grow_lookup_kernel<<<grid_of(G), 256>>>(ga);
            HIP_TRY(hipGetLastError());
        }
    }
    if (uint64_t(K) + Gk > 0xffffffffull)  // io.rs:53-56: ids 0 .. 2^32 - 2, id u32::MAX is never given out
        return set_error(VBM25_ERR_INVALID, "%u sealed + %u growing documents: more than 2^32 - 1", K, Gk);
    const uint32_t N2 = K + Gk;
    if (N2 == 0) {  // nothing left: the empty segment
        std::unique_ptr<vbm25_device_segment> ds;
        if (int rc = empty_segment(s, ds)) return rc;
        if (relabel) std::fill(relabel, relabel + uint64_t(N) + G, 0xffffffffu);
        *out = ds.release();
        return VBM25_OK;
    }
    uint32_t n_unk = 0;
    HIP_TRY(hipMemcpy(&n_unk, d_nunk.p, 4, hipMemcpyDeviceToHost));
    g_link_bytes[1] += 4;
    HbmArray d_nhi, d_nlo;
    if (n_unk) {  // sort the unknown elements by key: low halves, then (stable) high halves
        HbmArray k1, k2, v2, fl, incl;
        HIP_TRY(k1.alloc(8ull * n_unk));
        HIP_TRY(k2.alloc(8ull * n_unk));
        HIP_TRY(v2.alloc(4ull * n_unk));
        mt_gather_u64_kernel<<<grid_of(n_unk), 256>>>(n_unk, d_unk.as<uint32_t>(), d_glo.as<ull>(), k1.as<ull>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) {
            return hipcub::DeviceRadixSort::SortPairs(t, tb, k1.as<ull>(), k2.as<ull>(), d_unk.as<uint32_t>(), v2.as<uint32_t>(), (int)n_unk);
        }));
        mt_gather_u64_kernel<<<grid_of(n_unk), 256>>>(n_unk, v2.as<uint32_t>(), d_ghi.as<ull>(), k1.as<ull>());
        HIP_TRY(hipGetLastError());
        size_t tb = tmp.bytes;  // (the same sort with the value arrays exchanged: the first one's temporary storage serves it)
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, k1.as<ull>(), k2.as<ull>(), v2.as<uint32_t>(), d_unk.as<uint32_t>(), (int)n_unk));
        HIP_TRY(fl.alloc(4ull * n_unk));
        HIP_TRY(incl.alloc(4ull * n_unk));
        mt_unique_flag_kernel<<<grid_of(n_unk), 256>>>(n_unk, d_unk.as<uint32_t>(), d_ghi.as<ull>(), d_glo.as<ull>(), fl.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::InclusiveSum(t, tb, fl.as<uint32_t>(), incl.as<uint32_t>(), (int)n_unk); }));
        HIP_TRY(hipMemcpy(&U, incl.as<uint32_t>() + (n_unk - 1), 4, hipMemcpyDeviceToHost));
        g_link_bytes[1] += 4;
        HIP_TRY(d_nhi.alloc(8ull * U));
        HIP_TRY(d_nlo.alloc(8ull * U));
        mt_unique_write_kernel<<<grid_of(n_unk), 256>>>(n_unk, T, d_unk.as<uint32_t>(), fl.as<uint32_t>(), incl.as<uint32_t>(), d_ghi.as<ull>(),
                                                        d_glo.as<ull>(), d_nhi.as<ull>(), d_nlo.as<ull>(), d_ext.as<uint32_t>());
        HIP_TRY(hipGetLastError());
    }
    if (uint64_t(T) + U > 0xfffffff0ull) return set_error(VBM25_ERR_UNSUPPORTED, "more than 2^32 tokens");
    const uint32_t M = T + U;
    HbmArray d_rank, d_src, d_mkey, d_gcnt, d_gscan, d_skept, d_total, d_ts_m, d_nz, d_fid, d_key_f, d_ts_f, d_sbase, d_gbase, d_mkey_tf, d_mtf;
    HIP_TRY(d_rank.alloc(4ull * M));
    HIP_TRY(d_src.alloc(4ull * M));
    HIP_TRY(d_mkey.alloc(16ull * M));
    HIP_TRY(d_gcnt.alloc(4ull * (M + 1ull)));
    HIP_TRY(hipMemset(d_gcnt.p, 0, 4ull * (M + 1ull)));
    if (M) {
        mt_merge_kernel<<<grid_of(M), 256>>>(T, U, d_shi.as<ull>(), d_slo.as<ull>(), d_nhi.as<ull>(), d_nlo.as<ull>(), d_rank.as<uint32_t>(),
                                              d_src.as<uint32_t>(), d_mkey.as<ulonglong2>());
        HIP_TRY(hipGetLastError());
    }
    // the growing mappings (rank << 32 | new id, tf), lengths, payloads, relabel entries
    HbmArray d_relabel;
    if (relabel) HIP_TRY(d_relabel.alloc(4ull * (uint64_t(N) + G)));
    HIP_TRY(d_mkey_tf.alloc(8ull * n_gel));
    HIP_TRY(d_mtf.alloc(4ull * n_gel));
    if (G) {
        ga.rank_of_ext = d_rank.as<uint32_t>();
        ga.map_key = d_mkey_tf.as<ull>();
        ga.map_tf = d_mtf.as<uint32_t>();
        ga.gcnt = d_gcnt.as<uint32_t>();
        ga.len = d_len.as<uint32_t>();
        ga.new_payload = d_pay.as<uint16_t>();
        ga.relabel = relabel ? d_relabel.as<uint32_t>() + N : nullptr;
        mt_grow_map_kernel<<<grid_of(G), 256>>>(ga);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(d_skept.alloc(8ull * (M + 1ull)));
    HIP_TRY(d_total.alloc(8ull * (M + 1ull)));
    HIP_TRY(d_ts_m.alloc(8ull * (M + 1ull)));
    HIP_TRY(d_nz.alloc(4ull * (M + 1ull)));
    HIP_TRY(d_fid.alloc(4ull * (M + 1ull)));
    HIP_TRY(d_gscan.alloc(4ull * (M + 1ull)));
    HIP_TRY(hipMemset(d_total.as<ull>() + M, 0, 8));
    HIP_TRY(hipMemset(d_nz.as<uint32_t>() + M, 0, 4));
    if (M) {
        mt_term_count_kernel<<<grid_of(M), 256>>>(M, T, d_src.as<uint32_t>(), s.term_first_block, d_blk_base.as<ull>(), d_gcnt.as<uint32_t>(),
                                                   d_skept.as<ull>(), d_total.as<ull>(), d_nz.as<uint32_t>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, d_total.as<ull>(), d_ts_m.as<ull>(), (int)(M + 1)); }));
    HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, d_nz.as<uint32_t>(), d_fid.as<uint32_t>(), (int)(M + 1)); }));
    HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, d_gcnt.as<uint32_t>(), d_gscan.as<uint32_t>(), (int)(M + 1)); }));
    uint32_t F = 0;
    uint64_t P = 0;
    HIP_TRY(hipMemcpy(&F, d_fid.as<uint32_t>() + M, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&P, d_ts_m.as<ull>() + M, 8, hipMemcpyDeviceToHost));
    g_link_bytes[1] += 12;
    HIP_TRY(d_key_f.alloc(16ull * F));
    HIP_TRY(d_ts_f.alloc(8ull * (F + 1ull)));
    HIP_TRY(d_sbase.alloc(8ull * T));
    HIP_TRY(d_gbase.alloc(8ull * M));
    mt_finalize_kernel<<<grid_of(M + 1ull), 256>>>(M, T, d_src.as<uint32_t>(), s.term_first_block, d_blk_base.as<ull>(), d_ts_m.as<ull>(),
                                                   d_skept.as<ull>(), d_total.as<ull>(), d_fid.as<uint32_t>(), d_gscan.as<uint32_t>(),
                                                   d_mkey.as<ulonglong2>(), d_key_f.as<ulonglong2>(), d_ts_f.as<ull>(), d_sbase.as<ull>(),
                                                   d_gbase.as<ull>());
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> key_f(16ull * F);
    std::vector<uint64_t> ts_f(size_t(F) + 1);
    if (F) HIP_TRY(hipMemcpy(key_f.data(), d_key_f.p, 16ull * F, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ts_f.data(), d_ts_f.p, 8ull * (F + 1ull), hipMemcpyDeviceToHost));
    g_link_bytes[1] += 16.0 * F + 8.0 * (F + 1.0);
    for (HbmArray *b : {&d_rank, &d_mkey, &d_skept, &d_total, &d_nz, &d_fid, &d_gscan, &d_key_f, &d_ts_f, &d_ghi, &d_glo, &d_shi, &d_slo, &d_ext,
                    &d_unk, &d_gtf})
        b->release();
    HIP_TRY(lap(2));

    // scatter
    HbmArray d_doc, d_tf;
    HIP_TRY(d_doc.alloc(4ull * P));
    HIP_TRY(d_tf.alloc(4ull * P));
    sa.sbase = d_sbase.as<ull>();
    sa.post_doc = d_doc.as<uint32_t>();
    sa.post_tf = d_tf.as<uint32_t>();
    if (B) {
        mt_scatter_kernel<<<(B + 3) / 4, 256>>>(sa);
        HIP_TRY(hipGetLastError());
    }
    if (N) {
        mt_sealed_docs_kernel<<<grid_of(N), 256>>>(N, d_keep.as<ull>(), d_base.as<uint32_t>(), s.doc_payload, d_pay.as<uint16_t>(),
                                                   relabel ? d_relabel.as<uint32_t>() : nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (n_gel) {
        int end_bit = 32;  // the new id and as much of the rank as M needs
        while (end_bit < 64 && (uint64_t(M) >> (end_bit - 32)) != 0) ++end_bit;
        HbmArray k2, v2;
        HIP_TRY(k2.alloc(8ull * n_gel));
        HIP_TRY(v2.alloc(4ull * n_gel));
        hipcub::DoubleBuffer<ull> keys(d_mkey_tf.as<ull>(), k2.as<ull>());
        hipcub::DoubleBuffer<uint32_t> vals(d_mtf.as<uint32_t>(), v2.as<uint32_t>());
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceRadixSort::SortPairs(t, tb, keys, vals, (int)n_gel, 0, end_bit); }));
        mt_grow_scatter_kernel<<<grid_of(n_gel), 256>>>(n_gel, keys.Current(), vals.Current(), d_gbase.as<ull>(), d_doc.as<uint32_t>(),
                                                        d_tf.as<uint32_t>());
        HIP_TRY(hipGetLastError());
    }
    if (relabel) {
        HIP_TRY(hipMemcpy(relabel, d_relabel.p, 4ull * (uint64_t(N) + G), hipMemcpyDeviceToHost));
        g_link_bytes[1] += 4.0 * (double(N) + G);
    }
    for (HbmArray *b : {&d_keep, &d_cnt, &d_base, &d_kept_blk, &d_blk_base, &d_sbase, &d_gbase, &d_mkey_tf, &d_mtf, &d_relabel, &d_start, &d_gdel,
                    &d_gpay, &d_live, &d_live_el, &d_gnew, &d_gel, &tmp, &d_src, &d_gcnt, &d_ts_m})
        b->release();
    HIP_TRY(lap(3));

    // encode
    std::unique_ptr<vbm25_device_segment> ds;
    if (int rc = build_device_core(s.device, s.k1, s.b, N2, nullptr, d_len.as<uint32_t>(), nullptr, d_pay.as<uint16_t>(), F, key_f.data(),
                                   ts_f.data(), nullptr, nullptr, d_doc.as<uint32_t>(), d_tf.as<uint32_t>(), ds))
        return rc;
    double encode[2];
    encode_link_bytes(encode);
    g_link_bytes[0] += encode[0];
    g_link_bytes[1] += encode[1];
    HIP_TRY(lap(4));
    *out = ds.release();
    return VBM25_OK;
}

// ---------------------------------------------------------------------------
// vbm25_filter_remap: a filter's bitmaps carried across the compaction (filter.hip owns the filters and checks the arguments)
// ---------------------------------------------------------------------------
// The old documents are one run of input words: the sealed bitmaps' W words, then the growing bitmaps' GW words.  keep / base are the
// relabel's pair over that run (mt_keep_kernel per side, ONE exclusive scan over both), so base[w] is input word w's first OUTPUT BIT:
// the growing side starts at bit n_kept, whatever n_kept % 64 is.  One thread per input word with a kept bit: the kept bits of the
// word compressed to its low end (the parallel-suffix compress of Hacker's Delight 7-4, its six move masks a function of keep[w] alone
// and so computed once for all F bitmaps) and ORed into the one or two output words at bit base[w].  Output words are shared between
// neighbouring input words (and between the last sealed and the first growing one): the output is zeroed first and written with
// atomicOr, which commutes -- the result does not depend on the order.  A run of fully deleted words costs its threads one load each.
namespace {
// n bytes (nonzero = deleted) -> ceil(n / 64) words, bit g % 64 of word g / 64: one wave per word, a ballot of its 64 bytes
__global__ void __launch_bounds__(256) mt_pack_deleted_kernel(uint32_t n, const uint8_t *deleted, ull *words) {
    const uint32_t lane = threadIdx.x & 63u, w = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (w >= (n + 63u) / 64u) return;  // (whole waves)
    const uint64_t g = 64ull * w + lane;
    const ull m = __ballot(g < n && deleted[g] != 0);
    if (lane == 0) words[w] = m;
}

__global__ void __launch_bounds__(256) filter_remap_kernel(uint32_t n_in, uint32_t n_sealed_words, const ull *keep, const uint32_t *base,
                                                           const ull *bits, const ull *grow_bits, uint32_t grow_stride, uint32_t n_bitmaps,
                                                           ull *out, uint32_t out_words) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n_in; w += gridDim.x * blockDim.x) {
        const ull k = keep[w];  // (the tail word's bits at or beyond the document count are cleared)
        if (!k) continue;
        ull m = k, mk = ~k << 1, mv[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            ull mp = mk ^ (mk << 1);
            mp ^= mp << 2;
            mp ^= mp << 4;
            mp ^= mp << 8;
            mp ^= mp << 16;
            mp ^= mp << 32;
            mv[i] = mp & m;
            m = (m ^ mv[i]) | (mv[i] >> (1 << i));
            mk &= ~mp;
        }
        const uint32_t at = base[w], ow = at >> 6, sh = at & 63u;
        const bool sealed = w < n_sealed_words;
        const ull *src = sealed ? bits + w : grow_bits + (w - n_sealed_words);
        const size_t stride = sealed ? n_sealed_words : grow_stride;
        for (uint32_t f = 0; f < n_bitmaps; ++f) {
            ull x = src[f * stride] & k;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const ull t = x & mv[i];
                x = (x ^ t) | (t >> (1 << i));
            }
            if (!x) continue;
            ull *o = out + size_t(f) * out_words + ow;
            atomicOr(o, x << sh);
            // (sh == 0: the word takes all 64 bits, and a shift by 64 is undefined)
            if (sh && (x >> (64u - sh)) && ow + 1u < out_words) atomicOr(o + 1, x >> (64u - sh));
        }
    }
}
}  // namespace

int filter_remap_device(int device, uint32_t n_bitmaps, uint32_t n_docs, const void *bits, uint32_t n_grow, const RemapDeletions &in,
                        const void *grow_bits, uint32_t grow_stride, uint32_t new_n_docs, void *out) {
    const bool deletions_on_device = in.dev != nullptr;
    const uint64_t *sealed_deleted = in.dev ? nullptr : in.sealed_deleted;
    const uint8_t *growing_deleted = in.dev || !n_grow ? nullptr : in.growing_deleted;
    const uint32_t W = (n_docs + 63u) / 64u, GW = (n_grow + 63u) / 64u, OW = (new_n_docs + 63u) / 64u;
    const uint64_t TW = uint64_t(W) + GW;
    // growing_deleted packed to the polarity and the form of sealed_deleted: both sides go through mt_keep_kernel.  Host inputs are
    // packed here and go up as one run of words; device inputs stay where they are, the bytes packed by mt_pack_deleted_kernel
    std::vector<ull> del(!deletions_on_device && (sealed_deleted || growing_deleted) ? TW : 0, 0ull);
    if (!del.empty() && sealed_deleted) std::copy(sealed_deleted, sealed_deleted + W, del.begin());
    if (!del.empty() && growing_deleted)
        for (uint32_t g = 0; g < n_grow; ++g)
            if (growing_deleted[g]) del[W + (g >> 6)] |= 1ull << (g & 63u);
    HIP_TRY(hipSetDevice(device));
    HbmArray d_del, d_keep, d_cnt, d_base, tmp;
    uint32_t got[2] = {0, 0};  // kept sealed documents, kept sealed + live growing
    if (TW) {
        HIP_TRY(d_keep.alloc(8ull * TW));
        HIP_TRY(d_cnt.alloc(4ull * (TW + 1ull)));
        HIP_TRY(d_base.alloc(4ull * (TW + 1ull)));
        const ull *sealed_words = nullptr, *grow_words = nullptr;
        if (!del.empty()) {
            HIP_TRY(d_del.alloc(8ull * TW));
            HIP_TRY(hipMemcpy(d_del.p, del.data(), 8ull * TW, hipMemcpyHostToDevice));
            if (sealed_deleted) sealed_words = d_del.as<ull>();
            if (growing_deleted) grow_words = d_del.as<ull>() + W;
        } else if (deletions_on_device) {
            sealed_words = in.dev->d_sealed_deleted.as<ull>();
            if (GW) {
                HIP_TRY(d_del.alloc(8ull * GW));
                mt_pack_deleted_kernel<<<(GW + 3) / 4, 256>>>(n_grow, in.dev->d_deleted.as<uint8_t>(), d_del.as<ull>());
                HIP_TRY(hipGetLastError());
                grow_words = d_del.as<ull>();
            }
        }
        HIP_TRY(hipMemset(d_cnt.as<uint32_t>() + TW, 0, 4));
        if (W) mt_keep_kernel<<<grid_of(W), 256>>>(W, n_docs, sealed_words, d_keep.as<ull>(), d_cnt.as<uint32_t>());
        if (GW) mt_keep_kernel<<<grid_of(GW), 256>>>(GW, n_grow, grow_words, d_keep.as<ull>() + W, d_cnt.as<uint32_t>() + W);
        HIP_TRY(hipGetLastError());
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, d_cnt.as<uint32_t>(), d_base.as<uint32_t>(), (int)uint32_t(TW + 1ull)); }));
        HIP_TRY(hipMemcpy(&got[0], d_base.as<uint32_t>() + W, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&got[1], d_base.as<uint32_t>() + TW, 4, hipMemcpyDeviceToHost));
    }
    if (got[1] != new_n_docs)
        return set_error(VBM25_ERR_INVALID, "%u kept sealed + %u live growing documents = %u, the new index holds %u: the filter is being "
                                            "remapped against another compaction", got[0], got[1] - got[0], got[1], new_n_docs);
    if (!OW) return VBM25_OK;
    HIP_TRY(hipMemset(out, 0, 8ull * n_bitmaps * OW));
    filter_remap_kernel<<<grid_of(TW), 256>>>(uint32_t(TW), W, d_keep.as<ull>(), d_base.as<uint32_t>(), static_cast<const ull *>(bits),
                                              static_cast<const ull *>(grow_bits), grow_stride, n_bitmaps, static_cast<ull *>(out), OW);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return VBM25_OK;
}

}  // namespace vbm25

// tools/maintain_cost.py: the phases of the calling thread's last vbm25_index_maintain (not part of include/vbm25.h)
// ... and every byte it copied over the host link, the encode included: [0] host -> device, [1] device -> host
extern "C" int vbm25_debug_maintain_link_bytes(double *out2) {
    if (!out2) return VBM25_ERR_INVALID;
    for (int i = 0; i < 2; ++i) out2[i] = g_link_bytes[i];
    return VBM25_OK;
}
extern "C" int vbm25_debug_maintain_phases(double *ms5) {
    if (!ms5) return VBM25_ERR_INVALID;
    for (int i = 0; i < 5; ++i) ms5[i] = g_phase_ms[i];
    return VBM25_OK;
}
