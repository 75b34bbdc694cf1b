// forward.hip -- the forward index of a sealed index, built on the device (vbm25_index_bind): the transpose of the index's postings
// into a vbm25_doc_terms -- per document its ascending term ids with their tfs and its fieldnorm code -- which the evaluate operator,
// the scorer and the reranker ring read as they read a handle bound from cast documents (evaluate_shared.h).  Everything comes from
// the index's HBM arrays; nothing is uploaded.  forward_lane.h holds the per-lane functions.
//
//   on a stream of the call's own:
//     fwd_count_kernel     one wave a block, the waves stride the blocks: the block's document ids (decode_doc_ids), one atomic add
//                          a posting into counts[doc]
//     (scan)               exclusive sum of the counts in 64 bits (hipcub) -> start, n_docs + 1 entries
//     fwd_classify_kernel  one lane a document: the class of its run (run_class) from start.  The documents of the workgroup class
//                          and of the long class go on a list each (a ballot and one atomic add a wave); a long run also reserves
//                          its place in the fallback's buffers.  The class counts are the call's one host read-back, with the
//                          posting total that sizes the result.
//     fwd_scatter_kernel   one wave a block again: ids, tfs (decode_fields) and the block's post_fn bytes; the block's term by
//                          bisection of term_first_block; each posting's slot is what the atomic add on its document's cursor
//                          returned (the counters, zeroed).  (term, tf) to start[doc] + slot, the fieldnorm byte to fieldnorm[doc].
//     fwd_sort_wave_kernel one wave a document of the wave class (<= 64 postings): one element a lane, a bitonic network in
//                          registers, the partner's element through ds_bpermute
//     fwd_sort_group_kernel  one workgroup a listed document (<= 2048 postings): a bitonic network in 16 KiB of LDS, a thread a pair
//     the long runs        fwd_long_copy_kernel gathers them into one buffer, hipcub::DeviceSegmentedRadixSort sorts its segments,
//                          fwd_long_copy_kernel puts them back: a double buffer of the long runs' size, not of the index's
//   The cursor order is arbitrary; term ids inside a document are distinct, so the sorted runs are not.  Every posting of a document
//   carries the same fieldnorm code, so the racing writers of fieldnorm[doc] store the same byte; a document without a posting keeps 0.
//   Every lane of a wave takes part in every block decode (decode_doc_ids' DPP scan reads them all); ids of lanes past the block's end
//   and ids >= n_docs are not looked at.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>

#include "vbm25_internal.h"
#include "host_objects.h"
#include "decode.h"
#include "evaluate_shared.h"
#include "forward_lane.h"

// the kernels (named, so that tools/asm_lines.py finds them by their symbols)
namespace vbm25 {
namespace fwd {

using ull = unsigned long long;
constexpr uint32_t FWD_WG = 256, FWD_MAX_GRID = 2048;

struct FwdArgs {
    uint32_t n_docs, n_terms, n_blocks;
    const uint4 *blk_meta;  // (min_doc, max_doc, off8, n | meta_doc << 8 | meta_tf << 16 | ...)
    const uint8_t *blob, *post_fn;
    const uint32_t *term_first_block;  // n_terms + 1
    uint32_t *counts;                  // per document: its postings (count), its cursor (scatter)
    const ull *start;                  // n_docs + 1
    uint32_t *term, *tf;
    uint8_t *fieldnorm;
};

// the ids of block j in the lanes' postings 2 lane, 2 lane + 1, and whether each is a posting of a document of the index
__device__ __forceinline__ void fwd_block_ids(const FwdArgs &a, uint32_t j, uint32_t lane, uint4 &m, uint32_t &d0, uint32_t &d1, bool &k0, bool &k1) {
    m = a.blk_meta[j];
    const uint32_t n = m.w & 0xffu, md = (m.w >> 8) & 0xffu;
    decode_doc_ids(a.blob + 8ull * m.z, md, n, m.x, lane, d0, d1);
    k0 = 2 * lane < n && d0 < a.n_docs;
    k1 = 2 * lane + 1 < n && d1 < a.n_docs;
}

__global__ void __launch_bounds__(FWD_WG) fwd_count_kernel(FwdArgs a) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = (gridDim.x * FWD_WG) >> 6;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int((blockIdx.x * FWD_WG + threadIdx.x) >> 6)));
    for (uint32_t j = wave; j < a.n_blocks; j += n_waves) {  // (whole waves)
        uint4 m;
        uint32_t d0, d1;
        bool k0, k1;
        fwd_block_ids(a, j, lane, m, d0, d1, k0, k1);
        if (k0) atomicAdd(&a.counts[d0], 1u);
        if (k1) atomicAdd(&a.counts[d1], 1u);
    }
}

__global__ void __launch_bounds__(FWD_WG) fwd_scatter_kernel(FwdArgs a) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = (gridDim.x * FWD_WG) >> 6;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int((blockIdx.x * FWD_WG + threadIdx.x) >> 6)));
    for (uint32_t j = wave; j < a.n_blocks; j += n_waves) {
        uint4 m;
        uint32_t d0, d1;
        bool k0, k1;
        fwd_block_ids(a, j, lane, m, d0, d1, k0, k1);
        const uint32_t n = m.w & 0xffu, md = (m.w >> 8) & 0xffu, mt = (m.w >> 16) & 0xffu;
        uint32_t f0, f1;
        decode_fields(a.blob + 8ull * m.z + ((payload_bytes(md, n) + 7u) & ~7u), mt, n, lane, f0, f1);
        const uchar2 fn = reinterpret_cast<const uchar2 *>(a.post_fn + 128ull * j)[lane];
        uint32_t lo = 0, hi = a.n_terms;  // the term of block j: term_first_block[t] <= j < [t + 1]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.term_first_block[mid] <= j) lo = mid; else hi = mid;
        }
        if (k0) {
            const ull at = slot_of(a.start[d0], atomicAdd(&a.counts[d0], 1u));
            a.term[at] = lo;
            a.tf[at] = f0;
            a.fieldnorm[d0] = fn.x;
        }
        if (k1) {
            const ull at = slot_of(a.start[d1], atomicAdd(&a.counts[d1], 1u));
            a.term[at] = lo;
            a.tf[at] = f1;
            a.fieldnorm[d1] = fn.y;
        }
    }
}

// what fwd_classify_kernel counts: the documents of each class, the postings of the long runs
struct ClassCounts {
    ull n[3];
    ull long_postings;
};

struct ClassArgs {
    uint32_t n_docs, wave_max, group_max;
    const ull *start;
    ClassCounts *counts;
    uint32_t *group_doc;                         // the documents of the workgroup class, in no order
    uint32_t *long_doc, *long_begin, *long_end;  // the long runs: the document, its run's place in the fallback's buffers
};

__global__ void __launch_bounds__(FWD_WG) fwd_classify_kernel(ClassArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const ull below = (1ull << lane) - 1ull;
    for (uint32_t base = blockIdx.x * FWD_WG; base < a.n_docs; base += gridDim.x * FWD_WG) {  // (whole waves: the ballots count every lane)
        const uint32_t d = base + threadIdx.x;
        const bool mine = d < a.n_docs;
        const ull len = mine ? a.start[d + 1] - a.start[d] : 0ull;
        const uint32_t cls = mine ? run_class(len, a.wave_max, a.group_max) : 3u;
        for (uint32_t c = 0; c < 3; ++c) {
            const ull b = __ballot(cls == c);
            if (!b) continue;  // (wave-uniform)
            const uint32_t leader = uint32_t(__ffsll((long long)b)) - 1u;
            uint32_t at = 0;  // (a class holds at most n_docs documents)
            if (lane == leader) at = uint32_t(atomicAdd(&a.counts->n[c], ull(__popcll(b))));
            at = uint32_t(__shfl(int(at), int(leader)));
            const uint32_t i = at + uint32_t(__popcll(b & below));
            if (cls == c && c == RUN_GROUP) a.group_doc[i] = d;
            if (cls == c && c == RUN_LONG) {
                const ull off = atomicAdd(&a.counts->long_postings, len);  // (used only when the total is below 2^31: the host checks)
                a.long_doc[i] = d;
                a.long_begin[i] = uint32_t(off);
                a.long_end[i] = uint32_t(off + len);
            }
        }
    }
}

// one wave a document, the waves stride the documents; a run of the wave class of 2 or more postings is sorted
__global__ void __launch_bounds__(FWD_WG) fwd_sort_wave_kernel(uint32_t n_docs, uint32_t wave_max, uint32_t group_max, const ull *start, uint32_t *term,
                                                          uint32_t *tf) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = (gridDim.x * FWD_WG) >> 6;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int((blockIdx.x * FWD_WG + threadIdx.x) >> 6)));
    for (uint32_t d = wave; d < n_docs; d += n_waves) {
        const ull b = start[d], len64 = start[d + 1] - b;
        if (run_class(len64, wave_max, group_max) != RUN_WAVE || len64 < 2) continue;  // (wave-uniform)
        const uint32_t len = uint32_t(len64), p = padded_len(len);
        const bool mine = lane < len;
        uint32_t key = mine ? term[b + lane] : PAD_TERM, val = mine ? tf[b + lane] : 0u;
        for (uint32_t k = 2, j = 1; k <= p; next_step(k, j)) {
            const int from = int(cx_partner(lane, j));
            const uint32_t pkey = uint32_t(__shfl(int(key), from)), pval = uint32_t(__shfl(int(val), from));
            cx_take(lane, k, j, key, val, pkey, pval);
        }
        if (mine) {
            term[b + lane] = key;
            tf[b + lane] = val;
        }
    }
}

// one workgroup a listed document, the workgroups stride the list
__global__ void __launch_bounds__(FWD_WG) fwd_sort_group_kernel(const uint32_t *group_doc, uint32_t n_group, const ull *start, uint32_t *term, uint32_t *tf) {
    __shared__ uint32_t s_key[FWD_GROUP_MAX], s_val[FWD_GROUP_MAX];
    for (uint32_t g = blockIdx.x; g < n_group; g += gridDim.x) {
        const uint32_t d = group_doc[g];
        const ull b = start[d];
        const uint32_t len = min(uint32_t(start[d + 1] - b), FWD_GROUP_MAX), p = padded_len(len);  // (the class bound is FWD_GROUP_MAX at most)
        for (uint32_t i = threadIdx.x; i < p; i += FWD_WG) {
            s_key[i] = i < len ? term[b + i] : PAD_TERM;
            s_val[i] = i < len ? tf[b + i] : 0u;
        }
        __syncthreads();
        for (uint32_t k = 2, j = 1; k <= p; next_step(k, j)) {
            for (uint32_t t = threadIdx.x; t < (p >> 1); t += FWD_WG) {
                const uint32_t lo = pair_low(t, j), hi = lo | j;
                const uint32_t kl = s_key[lo], kh = s_key[hi];
                if (pair_swaps(kl, kh, pair_ascending(lo, k))) {
                    const uint32_t vl = s_val[lo], vh = s_val[hi];
                    s_key[lo] = kh;
                    s_key[hi] = kl;
                    s_val[lo] = vh;
                    s_val[hi] = vl;
                }
            }
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < len; i += FWD_WG) {
            term[b + i] = s_key[i];
            tf[b + i] = s_val[i];
        }
        __syncthreads();  // (the next document's load overwrites the arrays)
    }
}

// the long runs between the result arrays and the fallback's buffers: one workgroup a run, the workgroups stride the runs
__global__ void __launch_bounds__(FWD_WG) fwd_long_copy_kernel(bool gather, const uint32_t *long_doc, const uint32_t *long_begin, const uint32_t *long_end,
                                                          uint32_t n_long, const ull *start, uint32_t *term, uint32_t *tf, uint32_t *buf_term,
                                                          uint32_t *buf_tf) {
    for (uint32_t g = blockIdx.x; g < n_long; g += gridDim.x) {
        const ull b = start[long_doc[g]];
        const uint32_t at = long_begin[g], len = long_end[g] - at;
        for (uint32_t i = threadIdx.x; i < len; i += FWD_WG) {
            if (gather) {
                buf_term[at + i] = term[b + i];
                buf_tf[at + i] = tf[b + i];
            } else {
                term[b + i] = buf_term[at + i];
                tf[b + i] = buf_tf[at + i];
            }
        }
    }
}
}  // namespace fwd
}  // namespace vbm25

namespace {

using namespace vbm25;
using namespace vbm25::fwd;

// fwd_grid (the most workgroups of any kernel of this file, 0 = no cap beyond FWD_MAX_GRID), fwd_wave_max and fwd_group_max of
// vbm25_tuning_set: read at the start of each bind
std::atomic<uint32_t> g_fwd_grid{0}, g_wave_max{FWD_WAVE_MAX}, g_group_max{FWD_GROUP_MAX};
// the calling thread's last bind: its kernels by HIP events (allocations and the read-back excluded), the documents of each class
thread_local double g_fwd_ms = -1.0;
thread_local ull g_fwd_class[3] = {0, 0, 0};

uint32_t capped_grid(uint64_t units, uint32_t per_block, uint32_t cap) {
    return std::min(grid_for(units, per_block, FWD_MAX_GRID), cap ? cap : FWD_MAX_GRID);
}

int use_forward_device(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: vbm25_index_bind builds the forward index on the device and has no host fallback");
    return use_device(device);
}

int index_bind(const vbm25_index *ix, vbm25_doc_terms **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ix) return set_error(VBM25_ERR_INVALID, "NULL argument");
    int n_dev = 0;  // (before the index is looked at: without a device there is no index)
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return use_forward_device(0);
    if (int rc = use_forward_device(ix->device)) return rc;
    g_fwd_ms = -1.0;
    g_fwd_class[0] = g_fwd_class[1] = g_fwd_class[2] = 0;
    const uint32_t cap = g_fwd_grid.load(), wave_max = g_wave_max.load(), group_max = g_group_max.load();
    const uint32_t n_docs = ix->n_docs, n_blocks = ix->n_blocks;
    auto t = std::make_unique<vbm25_doc_terms>();
    t->index = ix;
    t->device = ix->device;
    t->n_docs = t->base_docs = n_docs;
    t->from_index = true;
    HbmArray counts, cub, cls, group_doc, long_doc, long_begin, long_end, buf_term, buf_tf, buf_term2, buf_tf2, seg_cub;
    Event ev_start, ev_mid, ev_resume, ev_done;
    Stream st;  // (of the call's own: a launch on the null stream would wait for every other stream of the device)
    HIP_TRY(st.create());
    Quiesce quiesce(st.s);
    for (Event *e : {&ev_start, &ev_mid, &ev_resume, &ev_done}) HIP_TRY(e->create());
    size_t cub_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(nullptr, WidenU32()),
                                            (ull *)nullptr, int(n_docs + 1), st.s));
    HIP_TRY(counts.alloc(4ull * (n_docs + 1ull)));
    HIP_TRY(cub.alloc(cub_bytes));
    HIP_TRY(cls.alloc(sizeof(ClassCounts)));
    HIP_TRY(group_doc.alloc(4ull * n_docs));
    HIP_TRY(long_doc.alloc(4ull * n_docs));
    HIP_TRY(long_begin.alloc(4ull * n_docs));
    HIP_TRY(long_end.alloc(4ull * n_docs));
    HIP_TRY(t->d_start.alloc(8ull * (n_docs + 1ull)));
    HIP_TRY(t->d_fieldnorm.alloc(n_docs));
    FwdArgs a{};
    a.n_docs = n_docs;
    a.n_terms = ix->n_terms;
    a.n_blocks = n_blocks;
    a.blk_meta = ix->blk_meta.as<uint4>();
    a.blob = ix->blob.as<uint8_t>();
    a.post_fn = ix->post_fn.as<uint8_t>();
    a.term_first_block = ix->term_first_block.as<uint32_t>();
    a.counts = counts.as<uint32_t>();
    a.start = t->d_start.as<ull>();
    a.fieldnorm = t->d_fieldnorm.as<uint8_t>();
    const uint32_t block_grid = capped_grid(n_blocks, FWD_WG / 64, cap);
    HIP_TRY(hipEventRecord(ev_start.e, st.s));
    HIP_TRY(hipMemsetAsync(counts.p, 0, 4ull * (n_docs + 1ull), st.s));
    HIP_TRY(hipMemsetAsync(cls.p, 0, sizeof(ClassCounts), st.s));
    if (n_docs) HIP_TRY(hipMemsetAsync(t->d_fieldnorm.p, 0, n_docs, st.s));
    if (n_blocks && n_docs) {
        fwd_count_kernel<<<block_grid, FWD_WG, 0, st.s>>>(a);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub.p, cub_bytes, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(counts.as<uint32_t>(), WidenU32()),
                                            t->d_start.as<ull>(), int(n_docs + 1), st.s));
    if (n_docs) {
        const ClassArgs ca{n_docs, wave_max, group_max, a.start, cls.as<ClassCounts>(), group_doc.as<uint32_t>(), long_doc.as<uint32_t>(),
                           long_begin.as<uint32_t>(), long_end.as<uint32_t>()};
        fwd_classify_kernel<<<capped_grid(n_docs, FWD_WG, cap), FWD_WG, 0, st.s>>>(ca);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(counts.p, 0, 4ull * (n_docs + 1ull), st.s));  // the counters become the cursors
    }
    HIP_TRY(hipEventRecord(ev_mid.e, st.s));
    // the one read-back: the posting total sizes the result, the long runs size the fallback's buffers
    ull n_known = 0;
    ClassCounts cc{};
    HIP_TRY(hipMemcpyAsync(&n_known, t->d_start.as<ull>() + n_docs, 8, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipMemcpyAsync(&cc, cls.p, sizeof cc, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    if (cc.long_postings >= (1ull << 31))
        return set_error(VBM25_ERR_UNSUPPORTED, "%llu postings in documents of more than %u: the long runs of one bind hold fewer than 2^31",
                         cc.long_postings, group_max);
    t->n_known = n_known;
    HIP_TRY(t->d_term.alloc(4ull * n_known));
    HIP_TRY(t->d_tf.alloc(4ull * n_known));
    a.term = t->d_term.as<uint32_t>();
    a.tf = t->d_tf.as<uint32_t>();
    const uint32_t n_group = uint32_t(cc.n[RUN_GROUP]), n_long = uint32_t(cc.n[RUN_LONG]), n_long_post = uint32_t(cc.long_postings);
    size_t seg_bytes = 0;
    if (n_long) {
        for (HbmArray *b : {&buf_term, &buf_tf, &buf_term2, &buf_tf2}) HIP_TRY(b->alloc(4ull * n_long_post));
        HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, seg_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                                           (uint32_t *)nullptr, int(n_long_post), int(n_long), (const uint32_t *)nullptr,
                                                           (const uint32_t *)nullptr, 0, 32, st.s));
        HIP_TRY(seg_cub.alloc(seg_bytes));
    }
    HIP_TRY(hipEventRecord(ev_resume.e, st.s));
    if (n_known) {
        fwd_scatter_kernel<<<block_grid, FWD_WG, 0, st.s>>>(a);
        HIP_TRY(hipGetLastError());
        if (cc.n[RUN_WAVE]) {
            fwd_sort_wave_kernel<<<capped_grid(n_docs, FWD_WG / 64, cap), FWD_WG, 0, st.s>>>(n_docs, wave_max, group_max, a.start, a.term, a.tf);
            HIP_TRY(hipGetLastError());
        }
        if (n_group) {
            fwd_sort_group_kernel<<<capped_grid(n_group, 1, cap), FWD_WG, 0, st.s>>>(group_doc.as<uint32_t>(), n_group, a.start, a.term, a.tf);
            HIP_TRY(hipGetLastError());
        }
        if (n_long) {
            const uint32_t grid = capped_grid(n_long, 1, cap);
            fwd_long_copy_kernel<<<grid, FWD_WG, 0, st.s>>>(true, long_doc.as<uint32_t>(), long_begin.as<uint32_t>(), long_end.as<uint32_t>(), n_long, a.start,
                                                      a.term, a.tf, buf_term.as<uint32_t>(), buf_tf.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(seg_cub.p, seg_bytes, buf_term.as<uint32_t>(), buf_term2.as<uint32_t>(), buf_tf.as<uint32_t>(),
                                                               buf_tf2.as<uint32_t>(), int(n_long_post), int(n_long), long_begin.as<uint32_t>(),
                                                               long_end.as<uint32_t>(), 0, 32, st.s));
            fwd_long_copy_kernel<<<grid, FWD_WG, 0, st.s>>>(false, long_doc.as<uint32_t>(), long_begin.as<uint32_t>(), long_end.as<uint32_t>(), n_long, a.start,
                                                      a.term, a.tf, buf_term2.as<uint32_t>(), buf_tf2.as<uint32_t>());
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(ev_done.e, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    float ms = 0, ms2 = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev_start.e, ev_mid.e));
    HIP_TRY(hipEventElapsedTime(&ms2, ev_resume.e, ev_done.e));
    g_fwd_ms = double(ms) + ms2;
    for (uint32_t c = 0; c < 3; ++c) g_fwd_class[c] = cc.n[c];
    *out = t.release();
    return VBM25_OK;
}

}  // namespace

namespace vbm25 {
int forward_tuning_set(const char *name, long long value) {
    const std::string n(name);
    if (n == "fwd_grid") {
        if (value < 0 || value > (long long)FWD_MAX_GRID) return set_error(VBM25_ERR_INVALID, "%s %lld is outside 0 .. %u", name, value, FWD_MAX_GRID);
        g_fwd_grid.store(uint32_t(value));
        return VBM25_OK;
    }
    std::atomic<uint32_t> &slot = n == "fwd_wave_max" ? g_wave_max : g_group_max;
    const uint32_t bound = n == "fwd_wave_max" ? FWD_WAVE_MAX : FWD_GROUP_MAX;
    if (value < 0 || value > (long long)bound) return set_error(VBM25_ERR_INVALID, "%s %lld is outside 0 .. %u", name, value, bound);
    slot.store(uint32_t(value));
    return VBM25_OK;
}
void forward_tuning_reset() {
    g_fwd_grid.store(0);
    g_wave_max.store(FWD_WAVE_MAX);
    g_group_max.store(FWD_GROUP_MAX);
}
}  // namespace vbm25

extern "C" {

int vbm25_index_bind(const vbm25_index *ix, vbm25_doc_terms **out) {
    return guarded([&] { return index_bind(ix, out); });
}

// tools/forward_cost.py and the tests of the classes: the device time of the calling thread's last vbm25_index_bind's kernels by HIP
// events (allocations and the read-back excluded; -1 when it enqueued nothing) and how many documents took the wave class, the
// workgroup class and the segmented radix sort.  Not in the header.
int vbm25_debug_forward(double *kernel_ms, uint64_t *n_wave, uint64_t *n_group, uint64_t *n_long) {
    if (!kernel_ms || !n_wave || !n_group || !n_long) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *kernel_ms = g_fwd_ms;
    *n_wave = g_fwd_class[RUN_WAVE];
    *n_group = g_fwd_class[RUN_GROUP];
    *n_long = g_fwd_class[RUN_LONG];
    return VBM25_OK;
}

// the tests of the bind: a handle's fieldnorm codes (vbm25_doc_terms_download has the other three arrays) and whether it came from
// an index.  Not in the header.
int vbm25_debug_doc_terms_fieldnorm(const vbm25_doc_terms *t, uint8_t *fieldnorm, uint32_t *from_index) {
    if (!t || !fieldnorm || !from_index) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = use_forward_device(t->device)) return rc;
    if (t->n_docs) HIP_TRY(hipMemcpy(fieldnorm, t->d_fieldnorm.p, t->n_docs, hipMemcpyDeviceToHost));
    *from_index = t->from_index ? 1u : 0u;
    return VBM25_OK;
}

}  // extern "C"
