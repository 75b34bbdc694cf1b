// live.hip -- the rerank stack follows a live table: a bound handle (vbm25_doc_terms) grows in place from a delta of cast documents,
// and a reranker's ctid directory takes the new rows by a merge on the device (vbm25_reranker_sync in reranker.hip, with the kernels
// of this file through live_shared.h).
//
//   the append (vbm25_doc_terms_append_documents; vbm25_doc_terms_append stages a host CSR and takes the same path): the bind of the
//   delta written behind the handle's documents, on a stream of the call's own.
//     bind_lookup_kernel, bind_count_kernel, (scan), bind_compact_kernel   evaluate.hip's, through evaluate_shared.h: the scan's sums
//                          are the delta's own, and the runs are compacted to term / tf at the old n_known
//     live_start_kernel    start[n_docs + i + 1] = the delta's sum i + 1, rebased by the old n_known
//     the fieldnorm codes and the payloads are device-to-device copies behind the handle's
//   Lookup, count and scan read the delta and write the call's scratch; the read-back of the delta's known elements sizes the arrays.
//   Everything is allocated then, and only then the call waits for the device and writes -- behind the documents every consumer reads,
//   or into larger arrays that are swapped in at the end.  A capacity at least doubles (vbm25_documents_extend's factor), and a growth
//   step copies device to device.
//
//   the directory's kernels:
//     live_sort_kernel     a delta of <= 4096 rows: one workgroup, the rows' words (tid_lane.h: key above position) in LDS, a
//                          bitonic network over them
//     live_merge_kernel    one lane an entry of the old directory or of the delta: its place in the merged arrays by rank.  The old
//                          directory's evenly spaced keys staged in LDS once per workgroup, as cand_lookup_kernel stages them.
//
//   the deletes (vbm25_doc_terms_delete, vbm25_doc_terms_delete_tids): a bitmap of one bit a document on the handle, made by the first
//   delete that names a document; rerank_part_kernel and cand_lookup_kernel leave a dead document out.  Checks and allocations, the
//   wait for the device, then one kernel on the null stream and the count read back -- the append's contract.
//     live_dead_docs_kernel   one lane a document index: atomicOr of its bit, the new bits counted from the word the atomic returns
//     live_dead_tids_kernel   tid_match_kernel's OR_COUNT mode over a grown handle: wave w answers word w, each lane's ctid from the
//                             base plane or the handle's tail, tid_contains with the set's directory in LDS, one ballot a word
//   An append carries the bitmap along (append_core's parts): capacity for the fieldnorm array's, new words zero.
//   No kernel here has scratch memory.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "evaluate_shared.h"
#include "live_shared.h"
#include "tid_lane.h"

namespace {

using namespace vbm25;
using namespace vbm25::evl;
using namespace vbm25::tid;
using ull = unsigned long long;

constexpr uint32_t WG = 256, MAX_GRID = 2048;

std::atomic<uint32_t> g_live_sort_max{live::LIVE_SORT_CAP};
// the calling thread's last append: its kernels and device-to-device copies by HIP events (allocations, the read-back and the wait for
// the device excluded; -1 when it enqueued nothing)
thread_local double g_append_ms = -1.0;

__global__ void __launch_bounds__(WG) live_start_kernel(const ull *delta_start, uint32_t n, ull base, ull *start_at) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) start_at[i + 1] = delta_start[i + 1] + base;
}

__global__ void __launch_bounds__(WG) live_sort_kernel(const uint16_t *payload, uint32_t m, uint32_t padded, uint32_t first_doc, ull *keys, uint32_t *docs) {
    extern __shared__ ull s_word[];
    for (uint32_t j = threadIdx.x; j < padded; j += WG) {
        uint64_t w = LIVE_SORT_PAD;
        if (j < m) {
            const uint16_t *p = payload + 3ull * j;
            const uint16_t p3[3] = {p[0], p[1], p[2]};
            w = live_sort_word(tid_key(p3), j);
        }
        s_word[j] = w;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= padded; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (padded >> 1); t += WG) live_sort_step((uint64_t *)s_word, t, k, j);
            __syncthreads();
        }
    for (uint32_t j = threadIdx.x; j < m; j += WG) {
        keys[j] = live_sort_key(s_word[j]);
        docs[j] = first_doc + live_sort_row(s_word[j]);
    }
}

__global__ void __launch_bounds__(WG) live_merge_kernel(live::MergeArgs a) {
    extern __shared__ ull s_dir[];
    for (uint32_t i = threadIdx.x; i < a.n_dir; i += WG) s_dir[i] = a.dir[i];
    __syncthreads();
    const ull n = a.n_old + a.n_delta;
    for (ull i = ull(blockIdx.x) * WG + threadIdx.x; i < n; i += ull(gridDim.x) * WG) {
        if (i < a.n_delta) {
            const ull key = a.delta_keys[i];
            const ull at = i + live_rank_delta(key, (const uint64_t *)s_dir, a.n_dir, (const uint64_t *)a.keys, a.n_old, a.stride);
            a.out_keys[at] = key;
            a.out_docs[at] = a.delta_docs[i];
        } else {
            const ull o = i - a.n_delta, key = a.keys[o];
            const ull at = o + live_rank_old(key, (const uint64_t *)a.delta_keys, a.n_delta);
            a.out_keys[at] = key;
            a.out_docs[at] = a.docs[o];
        }
    }
}

// ---- the deletion bitmap ----
constexpr uint32_t WAVES = WG / 64;
// the bitmap's words for n documents, in bytes
uint64_t dead_bytes(uint64_t n) { return 8 * ((n + 63) / 64); }

// docs: n document indices below the handle's n_docs, repeats allowed.  One lane an index: the bit ORed into its word, and the word
// the atomic returns says whether this lane was the one that set it -- a repeat within the call counts once.
__global__ void __launch_bounds__(WG) live_dead_docs_kernel(const uint32_t *docs, ull n, ull *words, uint32_t *count) {
    uint32_t counted = 0;
    for (ull i = ull(blockIdx.x) * WG + threadIdx.x; i < n; i += ull(gridDim.x) * WG) {
        const uint32_t d = docs[i];
        const ull bit = 1ull << (d & 63u);
        if (!(atomicOr(&words[d >> 6], bit) & bit)) ++counted;
    }
    if (counted) atomicAdd(count, counted);
}

struct DeadTidArgs {
    const uint16_t *base, *tail;  // the ctids of documents 0 .. base_docs, and of base_docs .. n
    uint32_t base_docs, n;
    const ull *dir, *keys;  // the set
    uint64_t n_keys;
    uint32_t n_dir, stride;
    ull *words;  // ceil(n / 64): the handle's bitmap
    uint32_t *count;
};

// tid_match_kernel (tid.hip) over a grown handle, in its OR_COUNT mode: wave w answers word w, each lane with its document's ctid
// from the base plane or the tail (the split falls inside a word whenever base_docs % 64 != 0), one ballot a word, and lane 0 ORs
// the word in and counts the bits that were not set.  No word has two writers: the waves take distinct words.
__global__ void __launch_bounds__(WG) live_dead_tids_kernel(DeadTidArgs a) {
    extern __shared__ ull s_set_dir[];
    for (uint32_t i = threadIdx.x; i < a.n_dir; i += WG) s_set_dir[i] = a.dir[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, n_words = uint32_t((uint64_t(a.n) + 63u) >> 6);
    uint32_t counted = 0;
    for (uint64_t w = uint64_t(blockIdx.x) * WAVES + (threadIdx.x >> 6); w < n_words; w += uint64_t(gridDim.x) * WAVES) {
        const uint64_t d = (w << 6) + lane;
        bool hit = false;
        if (d < a.n) {
            const uint16_t *p = split_payload(a.base, a.tail, a.base_docs, d);
            const uint16_t p3[3] = {p[0], p[1], p[2]};
            hit = tid_contains(tid_key(p3), (const uint64_t *)s_set_dir, a.n_dir, (const uint64_t *)a.keys, a.n_keys, a.stride);
        }
        const uint64_t word = match_word(__ballot(hit), w << 6, a.n, 0);
        if (lane == 0) {
            const uint64_t old = a.words[w];
            counted += new_bits(old, word);
            if (word & ~old) a.words[w] = old | word;
        }
    }
    if (lane == 0 && counted) atomicAdd(a.count, counted);
}

// What both deletes share.  `bitmap`: the handle's, or -- a handle nobody deleted from -- one made for this call, all zero, words for
// the fieldnorm array's capacity; it becomes the handle's only when the call set a bit.
struct DeadTarget {
    HbmArray fresh, count;
    ull *words = nullptr;
};
int dead_prepare(const vbm25_doc_terms *t, DeadTarget *dt) {
    HIP_TRY(dt->count.alloc(4));
    if (t->d_dead.p) {
        dt->words = t->d_dead.as<ull>();
        return VBM25_OK;
    }
    HIP_TRY(dt->fresh.alloc(dead_bytes(std::max<uint64_t>(t->d_fieldnorm.bytes, t->n_docs))));
    dt->words = dt->fresh.as<ull>();
    return VBM25_OK;
}
// behind the kernel: the count read back, the new bitmap kept if it holds a bit
int dead_finish(vbm25_doc_terms *t, DeadTarget *dt, uint32_t *n_new) {
    uint32_t fresh = 0;
    HIP_TRY(hipMemcpy(&fresh, dt->count.p, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    if (dt->fresh.p && fresh) {
        std::swap(t->d_dead.p, dt->fresh.p);
        std::swap(t->d_dead.bytes, dt->fresh.bytes);
    }
    t->n_dead += fresh;
    if (n_new) *n_new = fresh;
    return VBM25_OK;
}

int delete_docs(vbm25_doc_terms *t, const uint32_t *docs, uint64_t n, uint32_t *n_new) {
    if (!t || (n && !docs)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_new) *n_new = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (docs[i] >= t->n_docs)
            return set_error(VBM25_ERR_INVALID, "docs[%llu] is %u: outside the handle's %u documents", (ull)i, docs[i], t->n_docs);
    if (!n) return VBM25_OK;
    if (int rc = use_eval_device(t->device)) return rc;
    // every allocation and the upload first; then the wait for the device, and only then the words change
    DeadTarget dt;
    HbmArray d_docs;
    HIP_TRY(d_docs.alloc(4 * n));
    if (int rc = dead_prepare(t, &dt)) return rc;
    HIP_TRY(hipMemcpy(d_docs.p, docs, 4 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    if (dt.fresh.p) HIP_TRY(hipMemsetAsync(dt.fresh.p, 0, dt.fresh.bytes));
    HIP_TRY(hipMemsetAsync(dt.count.p, 0, 4));
    live_dead_docs_kernel<<<grid_for(n, WG, std::min(MAX_GRID, std::max(1u, eval_grid_cap()))), WG>>>(d_docs.as<uint32_t>(), n, dt.words,
                                                                                                     dt.count.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    return dead_finish(t, &dt, n_new);
}

int delete_tids(vbm25_doc_terms *t, const vbm25_tid_set *s, const vbm25_documents *payloads, uint32_t *n_new) {
    if (!t || !s) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_new) *n_new = 0;
    TidSetView v;
    tid_set_view(s, &v);
    if (v.device != t->device) return set_error(VBM25_ERR_INVALID, "the TID set is on device %d, the bound documents on device %d", v.device, t->device);
    const uint32_t n_tail = t->n_docs - t->base_docs;
    const uint16_t *base = nullptr;
    if (t->from_index) {
        if (payloads) return set_error(VBM25_ERR_INVALID, "payloads are given and the handle is bound to an index: its ctids are the index's own");
        uint32_t n = 0;
        if (int rc = index_payloads(t->index, &base, &n)) return rc;
        if (n != t->base_docs) return set_error(VBM25_ERR_INVALID, "the index has %u documents, the handle was bound with %u", n, t->base_docs);
    } else if (payloads) {  // vbm25_reranker_create's checks of the same handle
        if (!payloads->has_payload) return set_error(VBM25_ERR_INVALID, "the documents given for the ctid lookup carry no payloads");
        if (payloads->n_docs != t->base_docs)
            return set_error(VBM25_ERR_INVALID, "the documents given for the ctid lookup are %u, the bound documents %u", payloads->n_docs, t->base_docs);
        if (payloads->device != t->device)
            return set_error(VBM25_ERR_INVALID, "the documents given for the ctid lookup are on device %d, the bound documents on device %d",
                             payloads->device, t->device);
        base = payloads->d_payload.as<uint16_t>();
    } else if (t->base_docs) {
        return set_error(VBM25_ERR_INVALID, "payloads is NULL: the %u documents the handle was bound with have their ctids in the vbm25_documents", t->base_docs);
    }
    if (n_tail && !t->tail_payload)
        return set_error(VBM25_ERR_INVALID, "the %u documents appended to the bound documents carry no payloads: no ctid names them", n_tail);
    if (!t->n_docs || !v.n_keys) return VBM25_OK;
    if (int rc = use_eval_device(t->device)) return rc;
    DeadTarget dt;
    if (int rc = dead_prepare(t, &dt)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (dt.fresh.p) HIP_TRY(hipMemsetAsync(dt.fresh.p, 0, dt.fresh.bytes));
    HIP_TRY(hipMemsetAsync(dt.count.p, 0, 4));
    const DeadTidArgs a{base, t->d_tail_payload.as<uint16_t>(), t->base_docs, t->n_docs, v.dir, v.keys, v.n_keys, v.n_dir, v.stride, dt.words,
                        dt.count.as<uint32_t>()};
    const uint32_t n_words = uint32_t((uint64_t(t->n_docs) + 63u) / 64u);
    live_dead_tids_kernel<<<grid_for(n_words, WAVES, tid_grid_now()), WG, 8ull * std::max(1u, v.n_dir)>>>(a);
    HIP_TRY(hipGetLastError());
    return dead_finish(t, &dt, n_new);
}

int read_dead(const vbm25_doc_terms *t, uint64_t *words) {
    if (!t || (t->n_docs && !words)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    const uint64_t bytes = dead_bytes(t->n_docs);
    if (!bytes) return VBM25_OK;
    if (!t->d_dead.p) {
        std::memset(words, 0, bytes);
        return VBM25_OK;
    }
    if (int rc = use_eval_device(t->device)) return rc;
    HIP_TRY(hipMemcpy(words, t->d_dead.p, bytes, hipMemcpyDeviceToHost));
    return VBM25_OK;
}

// a delta's arrays in HBM on the handle's device (a cast's, or the staged CSR's); payload NULL: none
struct Delta {
    uint32_t n_docs;
    uint64_t n_elements;
    const ull *start;
    const void *key;
    const uint32_t *tf;
    const uint8_t *fieldnorm;
    const uint16_t *payload;
};

// the checks that read neither the delta's arrays nor the device: both appends make them, in this order, before anything else
int append_checks(const vbm25_doc_terms *t, const vbm25_resolver *rs, int delta_device, bool has_payload, uint64_t n_docs, uint64_t n_elements,
                  ResolverVocabulary *v) {
    if (int rc = resolver_vocabulary(rs, v)) return rc;
    if (delta_device != t->device)
        return set_error(VBM25_ERR_INVALID, "the delta is on device %d, the bound documents on device %d", delta_device, t->device);
    if (v->device != t->device)
        return set_error(VBM25_ERR_INVALID, "the bound documents are on device %d, the resolver's index is on device %d", t->device, v->device);
    if (v->index != t->index) return set_error(VBM25_ERR_INVALID, "the documents are bound to another index than the resolver's");
    if (t->from_index && !has_payload)
        return set_error(VBM25_ERR_INVALID, "the delta carries no payloads: documents appended to an index-bound handle need their ctids");
    if (t->tail_decided && t->tail_payload != has_payload)
        return set_error(VBM25_ERR_INVALID, "the delta %s payloads and the documents appended so far %s", has_payload ? "carries" : "carries no",
                         t->tail_payload ? "carry them" : "carry none");
    // a document index is 32 bits and 0xFFFFFFFF names no document (rerank_shared.h: NO_DOC); a run's bounds are read as 32 bits
    // (eval_score_kernel, rerank_part_kernel)
    if (uint64_t(t->n_docs) + n_docs >= 0xFFFFFFFFull)
        return set_error(VBM25_ERR_UNSUPPORTED, "%llu documents: a bound handle takes fewer than 2^32 - 1", (ull)(uint64_t(t->n_docs) + n_docs));
    if (t->n_known + n_elements >= (1ull << 32))
        return set_error(VBM25_ERR_UNSUPPORTED, "%llu known elements at the most: a bound handle takes fewer than 2^32", (ull)(t->n_known + n_elements));
    return VBM25_OK;
}

int append_core(vbm25_doc_terms *t, const Delta &d, const ResolverVocabulary &v) {
    const uint32_t n = d.n_docs, n_el = uint32_t(d.n_elements), n0 = t->n_docs;  // (fewer than 2^31 elements: a cast, or the CSR's check)
    const bool has_payload = d.payload != nullptr;
    g_append_ms = -1.0;
    if (!n) return VBM25_OK;
    if (int rc = use_eval_device(t->device)) return rc;
    HbmArray ids, counts, sums, cub, grown[6];
    Event ev_start, ev_mid, ev_resume, ev_done;
    Stream st;  // (of the call's own, as the bind's)
    HIP_TRY(st.create());
    Quiesce quiesce(st.s);
    for (Event *e : {&ev_start, &ev_mid, &ev_resume, &ev_done}) HIP_TRY(e->create());
    size_t cub_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(nullptr, WidenU32()),
                                            (ull *)nullptr, int(n + 1), st.s));
    HIP_TRY(ids.alloc(4ull * n_el));
    HIP_TRY(counts.alloc(4ull * (n + 1ull)));
    HIP_TRY(sums.alloc(8ull * (n + 1ull)));
    HIP_TRY(cub.alloc(cub_bytes));
    // the delta's bind as far as its sums: reads the delta and the vocabulary, writes the call's scratch
    HIP_TRY(hipEventRecord(ev_start.e, st.s));
    HIP_TRY(hipMemsetAsync(counts.p, 0, 4ull * (n + 1ull), st.s));
    if (n_el) {
        HIP_TRY(launch_bind_lookup(d.key, n_el, v.keys, v.n_terms, ids.as<uint32_t>(), st.s));
        HIP_TRY(launch_bind_count(ids.as<uint32_t>(), d.start, n, counts.as<uint32_t>(), st.s));
    }
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub.p, cub_bytes, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(counts.as<uint32_t>(), WidenU32()),
                                            sums.as<ull>(), int(n + 1), st.s));
    HIP_TRY(hipEventRecord(ev_mid.e, st.s));
    ull n_new = 0;
    HIP_TRY(hipMemcpyAsync(&n_new, sums.as<ull>() + n, 8, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    const uint64_t nd = uint64_t(n0) + n, nk = t->n_known + n_new, n_tail = nd - t->base_docs;
    // per array: (the array, the bytes in use, the bytes needed).  Every larger array first: a failure so far leaves the handle as it
    // was.  Capacities at least double, so appending n deltas copies O(n) bytes.
    struct Part {
        HbmArray *a;
        uint64_t used, need;
    } parts[6] = {{&t->d_start, 8ull * (n0 + 1ull), 8 * (nd + 1)},
                  {&t->d_term, 4 * t->n_known, 4 * nk},
                  {&t->d_tf, 4 * t->n_known, 4 * nk},
                  {&t->d_fieldnorm, n0, nd},
                  {&t->d_tail_payload, 6ull * (n0 - t->base_docs), 6 * n_tail},
                  {&t->d_dead, dead_bytes(n0), 0}};
    constexpr int FIELDNORM = 3, DEAD = 5, n_swap = 6;
    const int n_parts = has_payload ? 5 : 4;
    for (int i = 0; i < n_parts; ++i)
        if (parts[i].need > parts[i].a->bytes || !parts[i].a->p) HIP_TRY(grown[i].alloc(std::max<uint64_t>(parts[i].need, 2 * uint64_t(parts[i].a->bytes))));
    // a handle somebody deleted from: the bitmap's capacity follows the fieldnorm array's (a handle without a bitmap stays without)
    if (t->d_dead.p) {
        parts[DEAD].need = dead_bytes(grown[FIELDNORM].p ? grown[FIELDNORM].bytes : t->d_fieldnorm.bytes);
        if (parts[DEAD].need > t->d_dead.bytes) HIP_TRY(grown[DEAD].alloc(parts[DEAD].need));
    }
    // from here on the handle's arrays are written or replaced: whatever was enqueued before the call ends on the old ones
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipEventRecord(ev_resume.e, st.s));
    // (a larger bitmap: new words zero -- the appended documents are live -- and the old words copied in front of them)
    if (grown[DEAD].p) HIP_TRY(hipMemsetAsync(grown[DEAD].p, 0, grown[DEAD].bytes, st.s));
    for (int i = 0; i < n_swap; ++i)
        if (grown[i].p && parts[i].used) HIP_TRY(hipMemcpyAsync(grown[i].p, parts[i].a->p, parts[i].used, hipMemcpyDeviceToDevice, st.s));
    auto now = [&](int i) { return static_cast<uint8_t *>(grown[i].p ? grown[i].p : parts[i].a->p); };
    ull *start = reinterpret_cast<ull *>(now(0));
    if (n_new)
        HIP_TRY(launch_bind_compact(ids.as<uint32_t>(), d.tf, d.start, sums.as<ull>(), n, reinterpret_cast<uint32_t *>(now(1)) + t->n_known,
                                    reinterpret_cast<uint32_t *>(now(2)) + t->n_known, st.s));
    live_start_kernel<<<grid_for(n, WG, std::min(MAX_GRID, std::max(1u, eval_grid_cap()))), WG, 0, st.s>>>(sums.as<ull>(), n, t->n_known, start + n0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(now(3) + n0, d.fieldnorm, n, hipMemcpyDeviceToDevice, st.s));
    if (has_payload) HIP_TRY(hipMemcpyAsync(now(4) + 6ull * (n0 - t->base_docs), d.payload, 6ull * n, hipMemcpyDeviceToDevice, st.s));
    HIP_TRY(hipEventRecord(ev_done.e, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    float ms = 0, ms2 = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev_start.e, ev_mid.e));
    HIP_TRY(hipEventElapsedTime(&ms2, ev_resume.e, ev_done.e));
    g_append_ms = double(ms) + ms2;
    for (int i = 0; i < n_swap; ++i)
        if (grown[i].p) {
            std::swap(grown[i].p, parts[i].a->p);  // (the old array goes with `grown`)
            std::swap(grown[i].bytes, parts[i].a->bytes);
        }
    t->n_docs = uint32_t(nd);
    t->n_known = nk;
    t->tail_decided = true;
    t->tail_payload = has_payload;
    return VBM25_OK;
}

int append_documents(vbm25_doc_terms *t, const vbm25_documents *h, const vbm25_resolver *rs) {
    if (!t || !h || !rs) return set_error(VBM25_ERR_INVALID, "NULL argument");
    ResolverVocabulary v;
    if (h->caster && h->in_flight)
        // (all that can be told from the pointer: after that batch's collect it names the new documents, a valid delta)
        return set_error(VBM25_ERR_INVALID, "the delta belongs to a caster slot that was submitted again: its arrays are being rewritten");
    if (int rc = append_checks(t, rs, h->device, h->has_payload, h->n_docs, h->n_elements, &v)) return rc;
    const Delta d{h->n_docs, h->n_elements, h->d_start.as<ull>(), h->d_key.p, h->d_tf.as<uint32_t>(), h->d_fieldnorm.as<uint8_t>(),
                  h->has_payload ? h->d_payload.as<uint16_t>() : nullptr};
    return append_core(t, d, v);
}

// the host CSR: upload's validation, then the arrays staged once -- a deleted document with an empty run, its elements left out
int append_csr(vbm25_doc_terms *t, const vbm25_growing_desc *g, const vbm25_resolver *rs) {
    if (!t || !g || !rs) return set_error(VBM25_ERR_INVALID, "NULL argument");
    const uint32_t n = g->n_docs;
    if (n && (!g->start || !g->fieldnorm)) return set_error(VBM25_ERR_INVALID, "growing arrays missing");
    for (uint32_t i = 0; i < n; ++i)
        if (g->start[i + 1] < g->start[i]) return set_error(VBM25_ERR_INVALID, "start not monotone at document %u", i);
    const uint64_t e_first = n ? g->start[0] : 0, e_end = n ? g->start[n] : 0;
    if (e_end > g->n_elements)
        return set_error(VBM25_ERR_INVALID, "start reaches element %llu of %llu", (ull)e_end, (ull)g->n_elements);
    if (e_end - e_first && (!g->key || !g->tf)) return set_error(VBM25_ERR_INVALID, "growing arrays missing");
    if (e_end - e_first >= (1ull << 31))
        return set_error(VBM25_ERR_UNSUPPORTED, "%llu elements in one delta: an append takes fewer than 2^31", (ull)(e_end - e_first));
    for (uint32_t i = 0; i < n; ++i)  // Document::checked_new, vector.rs:56-61
        for (uint64_t e = g->start[i] + 1; e < g->start[i + 1]; ++e)
            if (std::memcmp(g->key + 16ull * (e - 1), g->key + 16ull * e, 16) >= 0)
                return set_error(VBM25_ERR_INVALID, "growing document %u: keys must be strictly ascending", i);
    std::vector<uint64_t> start(size_t(n) + 1, 0);
    for (uint32_t i = 0; i < n; ++i) start[i + 1] = start[i] + (g->deleted && g->deleted[i] ? 0 : g->start[i + 1] - g->start[i]);
    const uint64_t n_el = start[n];
    ResolverVocabulary v;
    if (int rc = append_checks(t, rs, t->device, g->payload != nullptr, n, n_el, &v)) return rc;
    if (!n) return VBM25_OK;
    if (int rc = use_eval_device(t->device)) return rc;
    HbmArray d_start, d_key, d_tf, d_fn, d_pay;
    HIP_TRY(d_start.alloc(8ull * (n + 1ull)));
    HIP_TRY(d_key.alloc(16 * n_el));
    HIP_TRY(d_tf.alloc(4 * n_el));
    HIP_TRY(d_fn.alloc(n));
    if (g->payload) HIP_TRY(d_pay.alloc(6ull * n));
    HIP_TRY(hipMemcpy(d_start.p, start.data(), 8ull * (n + 1ull), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_fn.p, g->fieldnorm, n, hipMemcpyHostToDevice));
    if (g->payload) HIP_TRY(hipMemcpy(d_pay.p, g->payload, 6ull * n, hipMemcpyHostToDevice));
    // the live documents' elements, in runs of neighbours: without a deleted document one copy an array
    for (uint32_t i = 0; i < n;) {
        if (g->deleted && g->deleted[i]) {
            ++i;
            continue;
        }
        uint32_t j = i + 1;
        while (j < n && !(g->deleted && g->deleted[j])) ++j;
        const uint64_t from = g->start[i], len = g->start[j] - from;
        if (len) {
            HIP_TRY(hipMemcpy(d_key.as<uint8_t>() + 16 * start[i], g->key + 16 * from, 16 * len, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_tf.as<uint32_t>() + start[i], g->tf + from, 4 * len, hipMemcpyHostToDevice));
        }
        i = j;
    }
    const Delta d{n, n_el, d_start.as<ull>(), d_key.p, d_tf.as<uint32_t>(), d_fn.as<uint8_t>(), g->payload ? d_pay.as<uint16_t>() : nullptr};
    return append_core(t, d, v);
}

}  // namespace

namespace vbm25 {
namespace live {

uint32_t live_sort_max_now() { return g_live_sort_max.load(); }

hipError_t launch_live_sort(const uint16_t *payload, uint32_t m, uint32_t first_doc, ull *keys, uint32_t *docs, hipStream_t stream) {
    uint32_t padded = 1;
    while (padded < m) padded <<= 1;
    live_sort_kernel<<<1, WG, 8ull * padded, stream>>>(payload, m, padded, first_doc, keys, docs);
    return hipGetLastError();
}

hipError_t launch_live_merge(const MergeArgs &a, hipStream_t stream) {
    const uint32_t cap = std::min(MAX_GRID, std::max(1u, eval_grid_cap()));
    live_merge_kernel<<<grid_for(a.n_old + a.n_delta, WG, cap), WG, 8ull * std::max(1u, a.n_dir), stream>>>(a);
    return hipGetLastError();
}

}  // namespace live

int live_tuning_set(long long value) {
    if (value < 0 || value > (long long)live::LIVE_SORT_CAP)
        return set_error(VBM25_ERR_INVALID, "live_sort_max %lld is outside 0 .. %u", value, live::LIVE_SORT_CAP);
    g_live_sort_max.store(uint32_t(value));
    return VBM25_OK;
}
void live_tuning_reset() { g_live_sort_max.store(live::LIVE_SORT_CAP); }

}  // namespace vbm25

extern "C" {

int vbm25_doc_terms_append_documents(vbm25_doc_terms *t, const vbm25_documents *delta, const vbm25_resolver *r) {
    return guarded([&] { return append_documents(t, delta, r); });
}

int vbm25_doc_terms_append(vbm25_doc_terms *t, const vbm25_growing_desc *delta, const vbm25_resolver *r) {
    return guarded([&] { return append_csr(t, delta, r); });
}

uint32_t vbm25_doc_terms_base_docs(const vbm25_doc_terms *t) { return t ? t->base_docs : 0; }

int vbm25_doc_terms_delete(vbm25_doc_terms *t, const uint32_t *docs, uint64_t n, uint32_t *n_new) {
    return guarded([&] { return delete_docs(t, docs, n, n_new); });
}

int vbm25_doc_terms_delete_tids(vbm25_doc_terms *t, const vbm25_tid_set *s, const vbm25_documents *payloads, uint32_t *n_new) {
    return guarded([&] { return delete_tids(t, s, payloads, n_new); });
}

uint32_t vbm25_doc_terms_dead_docs(const vbm25_doc_terms *t) { return t ? t->n_dead : 0; }

int vbm25_doc_terms_read_dead(const vbm25_doc_terms *t, uint64_t *words) {
    return guarded([&] { return read_dead(t, words); });
}

// tools/live_rerank_cost.py: the device time of the calling thread's last append's kernels and copies, by HIP events.  Not in the header.
int vbm25_debug_append_kernel_ms(double *ms) {
    if (!ms) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *ms = g_append_ms;
    return VBM25_OK;
}

}  // extern "C"
