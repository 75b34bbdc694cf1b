// evaluate.hip -- the `<&>` operator from cast documents: bm25::evaluate (evaluate.rs:22-74; src/index/operators.rs:22-55) for batches
// of queries, each against its own list of candidate documents, everything read from HBM.  evaluate_lane.h holds the per-lane functions;
// the scoring kernel here is a loop over them.
//
//   the bind (vbm25_documents_bind): a vbm25_documents handle's keys -> term ids of ONE index's vocabulary, which the resolver of that
//   index already keeps in HBM.  On a stream of the call's own:
//     bind_lookup_kernel   one lane an element: lookup_lane (resolve_lane.h) of its key -> id or NOT_FOUND
//     bind_count_kernel    one wave a document: its known elements, by ballot -> counts[doc]
//     (scan)               exclusive sum of the counts in 64 bits -> start
//     bind_compact_kernel  one wave a document: (id, tf) of the known elements to start[doc] .., in element order
//   Keys and the vocabulary both ascend in key_order, so a document's run of ids ascends strictly.  The fieldnorm codes are copied
//   from the cast: elements the vocabulary lacks count for the length.
//
//   the score (vbm25_evaluate_documents): a work item is (query, 64 of its candidates), one wave an item, the waves stride the items.
//     eval_score_kernel    the item's query by bisection of item_start (the host's scan of the candidate counts).  Each lane owns a
//                          candidate: its run's bounds, its fieldnorm's s1.  The query's (id, idf) pairs are read 64 at a time, one
//                          a lane, and handed to all lanes through v_readlane -- wave-uniform, in registers, whatever the query's
//                          length; then score_step per term in query order.  A lane without a candidate has an empty run and reads
//                          nothing (evaluate_lane.h: a position is read only inside a non-empty range).
//   No kernel here has scratch memory or LDS.
//   The argument checks of a scoring call, the kernel's arguments and its launch are declared in evaluate_shared.h: the scorer handle
//   of rerank.hip makes the same checks and launches the same kernel.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "resolve_lane.h"
#include "evaluate_lane.h"
#include "evaluate_shared.h"

namespace {

using namespace vbm25;
using namespace vbm25::rsv;
using namespace vbm25::evl;
using ull = unsigned long long;

constexpr uint32_t WG = 256, MAX_GRID = 2048;

// eval_grid of vbm25_tuning_set: the most workgroups any kernel of this file is launched with; read at the start of each call
std::atomic<uint32_t> g_eval_grid{MAX_GRID};
// the calling thread's last bind / last score: the kernels by HIP events (uploads, downloads and allocations excluded)
thread_local double g_bind_ms = -1.0, g_score_ms = -1.0;

uint32_t capped_grid(uint64_t units, uint32_t per_block, uint32_t cap) { return std::min(grid_for(units, per_block, MAX_GRID), std::max(1u, cap)); }

__global__ void __launch_bounds__(WG) bind_lookup_kernel(const Key *key, uint32_t n, const Key *vocab, uint32_t n_terms, uint32_t *ids) {
    for (uint32_t e = blockIdx.x * WG + threadIdx.x; e < n; e += gridDim.x * WG) ids[e] = lookup_lane(vocab, n_terms, key[e]);
}

__global__ void __launch_bounds__(WG) bind_count_kernel(const uint32_t *ids, const ull *doc_start, uint32_t n_docs, uint32_t *counts) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG + threadIdx.x) >> 6, n_waves = (gridDim.x * WG) >> 6;
    for (uint32_t d = wave; d < n_docs; d += n_waves) {
        const uint32_t b = uint32_t(doc_start[d]), n = uint32_t(doc_start[d + 1]) - b;
        uint32_t known = 0;
        for (uint32_t j = 0; j < n; j += 64) {
            const bool k = j + lane < n && ids[b + j + lane] != NOT_FOUND;
            known += uint32_t(__popcll(__ballot(k)));
        }
        if (lane == 0) counts[d] = known;
    }
}

__global__ void __launch_bounds__(WG) bind_compact_kernel(const uint32_t *ids, const uint32_t *tf, const ull *doc_start, const ull *start,
                                                         uint32_t n_docs, uint32_t *out_term, uint32_t *out_tf) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG + threadIdx.x) >> 6, n_waves = (gridDim.x * WG) >> 6;
    for (uint32_t d = wave; d < n_docs; d += n_waves) {
        const uint32_t b = uint32_t(doc_start[d]), n = uint32_t(doc_start[d + 1]) - b;
        ull at = start[d];
        for (uint32_t j = 0; j < n; j += 64) {
            const bool mine = j + lane < n;
            const uint32_t id = mine ? ids[b + j + lane] : NOT_FOUND;
            const ull known = __ballot(id != NOT_FOUND);
            if (id != NOT_FOUND) {
                const ull o = at + uint32_t(__popcll(known & ((1ull << lane) - 1ull)));
                out_term[o] = id;
                out_tf[o] = tf[b + j + lane];
            }
            at += uint32_t(__popcll(known));
        }
    }
}

__global__ void __launch_bounds__(WG) eval_score_kernel(ScoreArgs a) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = (gridDim.x * WG) >> 6;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int((blockIdx.x * WG + threadIdx.x) >> 6)));
    for (uint32_t item = wave; item < a.n_items; item += n_waves) {
        uint32_t ql = 0, qh = a.nq;  // the last query with item_start[q] <= item (queries without candidates in front of it share its start)
        while (qh - ql > 1) {
            const uint32_t mid = ql + ((qh - ql) >> 1);
            if (a.item_start[mid] <= item) ql = mid; else qh = mid;
        }
        const uint32_t q = uint32_t(__builtin_amdgcn_readfirstlane(int(ql)));
        const ull cand0 = a.q_cand ? a.q_cand[q] : ull(q) * a.cross_docs;
        const uint32_t n_cand = a.q_cand ? uint32_t(a.q_cand[q + 1] - cand0) : a.cross_docs;
        const uint32_t c = (item - a.item_start[q]) * 64u + lane;
        const bool mine = c < n_cand;
        // a lane without a candidate: the empty run 0 .. 0, which score_step never reads
        uint32_t cursor = 0, hi = 0;
        double s1 = 1.0;
        if (mine) {
            const uint32_t d = a.cand_doc ? a.cand_doc[cand0 + c] : c;
            cursor = uint32_t(a.start[d]);
            hi = uint32_t(a.start[d + 1]);
            s1 = a.s1[a.fieldnorm[d]];
        }
        const uint32_t qb = a.q_off[q], qn = a.q_off[q + 1] - qb;
        double result = 0.0;
        for (uint32_t t0 = 0; t0 < qn; t0 += 64) {
            const uint32_t chunk = qn - t0 < 64u ? qn - t0 : 64u;
            const uint32_t my_id = lane < chunk ? a.q_ids[qb + t0 + lane] : NOT_FOUND;
            const double my_idf = my_id < a.n_terms ? a.term_idf[my_id] : 0.0;
            for (uint32_t j = 0; j < chunk; ++j) {
                const uint32_t id = uint32_t(__builtin_amdgcn_readlane(int(my_id), int(j)));
                if (id >= a.n_terms) continue;
                score_step(a.term, a.tf, cursor, hi, id, lane_double(my_idf, j), a.k1p1, s1, result);
            }
        }
        if (mine) a.scores[cand0 + c] = result;
    }
}

int documents_bind(const vbm25_documents *h, const vbm25_resolver *r, vbm25_doc_terms **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h || !r) return set_error(VBM25_ERR_INVALID, "NULL argument");
    ResolverVocabulary v;
    if (int rc = resolver_vocabulary(r, &v)) return rc;
    if (v.device != h->device)
        return set_error(VBM25_ERR_INVALID, "the documents are on device %d, the resolver's index is on device %d", h->device, v.device);
    if (int rc = use_eval_device(h->device)) return rc;
    g_bind_ms = -1.0;
    const uint32_t n_docs = h->n_docs, n_el = uint32_t(h->n_elements);  // (fewer than 2^31: a cast takes no more)
    auto t = std::make_unique<vbm25_doc_terms>();
    t->index = v.index;
    t->device = h->device;
    t->n_docs = t->base_docs = n_docs;
    HbmArray ids, counts, cub;
    Event ev_start, ev_mid, ev_resume, ev_done;
    Stream st;  // (of the call's own: a launch on the null stream would wait for every other stream of the device)
    HIP_TRY(st.create());
    Quiesce quiesce(st.s);
    for (Event *e : {&ev_start, &ev_mid, &ev_resume, &ev_done}) HIP_TRY(e->create());
    size_t cub_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(nullptr, WidenU32()),
                                            (ull *)nullptr, int(n_docs + 1), st.s));
    HIP_TRY(ids.alloc(4ull * n_el));
    HIP_TRY(counts.alloc(4ull * (n_docs + 1ull)));
    HIP_TRY(cub.alloc(cub_bytes));
    HIP_TRY(t->d_start.alloc(8ull * (n_docs + 1ull)));
    HIP_TRY(t->d_fieldnorm.alloc(n_docs));
    HIP_TRY(hipEventRecord(ev_start.e, st.s));
    HIP_TRY(hipMemsetAsync(counts.p, 0, 4ull * (n_docs + 1ull), st.s));
    if (n_docs) HIP_TRY(hipMemcpyAsync(t->d_fieldnorm.p, h->d_fieldnorm.p, n_docs, hipMemcpyDeviceToDevice, st.s));
    const ull *doc_start = h->d_start.as<ull>();
    if (n_el) {
        HIP_TRY(launch_bind_lookup(h->d_key.p, n_el, v.keys, v.n_terms, ids.as<uint32_t>(), st.s));
        HIP_TRY(launch_bind_count(ids.as<uint32_t>(), doc_start, n_docs, counts.as<uint32_t>(), st.s));
    }
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub.p, cub_bytes, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(counts.as<uint32_t>(), WidenU32()),
                                            t->d_start.as<ull>(), int(n_docs + 1), st.s));
    HIP_TRY(hipEventRecord(ev_mid.e, st.s));
    ull n_known = 0;
    HIP_TRY(hipMemcpyAsync(&n_known, t->d_start.as<ull>() + n_docs, 8, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    t->n_known = n_known;
    HIP_TRY(t->d_term.alloc(4ull * n_known));
    HIP_TRY(t->d_tf.alloc(4ull * n_known));
    HIP_TRY(hipEventRecord(ev_resume.e, st.s));
    if (n_known) {
        HIP_TRY(launch_bind_compact(ids.as<uint32_t>(), h->d_tf.as<uint32_t>(), doc_start, t->d_start.as<ull>(), n_docs, t->d_term.as<uint32_t>(),
                                    t->d_tf.as<uint32_t>(), st.s));
    }
    HIP_TRY(hipEventRecord(ev_done.e, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    float ms = 0, ms2 = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev_start.e, ev_mid.e));
    HIP_TRY(hipEventElapsedTime(&ms2, ev_resume.e, ev_done.e));
    g_bind_ms = double(ms) + ms2;
    *out = t.release();
    return VBM25_OK;
}

int doc_terms_download(const vbm25_doc_terms *t, uint64_t *start, uint32_t *term, uint32_t *tf) {
    if (!t || !start || (t->n_known && (!term || !tf))) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = use_eval_device(t->device)) return rc;
    HIP_TRY(hipMemcpy(start, t->d_start.p, 8ull * (t->n_docs + 1ull), hipMemcpyDeviceToHost));
    if (t->n_known) {
        HIP_TRY(hipMemcpy(term, t->d_term.p, 4ull * t->n_known, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(tf, t->d_tf.p, 4ull * t->n_known, hipMemcpyDeviceToHost));
    }
    return VBM25_OK;
}

int evaluate_documents(const vbm25_doc_terms *t, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                       const uint32_t *cand_doc, double *scores) {
    EvaluateTables ix;
    uint64_t n_pairs = 0;
    if (int rc = check_score_call(t, term_ids, q_off, nq, q_cand, cand_doc, scores, &ix, &n_pairs)) return rc;
    if (n_pairs == 0) return VBM25_OK;
    // the items: a scan of the candidate counts, 64 candidates an item
    std::vector<uint32_t> item_start(size_t(nq) + 1, 0);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t n = q_cand ? q_cand[q + 1] - q_cand[q] : t->n_docs;
        item_start[q + 1] = item_start[q] + uint32_t((n + 63) / 64);
    }
    const uint32_t n_items = item_start[nq], n_ids = q_off[nq];
    if (int rc = use_eval_device(t->device)) return rc;
    g_score_ms = -1.0;
    HbmArray d_ids, d_off, d_cand, d_doc, d_items, d_scores;
    Event ev_start, ev_done;
    Stream st;  // (of the call's own, as the bind's)
    HIP_TRY(st.create());
    Quiesce quiesce(st.s);
    HIP_TRY(ev_start.create());
    HIP_TRY(ev_done.create());
    HIP_TRY(d_ids.alloc(4ull * n_ids));
    HIP_TRY(d_off.alloc(4ull * (nq + 1ull)));
    HIP_TRY(d_items.alloc(4ull * (nq + 1ull)));
    HIP_TRY(d_scores.alloc(8ull * n_pairs));
    if (n_ids) HIP_TRY(hipMemcpyAsync(d_ids.p, term_ids, 4ull * n_ids, hipMemcpyHostToDevice, st.s));
    HIP_TRY(hipMemcpyAsync(d_off.p, q_off, 4ull * (nq + 1ull), hipMemcpyHostToDevice, st.s));
    HIP_TRY(hipMemcpyAsync(d_items.p, item_start.data(), 4ull * (nq + 1ull), hipMemcpyHostToDevice, st.s));
    if (q_cand) {
        HIP_TRY(d_cand.alloc(8ull * (nq + 1ull)));
        HIP_TRY(d_doc.alloc(4ull * n_pairs));
        HIP_TRY(hipMemcpyAsync(d_cand.p, q_cand, 8ull * (nq + 1ull), hipMemcpyHostToDevice, st.s));
        HIP_TRY(hipMemcpyAsync(d_doc.p, cand_doc, 4ull * n_pairs, hipMemcpyHostToDevice, st.s));
    }
    ScoreArgs a{};
    fill_score_tables(t, ix, &a);
    a.q_ids = d_ids.as<uint32_t>();
    a.q_off = d_off.as<uint32_t>();
    a.q_cand = q_cand ? d_cand.as<ull>() : nullptr;
    a.cand_doc = q_cand ? d_doc.as<uint32_t>() : nullptr;
    a.cross_docs = q_cand ? 0u : t->n_docs;
    a.item_start = d_items.as<uint32_t>();
    a.nq = nq;
    a.n_items = n_items;
    a.scores = d_scores.as<double>();
    HIP_TRY(hipEventRecord(ev_start.e, st.s));
    HIP_TRY(launch_eval_score(a, st.s));
    HIP_TRY(hipEventRecord(ev_done.e, st.s));
    HIP_TRY(hipMemcpyAsync(scores, d_scores.p, 8ull * n_pairs, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev_start.e, ev_done.e));
    g_score_ms = ms;
    return VBM25_OK;
}

}  // namespace

namespace vbm25 {
namespace evl {

int use_eval_device(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: the evaluate operator on bound documents has no host fallback (vbm25_evaluate is the host function)");
    return use_device(device);
}

int check_score_call(const vbm25_doc_terms *t, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                     const uint32_t *cand_doc, const void *out, EvaluateTables *ixp, uint64_t *n_pairs_out, bool docs_later) {
    *n_pairs_out = 0;
    if (!t) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (nq == 0) return VBM25_OK;
    if (!term_ids || !q_off || !out) return set_error(VBM25_ERR_INVALID, "NULL argument");
    EvaluateTables &ix = *ixp;
    if (int rc = index_evaluate_tables(t->index, &ix)) return rc;
    if (q_off[0] != 0) return set_error(VBM25_ERR_INVALID, "q_off[0] is %u, not 0", q_off[0]);
    for (uint32_t q = 0; q < nq; ++q)
        if (q_off[q + 1] < q_off[q]) return set_error(VBM25_ERR_INVALID, "q_off is not monotone at query %u", q);
    if (q_cand) {
        if (!cand_doc && !docs_later) return set_error(VBM25_ERR_INVALID, "cand_doc is NULL while q_cand is not");
        if (q_cand[0] != 0) return set_error(VBM25_ERR_INVALID, "q_cand[0] is %llu, not 0", (ull)q_cand[0]);
        for (uint32_t q = 0; q < nq; ++q)
            if (q_cand[q + 1] < q_cand[q]) return set_error(VBM25_ERR_INVALID, "q_cand is not monotone at query %u", q);
    }
    const uint64_t n_pairs = q_cand ? q_cand[nq] : uint64_t(nq) * t->n_docs;
    if (n_pairs >= (1ull << 31)) return set_error(VBM25_ERR_UNSUPPORTED, "%llu pairs: one call scores fewer than 2^31", (ull)n_pairs);
    for (uint32_t q = 0; q < nq; ++q) {  // Query::checked_new, vector.rs:106-110, as vbm25_evaluate_batch checks it: known ids against the last known one
        bool have = false;
        uint32_t prev = 0;
        for (uint32_t i = q_off[q]; i < q_off[q + 1]; ++i) {
            if (term_ids[i] >= ix.n_terms) continue;
            if (have && term_ids[i] <= prev) return set_error(VBM25_ERR_INVALID, "query %u: term ids must be strictly ascending", q);
            prev = term_ids[i];
            have = true;
        }
    }
    if (q_cand && !docs_later)
        for (uint32_t q = 0; q < nq; ++q)
            for (uint64_t i = q_cand[q]; i < q_cand[q + 1]; ++i)
                if (cand_doc[i] >= t->n_docs)
                    return set_error(VBM25_ERR_INVALID, "query %u: candidate %u is outside the handle's %u documents", q, cand_doc[i], t->n_docs);
    if (ix.n_docs == 0) return set_error(VBM25_ERR_INVALID, "evaluate on an index without sealed documents");
    *n_pairs_out = n_pairs;
    return VBM25_OK;
}

void fill_score_tables(const vbm25_doc_terms *t, const EvaluateTables &ix, ScoreArgs *a) {
    a->start = t->d_start.as<ull>();
    a->term = t->d_term.as<uint32_t>();
    a->tf = t->d_tf.as<uint32_t>();
    a->fieldnorm = t->d_fieldnorm.as<uint8_t>();
    a->term_idf = ix.term_idf;
    a->s1 = ix.s1;
    a->k1p1 = ix.k1 + 1.0;
    a->n_terms = ix.n_terms;
}

hipError_t launch_eval_score(const ScoreArgs &a, hipStream_t stream) {
    eval_score_kernel<<<capped_grid(a.n_items, WG / 64, g_eval_grid.load()), WG, 0, stream>>>(a);
    return hipGetLastError();
}

uint32_t eval_grid_cap() { return g_eval_grid.load(); }

hipError_t launch_bind_lookup(const void *keys, uint32_t n_el, const void *vocab, uint32_t n_terms, uint32_t *ids, hipStream_t stream) {
    bind_lookup_kernel<<<capped_grid(n_el, WG, g_eval_grid.load()), WG, 0, stream>>>(static_cast<const Key *>(keys), n_el, static_cast<const Key *>(vocab),
                                                                                     n_terms, ids);
    return hipGetLastError();
}

hipError_t launch_bind_count(const uint32_t *ids, const ull *doc_start, uint32_t n_docs, uint32_t *counts, hipStream_t stream) {
    bind_count_kernel<<<capped_grid(n_docs, WG / 64, g_eval_grid.load()), WG, 0, stream>>>(ids, doc_start, n_docs, counts);
    return hipGetLastError();
}

hipError_t launch_bind_compact(const uint32_t *ids, const uint32_t *tf, const ull *doc_start, const ull *start, uint32_t n_docs, uint32_t *out_term,
                               uint32_t *out_tf, hipStream_t stream) {
    bind_compact_kernel<<<capped_grid(n_docs, WG / 64, g_eval_grid.load()), WG, 0, stream>>>(ids, tf, doc_start, start, n_docs, out_term, out_tf);
    return hipGetLastError();
}

}  // namespace evl
}  // namespace vbm25

namespace vbm25 {
int evaluate_tuning_set(long long value) {
    g_eval_grid.store(uint32_t(std::min<long long>(std::max(1ll, value), MAX_GRID)));
    return VBM25_OK;
}
void evaluate_tuning_reset() { g_eval_grid.store(MAX_GRID); }
}  // namespace vbm25

extern "C" {

int vbm25_documents_bind(const vbm25_documents *h, const vbm25_resolver *r, vbm25_doc_terms **out) {
    return guarded([&] { return documents_bind(h, r, out); });
}

int vbm25_doc_terms_info(const vbm25_doc_terms *t, uint32_t *n_docs, uint64_t *n_known, int *device) {
    if (!t) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_docs) *n_docs = t->n_docs;
    if (n_known) *n_known = t->n_known;
    if (device) *device = t->device;
    return VBM25_OK;
}

int vbm25_doc_terms_download(const vbm25_doc_terms *t, uint64_t *start, uint32_t *term, uint32_t *tf) {
    return guarded([&] { return doc_terms_download(t, start, term, tf); });
}

uint64_t vbm25_doc_terms_device_bytes(const vbm25_doc_terms *t) {
    uint64_t n = 0;
    if (t)
        for (const HbmArray *a : {&t->d_start, &t->d_term, &t->d_tf, &t->d_fieldnorm, &t->d_tail_payload, &t->d_dead})
            n += a->bytes;  // (the room to spare included; the deletion bitmap from the first delete that names a document)
    return n;
}

void vbm25_doc_terms_free(vbm25_doc_terms *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

int vbm25_evaluate_documents(const vbm25_doc_terms *t, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                             const uint32_t *cand_doc, double *scores) {
    return guarded([&] { return evaluate_documents(t, term_ids, q_off, nq, q_cand, cand_doc, scores); });
}

// tools/evaluate_cost.py: the device time of the calling thread's last bind's kernels and of its last scoring kernel, by HIP events.
// Not in the header.
int vbm25_debug_evaluate_kernel_ms(double *bind_ms, double *score_ms) {
    if (!bind_ms || !score_ms) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *bind_ms = g_bind_ms;
    *score_ms = g_score_ms;
    return VBM25_OK;
}

}  // extern "C"
