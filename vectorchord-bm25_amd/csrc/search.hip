// search.hip -- device half of libvbm25: batched BM25 top-k over compressed posting blocks for MI355X
// (gfx950, wave64).  Replaces the traversal of crates/bm25/src/search.rs:28-282 of the reference
// (bm25::search) for the sealed segment.  The batch's unit; the kernels live in headers:
//   plan.h         plan_kernel (queries -> doc-range work items)
//   scan_win.h     scan_win_kernel (its own translation unit, scan_win.hip): sparse queries of <= 8 terms of comparable length, k <= 256
//                  (k <= 64 beyond five terms) -- the document-window formulation, the dominant kernel of C3
//   scan_range.h   scan_range_kernel: every other sparse query of <= 16 terms, k <= 256; the one-launch route of vbm25_search_batch (C2)
//   scan_dense.h   scan_dense_kernel: queries with many postings per document (Zipf head terms; C5), <= 16 terms, k <= 256
//   scan_many.h    scan_many_kernel: up to 1024 terms, 256 < k <= 1024, items the others gave up (exhaustive)
//   merge.h        merge_kernel: per-item top-k lists -> hits with payloads
//   decode.h / block_fetch.h / topk_lds.h / topk_reg.h / device_types.h   shared pieces
// This file: vbm25_batch and nothing else -- create, routing, set_queries, the run_* routes, the growing segment's part of a run, fetch,
// the one-shot vbm25_search_batch* entry points, the tuning switches, the debug and timing entry points.  The other handles have
// units of their own over host_objects.h.  DESIGN.md has the full story.
//
// Result order is canonical: score descending, ties by ascending doc id.  All f64 arithmetic is IEEE
// (compiled with -ffp-contract=off, no fast-math): results are bit-identical to the CPU oracle's
// brute-force evaluation.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "vbm25_internal.h"
#include "host_objects.h"
#include "decode.h"
#include "plan.h"
#include "topk_lds.h"
#include "block_fetch.h"
#include "topk_reg.h"
#include "decode_id16.h"
#include "scan_range.h"
#include "scan_win_launch.h"
#include "scan_dense.h"
#include "scan_many.h"
#include "merge.h"
#include "growing.h"

namespace vbm25 {

// ---------------------------------------------------------------------------
// k > 1024 (bm25.limit goes up to 65535, gucs.rs:37-46): exhaustive path, one query at a time.  acc[d] is the
// score of document d: one launch per term in ascending key order adds that term's postings (a document has
// at most one posting per term, so the adds of a launch never collide and the sum order is the key order of
// evaluate.rs:43-72).  Positive doubles order like their bit patterns (crates/score/src/lib.rs:46-60), so a
// stable descending radix sort of (bits(acc[d]), d) over all documents gives score descending, ties by
// ascending id; the first k entries with a non-zero key are the result (Results, search.rs:284-314).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bigk_accum_kernel(DevIndex ix, uint32_t term, double *acc) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t j0 = ix.term_first_block[term], j1 = ix.term_first_block[term + 1];
    const double s0 = ix.term_s0[term];
    for (uint32_t j = j0 + blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); j < j1; j += gridDim.x * (blockDim.x / 64)) {
        const uint4 bm = ix.blk_meta[j];
        const uint32_t n = bm.w & 0xff, md = (bm.w >> 8) & 0xff, mt = (bm.w >> 16) & 0xff;
        const uint8_t *body = ix.blob + 8ull * bm.z;
        uint32_t d0, d1, f0, f1;
        decode_doc_ids(body, md, n, bm.x, lane, d0, d1);
        decode_fields(body + ((payload_bytes(md, n) + 7u) & ~7u), mt, n, lane, f0, f1);
        const uchar2 fn = reinterpret_cast<const uchar2 *>(ix.post_fn + 128ull * j)[lane];
        if (2 * lane < n) {
            const double tf = (double)f0;
            acc[d0] = acc[d0] + (tf * s0) / (tf + ix.s1[fn.x]);  // Cache::evaluate, bm25.rs:355-358
        }
        if (2 * lane + 1 < n) {
            const double tf = (double)f1;
            acc[d1] = acc[d1] + (tf * s0) / (tf + ix.s1[fn.y]);
        }
    }
}
// filtered search: the score of every rejected document is wiped before the sort -- a key of 0 is no hit (not emitted, not counted)
__global__ void __launch_bounds__(256) bigk_mask_kernel(const unsigned long long *words, uint32_t n_docs, double *acc) {
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += gridDim.x * blockDim.x)
        if (!((words[d >> 6] >> (d & 63u)) & 1ull)) acc[d] = 0.0;
}
__global__ void __launch_bounds__(256) bigk_iota_kernel(uint32_t *v, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = i;
}
__global__ void __launch_bounds__(256) bigk_emit_kernel(DevIndex ix, const unsigned long long *keys, const uint32_t *docs,
                                                        uint32_t n_docs, uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && (n_docs == 0 || keys[0] == 0)) *n_hits = 0;
    if (i >= k || i >= n_docs) return;
    const unsigned long long key = keys[i];
    if (key == 0) return;
    const uint32_t d = docs[i];
    const uint16_t *pl = ix.doc_payload + 3ull * d;
    unsigned long long *out = reinterpret_cast<unsigned long long *>(hits + i);
    out[0] = key;
    out[1] = (unsigned long long)d | (unsigned long long)pl[0] << 32 | (unsigned long long)pl[1] << 48;
    out[2] = (unsigned long long)pl[2];
    if (i + 1 == k || i + 1 == n_docs || keys[i + 1] == 0) *n_hits = i + 1;
}

// The process-wide tuning switches: this unit owns them and their lock (vbm25_tuning_set / _reset, in the extern "C" block, write them)
static Tuning g_tune;
static std::mutex g_tune_mutex;  // (set / reset / the copy a new batch takes)
Tuning tuning_snapshot() {
    std::lock_guard<std::mutex> g(g_tune_mutex);
    return g_tune;
}

namespace {

template <class F>
int dispatch_k(uint32_t k, F &&f) {
    if (k <= 64) return f(std::integral_constant<int, 64>());
    if (k <= 128) return f(std::integral_constant<int, 128>());
    if (k <= 256) return f(std::integral_constant<int, 256>());
    return f(std::integral_constant<int, 1024>());
}

}  // namespace

static int vbm25_batch_create_impl(vbm25_index *ix, uint32_t max_queries, uint32_t max_total_terms, uint32_t k,
                       vbm25_batch **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ix) return set_error(VBM25_ERR_INVALID, "index is NULL");
    if (k == 0) return set_error(VBM25_ERR_INVALID, "number of needed rows is set to 0");  // default.rs:114-116
    if (k > 65535) return set_error(VBM25_ERR_INVALID, "k exceeds bm25.limit's maximum of 65535");
    if (!max_queries) return set_error(VBM25_ERR_INVALID, "max_queries is 0");
    if (int rc = use_device(ix->device)) return rc;
    auto bt = std::make_unique<vbm25_batch>();
    bt->index = ix;
    bt->device = ix->device;
    bt->max_queries = max_queries;
    bt->max_terms = max_total_terms;
    bt->k = k;
    bt->tune = tuning_snapshot();
    bt->h_dense.resize(max_queries);
    bt->h_postings.resize(max_queries);
    // Routing by k: k <= 256 -- sparse queries of <= 16 terms: scan_range_kernel, dense ones: scan_dense_kernel, the rest and
    // whatever those two give up: scan_many_kernel; 256 < k <= 1024: scan_many_kernel (LDS top-k); above: the exhaustive path
    bt->use_range = k <= (uint32_t)REG_K;
    bt->lpi = bt->use_range ? (uint32_t)RNW : 1u;
    // (scan_dense_kernel reads post_rel16 unconditionally: an index made without the plane sends its dense queries to scan_many_kernel)
    bt->use_dense = bt->use_range && k <= (uint32_t)D_KMAX && bt->tune.dense != 0 && ix->post_rel16.p != nullptr;
    bt->target_items = bt->use_range ? std::max(256u, bt->tune.range_items) : TARGET_ITEMS;
    bt->min_chunk = bt->use_range ? std::max(128u, bt->tune.range_min_chunk) : MIN_CHUNK_POSTINGS;
    bt->max_items = max_queries + bt->target_items + (bt->use_dense ? std::max(256u, bt->tune.dense_items) : 0u);
    // scan_win_kernel's items are one wave's work each (a few per query): room for them
    if (bt->use_range && k <= scan_win_max_k(1) && bt->tune.win && !ix->term_win_host.empty())
        bt->max_items = std::max(bt->max_items, std::max(8192u, 8u * max_queries));
    int rc = 0;
    if (k > 1024) {  // exhaustive path: query buffers, results and an accumulator per document
        bt->bigk = true;
        bt->use_range = bt->use_dense = false;
        const size_t n = ix->n_docs ? ix->n_docs : 1;
        (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, bt->bk_tmp_bytes, (const unsigned long long *)nullptr,
                                                     (unsigned long long *)nullptr, (const uint32_t *)nullptr,
                                                     (uint32_t *)nullptr, (int)n);
        if ((rc = bt->hits.alloc(sizeof(vbm25_hit) * size_t(max_queries) * k)) || (rc = bt->n_hits.alloc(4ull * max_queries)) ||
            (rc = bt->error_flag.alloc(4)) || (rc = bt->bk_acc.alloc(8 * n)) || (rc = bt->bk_keys.alloc(8 * n)) ||
            (rc = bt->bk_iota.alloc(4 * n)) || (rc = bt->bk_docs.alloc(4 * n)) || (rc = bt->bk_tmp.alloc(bt->bk_tmp_bytes)))
            return rc;
        HIP_TRY(hipMemset(bt->error_flag.p, 0, 4));
        bigk_iota_kernel<<<1024, 256>>>(bt->bk_iota.as<uint32_t>(), (uint32_t)n);
        HIP_TRY(hipGetLastError());
        *out = bt.release();
        return VBM25_OK;
    }
    if ((rc = bt->term_ids.alloc(4ull * max_total_terms)) ||
        (rc = bt->q_off.alloc(4ull * (max_queries + 1))) ||
        (rc = bt->items.alloc(sizeof(Item) * size_t(bt->max_items))) || (rc = bt->n_items.alloc(4)) ||
        (rc = bt->q_item_base.alloc(4ull * (max_queries + 1))) ||
        (rc = bt->theta.alloc(8ull * max_queries)) ||
        (rc = bt->res_score.alloc(8ull * bt->max_items * bt->lpi * k)) ||
        (rc = bt->res_doc.alloc(4ull * bt->max_items * bt->lpi * k)) ||
        (rc = bt->res_cnt.alloc(4ull * bt->max_items * bt->lpi)) ||
        (rc = bt->hits.alloc(sizeof(vbm25_hit) * size_t(max_queries) * k)) ||
        (rc = bt->n_hits.alloc(4ull * max_queries)) || (rc = bt->error_flag.alloc(4)) ||
        (rc = bt->q_dense.alloc(max_queries)) ||
        (rc = bt->qin.alloc(8ull * max_total_terms + 4ull * (max_queries + 1) + max_queries + 8 + 4ull * bt->max_items + 4ull * max_queries + 64)) ||
        (rc = bt->id16_fb.alloc(4ull * max_total_terms)) ||
        (rc = bt->item_failed.alloc(4ull * bt->max_items)) || (rc = bt->item_order.alloc(4ull * bt->max_items)) || (rc = bt->work_ctr.alloc(8)) ||
        (rc = bt->hist.alloc(4ull * CUR_HB * max_queries)) || (rc = bt->fused_state.alloc(4ull * (max_queries + 1))) ||
        (rc = bt->fail_any.alloc(4)) || (rc = bt->q_failed.alloc(4ull * max_queries)) || (rc = bt->theta_last.alloc(8ull * max_queries)))
        return rc;
    HIP_TRY(hipMemset(bt->fail_any.p, 0, 4));
    HIP_TRY(hipMemset(bt->q_failed.p, 0, 4ull * max_queries));
    HIP_TRY(hipMemset(bt->error_flag.p, 0, 4));
    // The per-launch state starts zero and every route that sets state_clean leaves ALL of it zero -- whichever route runs
    // next (the plan-free route never touches fused_state: a one-launch run after it found the allocator's leftovers there
    // and no workgroup took itself for a query's last one).
    HIP_TRY(hipMemset(bt->fused_state.p, 0, 4ull * (max_queries + 1)));
    HIP_TRY(hipMemset(bt->work_ctr.p, 0, 8));
    HIP_TRY(hipMemset(bt->theta.p, 0, 8ull * max_queries));
    HIP_TRY(hipMemset(bt->theta_last.p, 0, 8ull * max_queries));
    HIP_TRY(hipMemset(bt->hist.p, 0, 4ull * CUR_HB * max_queries));
    HIP_TRY(hipMemset(bt->item_failed.p, 0, 4ull * bt->max_items));
    HIP_TRY(hipMemset(bt->res_cnt.p, 0, 4ull * bt->max_items * bt->lpi));
    if (int rc2 = bt->dbg.alloc(64)) return rc2;
    HIP_TRY(hipMemset(bt->dbg.p, 0, 64));
#ifdef VBM25_PROFILE
    if (int rc2 = bt->prof.alloc(8ull * 16 * RNW * R_GRID)) return rc2;  // (scan_win_kernel: 768 x 4 waves -- fewer)
    HIP_TRY(hipMemset(bt->prof.p, 0, 8ull * 16 * RNW * R_GRID));
#endif
    *out = bt.release();
    return VBM25_OK;
}



// The staged descriptors -- term ids, offsets, dense flags, the host's item order -- lie in ONE pinned block and go to ONE device
// block with one copy command (round 6: they were four commands into four buffers, 15 .. 25 us of a device's 100 us of host time per
// step on the multi-device route; vbm25_batch_run_impl points the kernels at the block's parts).
static int upload_staged(vbm25_batch *bt, const StagedLayout &L) {
    if (L.end > bt->qin.bytes) return set_error(VBM25_ERR_INVALID, "internal error: staged descriptors exceed the device block");
    HIP_TRY(hipMemcpyAsync(bt->qin.p, bt->pin_in, L.end, hipMemcpyHostToDevice, bt->lat_stream));
    bt->qin_live = true;
    return VBM25_OK;
}

// a pinned host block of at least `need` bytes (twice that when it grows: the next batch may be larger again)
static int pinned_fit(uint8_t *&p, size_t &bytes, size_t need) {
    if (need <= bytes) return VBM25_OK;
    if (p) HIP_TRY(hipHostFree(p));
    p = nullptr;
    bytes = 2 * need + 256;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p), bytes, hipHostMallocDefault));
    return VBM25_OK;
}

// The route of a validated query set (bt->h_dense and bt->h_postings hold its classes, plan its has_dense and range_mt), its item order
// in bt->h_order and, for the scratch plane, its id16 block starts in bt->h_id16_fb.  No HIP call, nothing committed.
static void plan_route(vbm25_batch *bt, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, bool fast, bool many,
                       uint32_t n_dense, QueryPlan &plan) {
    const uint8_t *dense = bt->h_dense.data();
    const unsigned long long *q_postings = bt->h_postings.data();
    const vbm25_index *ixh = bt->index;
    plan.n_term_pos = q_off[nq];
    plan.need_many = many || !bt->use_range;
    if (bt->use_range && nq && !many && !plan.has_dense && plan.range_mt != 0) {  // every query sparse, <= 16 indexed terms: the one-launch route
        unsigned long long most = 0;
        bool all = true;
        for (uint32_t q = 0; q < nq; ++q) {
            most = std::max(most, q_postings[q]);
            all = all && q_postings[q] != 0 && !dense[q];
        }
        if (all) {
            // items per query: by the largest query's postings, within the batch's target (every query gets the same number).
            // A handful of queries (the shim's nq = 1) is cut four times finer: its workgroups have the device to themselves,
            // and a second document range in flight is worth more than the merge of its lists costs (C2: 39.8 -> 36.2 us)
            const unsigned long long chunk = nq <= 8 ? std::max<unsigned long long>(bt->min_chunk / 4, 1) : bt->min_chunk;
            unsigned long long g = (most + chunk / 2) / chunk;
            g = std::min<unsigned long long>(g, std::max<unsigned long long>((bt->target_items + nq / 2) / nq, 1));
            g = std::min<unsigned long long>(std::max<unsigned long long>(g, 1), std::min<unsigned long long>(64, ixh->n_docs));
            // only where the launches it saves matter: a batch that fills the GPU runs slower through the FUSED
            // instantiation (more live state in the tile loop) than plan + scan + merge cost
            // scan_win_kernel (the window formulation): every query of <= 8 indexed terms, all with a window table, the lists of
            // comparable length (the MaxScore split of scan_range_kernel has nothing to skip) and neither too thin nor too thick
            // per 2^16-document window (32 .. 232 postings on average: one 8-byte load per lane holds a run)
            uint32_t win_g = 0;
            if (bt->tune.win && bt->k <= scan_win_max_k(plan.range_mt) && !ixh->term_win_host.empty()) {
                const double wins = std::max(1.0, double(ixh->n_docs) / 65536.0);
                double e_max = 1.0;
                bool ok = true;
                for (uint32_t q = 0; q < nq && ok; ++q) {
                    uint64_t dfs[8];
                    uint32_t n = 0;
                    ok = q_off[q + 1] - q_off[q] <= 64u;
                    for (uint32_t p = q_off[q]; p < q_off[q + 1] && ok; ++p) {
                        const uint32_t t = term_ids[p];
                        if (t >= ixh->n_terms) continue;
                        ok = n < scan_win_max_terms() && ixh->term_win_host[t] != UINT32_MAX;
                        if (!ok) break;
                        const double e = double(ixh->term_df_host[t]) / wins;
                        ok = bt->tune.win_force || (e >= 32.0 && e <= 232.0);
                        e_max = std::max(e_max, e);
                        dfs[n++] = ixh->term_df_host[t];
                    }
                    if (ok && !bt->tune.win_force && bt->tune.ne) {  // a prefix of the longest lists that scan_range_kernel would look up instead of scanning?
                        std::sort(dfs, dfs + n, [](uint64_t a, uint64_t b) { return a > b; });
                        uint64_t rest = 0;
                        for (uint32_t i = 0; i < n; ++i) rest += dfs[i];
                        for (uint32_t i = 0; i + 1 < n && ok; ++i) {
                            rest -= dfs[i];
                            ok = !(dfs[i] >= uint64_t(std::max(1u, bt->tune.ne_ratio)) * rest || dfs[i] * 16u >= ixh->n_docs);
                        }
                    }
                }
                if (ok) {
                    // items: one per resident wave (an item's setup is a chain of six round trips to memory: on C3 3072 items of 51
                    // windows take 0.270 ms, 6144 of 25 windows 0.287 ms)
                    // ... of as many windows as give every resident wave the same share of the batch's windows: L = ceil(nq n_win / waves).
                    // A query is cut into runs of L windows and a shorter rest (win_cut, run_window): with 14 waves per workgroup C3's
                    // 1024 queries x 153 windows are 3072 runs of 44 and 1024 of 21 for 3584 waves -- the short ones go last, two to a wave.
                    const uint32_t target = bt->tune.win_items ? bt->tune.win_items : scan_win_resident_waves(plan.range_mt, bt->k);
                    const uint32_t g_min = (ixh->n_win + 62u) / 63u;  // (an item holds at most 63 windows)
                    const uint64_t all_win = uint64_t(nq) * ixh->n_win;
                    const uint32_t len = uint32_t(std::min<uint64_t>(63u, std::max<uint64_t>(1u, (all_win + target - 1u) / target)));
                    uint32_t gw = std::max((ixh->n_win + len - 1u) / len, g_min);
                    gw = std::min(std::min(gw, ixh->n_win), bt->max_items / nq);
                    if (gw >= g_min && gw >= 1u) {
                        win_g = gw;
                        plan.win_len = (ixh->n_win + gw - 1u) / gw > len ? 0u : len;  // (0: equal runs -- the item limit cut the number of runs)
                    }
                }
            }
            if (win_g && !ixh->post_id16.p) {
                // An index without the post_id16 plane: every term position gets its blocks in the batch's scratch plane (a term's
                // blocks are full but its last: (df + 127) / 128 of them, post_fn_kernel's flag 8 saw to that), which
                // decode_id16_kernel fills ahead of the scan.  A batch whose terms need more blocks than the plane addresses takes
                // scan_range_kernel (or the general route), which decodes the blob's blocks itself.
                std::vector<uint32_t> &fbv = bt->h_id16_fb;
                fbv.resize(q_off[nq]);
                uint64_t blocks = 2;  // (block 0: what the null terms' run loads read)
                for (uint32_t p = 0; p < q_off[nq]; ++p) {
                    const uint32_t t = term_ids[p];
                    fbv[p] = uint32_t(std::min<uint64_t>(blocks, UINT32_MAX));
                    if (t < ixh->n_terms) blocks += (uint64_t(ixh->term_df_host[t]) + 127u) / 128u;
                }
                plan.id16_blocks = blocks;
                if (blocks > std::min<uint64_t>(bt->tune.id16_max_blocks, 0x00ffffffull)) {
                    win_g = 0;
                    plan.win_len = 0;
                }
            }
            if (bt->tune.fused && nq * g <= bt->tune.fused_items) {
                plan.route = Route::OneLaunch;
                plan.g = uint32_t(g);
                plan.fused_pinned = fast && nq <= 8 && !bt->timing;
            } else if (win_g || bt->tune.arith) {
                // Window, or the general route with its items made in the kernel (PlanFree: no plan_kernel, merge_kernel cleans)
                plan.route = win_g ? Route::Window : Route::PlanFree;
                if (win_g) g = win_g;
                plan.g = uint32_t(g);
                plan.id16_decode = win_g && !ixh->post_id16.p;
                // ... handed out longest first, as plan_kernel would (the host has the posting counts): queries by
                // descending postings, a query's g parts together
                std::vector<uint32_t> &ord = bt->h_order;
                ord.resize(size_t(nq) * g);
                std::vector<uint32_t> &qs = bt->h_order_q;
                qs.resize(nq);
                for (uint32_t q = 0; q < nq; ++q) qs[q] = q;
                {   // (queries of about the same length -- C3's -- keep their order: the sort, with the scratch buffer std::stable_sort
                    // allocates, was a quarter of a device's host time per step on the multi-device route)
                    unsigned long long lo = ~0ull, hi = 0;
                    for (uint32_t q = 0; q < nq; ++q) {
                        lo = std::min(lo, q_postings[q]);
                        hi = std::max(hi, q_postings[q]);
                    }
                    plan.order_identity = !(hi * 4 > lo * 5);  // (the queries keep their order: the skewed layout is arithmetic -- scan_win.h)
                    if (hi * 4 > lo * 5) std::stable_sort(qs.begin(), qs.end(), [&](uint32_t a, uint32_t b) { return q_postings[a] > q_postings[b]; });
                }

                const uint32_t wpw = win_g ? scan_win_wg(plan.range_mt, bt->k) : 0u;
                plan.win_skew = win_g == 3u && wpw == 12u && size_t(nq) * 3u <= scan_win_resident_waves(plan.range_mt, bt->k) && bt->tune.win_skew;
                // (queries of about the same length: the longest-first order buys nothing and costs every work item a dependent load --
                // unless there are more items than waves: then the queries' short last runs must be the ones drawn late)
                plan.order_useful = plan.win_skew || (!win_g || !bt->tune.win_guided ? q_postings[qs[0]] * 4 > q_postings[qs[nq - 1]] * 5 : true) ||
                                 (win_g && size_t(nq) * win_g > scan_win_resident_waves(plan.range_mt, bt->k));
                if (plan.win_skew) {
                    // One item per wave, three per query: a SIMD's three waves do not run equally fast -- the workgroup's waves 0..3
                    // (the first wave of every SIMD) lived 449 k cycles on C3, 4..7 497 k, 8..11 559 k, whatever priority they set
                    // themselves -- and the launch ends with the slowest.  A workgroup takes four queries; a query's three runs of
                    // windows, of lengths in the ratio of those speeds (win_cut, run_window), go to one wave of each kind.
                    // (nq mod 4 queries are left over: their items follow in plain order -- written to a partial last workgroup's
                    // slots they would land beyond the end of the array)
                    const uint32_t full = nq / 4u;
                    for (uint32_t wgi = 0; wgi < full; ++wgi)
                        for (uint32_t s4 = 0; s4 < 4u; ++s4)
                            for (uint32_t part = 0; part < 3u; ++part) ord[size_t(wgi) * 12u + part * 4u + s4] = qs[wgi * 4u + s4] * 3u + part;
                    for (uint32_t qi = full * 4u; qi < nq; ++qi)
                        for (uint32_t part = 0; part < 3u; ++part) ord[size_t(qi) * 3u + part] = qs[qi] * 3u + part;
                } else if (win_g)  // (parts of decreasing length: every query's first part, then every query's second one, ...)
                    for (uint32_t part = 0; part < g; ++part)
                        for (uint32_t i = 0; i < nq; ++i) ord[size_t(part) * nq + i] = qs[i] * uint32_t(g) + part;
                else
                for (uint32_t i = 0; i < nq; ++i)
                    for (uint32_t part = 0; part < g; ++part) ord[size_t(i) * g + part] = qs[i] * uint32_t(g) + part;
            }
        }
    }
    const bool with_order = plan.route == Route::PlanFree || plan.route == Route::Window;
    plan.staged = staged_layout(nq, q_off[nq], with_order ? size_t(nq) * plan.g : 0, plan.id16_decode);
    if (nq && q_off[1] != 0) {
        plan.q_stride = q_off[1];
        for (uint32_t q = 0; q < nq && plan.q_stride; ++q)
            if (q_off[q + 1] - q_off[q] != plan.q_stride) plan.q_stride = 0;
    }
    // the number of work items plan_kernel will make (same integer arithmetic): the persistent grids need not be larger (a single
    // query is a handful of items); with the dense-window kernel every dense query gets the same number of items (equal document counts)
    const uint32_t dense_target = std::max(256u, bt->tune.dense_items);
    plan.dense_c = plan.has_dense ? std::max(1u, (dense_target + n_dense / 2) / std::max(n_dense, 1u)) : 0u;
    if (plan.has_dense) {
        // (a few dense queries on a small corpus: no finer than 4096 items in all -- what the rounds before used -- or one item per
        // 2^16 documents, whichever is more: below that an item is all setup)
        const uint32_t floor_c = std::max(std::max(1u, 4096u / std::max(n_dense, 1u)), ixh->n_docs >> 16);
        if (bt->tune.dense_items == D_TARGET_ITEMS) plan.dense_c = std::min(plan.dense_c, floor_c);
    }
    unsigned long long sparse_postings = 0;
    for (uint32_t q = 0; q < nq; ++q)
        if (!(plan.dense_c && dense[q])) sparse_postings += q_postings[q];
    unsigned long long chunk = (sparse_postings + bt->target_items - 1) / bt->target_items;
    if (chunk < bt->min_chunk) chunk = bt->min_chunk;
    unsigned long long items = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        if (!q_postings[q]) continue;
        if (plan.dense_c && dense[q]) {
            items += std::min(plan.dense_c, ixh->n_docs);
            continue;
        }
        unsigned long long c = (q_postings[q] + chunk / 2) / chunk;
        if (c == 0) c = 1;
        if (c > ixh->n_docs) c = ixh->n_docs;
        items += c;
    }
    plan.range_grid = uint32_t(std::min<unsigned long long>(std::max<unsigned long long>(items, 1), std::max(1u, bt->tune.range_grid)));
    plan.dense_grid = uint32_t(std::min<unsigned long long>(std::max<unsigned long long>(items, 1), std::max(1u, bt->tune.dense_grid)));
#ifdef VBM25_PROFILE
    plan.range_grid = std::min<uint32_t>(plan.range_grid, R_GRID);  // (the phase counters are sized for R_GRID workgroups)
#endif
}

// The decided query set to the batch: the scratch plane, then the descriptors -- staged in pinned memory (fast) or copied to the
// separate device buffers -- and the plan last.  A failure on the way leaves a half-committed set: the caller clears it.
static int commit_queries(vbm25_batch *bt, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, bool fast, const QueryPlan &plan) {
    if (int rc = use_device(bt->index->device)) return rc;
    if (plan.route == Route::Exhaustive) {
        bt->h_terms.assign(term_ids, term_ids + q_off[nq]);
        bt->h_off.assign(q_off, q_off + nq + 1);
    } else {
        if (plan.id16_decode) {  // (the scratch plane grows with the largest batch it has held)
            const size_t need = 256ull * plan.id16_blocks + 1024;
            if (need > bt->id16_tmp.bytes) {
                if (bt->last_stream || bt->lat_stream) HIP_TRY(hipDeviceSynchronize());  // (a run still reading the old plane)
                if (bt->id16_tmp.p) HIP_TRY(hipFree(bt->id16_tmp.p));
                bt->id16_tmp.p = nullptr;
                bt->id16_tmp.bytes = 0;
                if (int rc = bt->id16_tmp.alloc(need + need / 4)) return rc;
                HIP_TRY(hipMemset(bt->id16_tmp.p, 0, bt->id16_tmp.bytes));
            }
            if (!fast && q_off[nq]) HIP_TRY(hipMemcpy(bt->id16_fb.p, bt->h_id16_fb.data(), 4ull * q_off[nq], hipMemcpyHostToDevice));
        }
        const StagedLayout &L = plan.staged;
        // (the fast path stages the item order with the queries and copies it on the batch's own stream: upload_staged)
        if (!fast && L.id16 > L.order) HIP_TRY(hipMemcpy(bt->item_order.p, bt->h_order.data(), L.id16 - L.order, hipMemcpyHostToDevice));
        if (fast) {
            // staged in pinned memory.  One-launch route with fused_pinned: the kernel reads the queries from there and writes the hits
            // into the pinned output buffer -- no copy is enqueued at all.  The other routes: copied on the batch's own stream,
            // nothing waits here.
            if (int rc = pinned_fit(bt->pin_in, bt->pin_in_bytes, L.end)) return rc;
            if (int rc = pinned_fit(bt->pin_out, bt->pin_out_bytes, pin_out_records(nq) + sizeof(vbm25_hit) * size_t(nq) * bt->k)) return rc;
            if (!bt->lat_stream) HIP_TRY(hipStreamCreateWithFlags(&bt->lat_stream, hipStreamNonBlocking));
            if (L.off) std::memcpy(bt->pin_in, term_ids, L.off);
            std::memcpy(bt->pin_in + L.off, q_off, L.dense - L.off);
            if (nq) std::memcpy(bt->pin_in + L.dense, bt->h_dense.data(), nq);
            if (L.id16 > L.order) std::memcpy(bt->pin_in + L.order, bt->h_order.data(), L.id16 - L.order);
            if (L.sel) {
                if (L.sel > L.id16) std::memcpy(bt->pin_in + L.id16, bt->h_id16_fb.data(), L.sel - L.id16);
                std::memcpy(bt->pin_in + L.sel, bt->stage_sel, L.end - L.sel);
            } else if (L.end > L.id16) std::memcpy(bt->pin_in + L.id16, bt->h_id16_fb.data(), L.end - L.id16);
            if (!(plan.route == Route::OneLaunch && plan.fused_pinned))
                if (int rc = upload_staged(bt, L)) return rc;
        } else {
            bt->qin_live = false;
            if (q_off[nq]) HIP_TRY(hipMemcpy(bt->term_ids.p, term_ids, 4ull * q_off[nq], hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(bt->q_off.p, q_off, 4ull * (nq + 1), hipMemcpyHostToDevice));
            if (nq) HIP_TRY(hipMemcpy(bt->q_dense.p, bt->h_dense.data(), nq, hipMemcpyHostToDevice));
        }
        bt->win_nofuse = false;
    }
    bt->nq = nq;
    bt->plan = plan;
    return VBM25_OK;
}

static int batch_set_queries_body(vbm25_batch *bt, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, bool fast) {
    if (!bt || !q_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (!term_ids && nq && q_off[nq] != 0) return set_error(VBM25_ERR_INVALID, "term_ids is NULL but the queries have terms");
    if (nq > bt->max_queries) return set_error(VBM25_ERR_INVALID, "%u queries exceed the batch capacity %u", nq, bt->max_queries);
    if (q_off[0] != 0) return set_error(VBM25_ERR_INVALID, "q_off[0] must be 0");
    QueryPlan plan;
    bool many = false;
    uint32_t n_dense = 0;
    // Routing: scan_range_kernel is built for sparse queries; a query with many postings per document (Zipf head terms)
    // takes the dense-window kernel, one with more than 16 indexed terms scan_many_kernel.  (The scratch vectors were
    // sized when the batch was created: nothing is allocated here.)
    const unsigned long long dense_x1000 = (unsigned long long)std::max(0ll, bt->tune.dense_x1000);
    uint8_t *dense = bt->h_dense.data();
    unsigned long long *q_postings = bt->h_postings.data();
    for (uint32_t q = 0; q < nq; ++q) {
        if (q_off[q + 1] < q_off[q]) return set_error(VBM25_ERR_INVALID, "q_off not monotone at query %u", q);
        uint32_t valid = 0;
        unsigned long long postings = 0;
        for (uint32_t p = q_off[q]; p < q_off[q + 1]; ++p) {
            if (p > q_off[q] && term_ids[p] <= term_ids[p - 1])  // Query::checked_new, vector.rs:106-110
                return set_error(VBM25_ERR_INVALID, "query %u: term ids must be strictly ascending", q);
            valid += term_ids[p] < bt->index->n_terms;
            if (term_ids[p] < bt->index->n_terms) postings += bt->index->term_df_host[term_ids[p]];
        }
        q_postings[q] = postings;
        dense[q] = 0;
        if (postings * 1000ull >= dense_x1000 * bt->index->n_docs) {
            dense[q] = 1;
            many = true;
            n_dense += postings != 0;
        }
        if (bt->use_range) {  // sparse queries of <= 16 terms: scan_range_kernel; dense ones: scan_dense_kernel; the rest: scan_many_kernel
            many |= valid > 16u;
            plan.has_dense |= bt->use_dense && dense[q] && valid <= (uint32_t)D_T;
            if (!dense[q] && valid <= 16u) plan.range_mt = std::max(plan.range_mt, valid);
        } else {
            many = true;
        }
        if (valid > MAX_TERMS)
            return set_error(VBM25_ERR_UNSUPPORTED, "query %u has %u indexed terms; the GPU path handles up to %d", q, valid, MAX_TERMS);
    }
    if (q_off[nq] > bt->max_terms) return set_error(VBM25_ERR_INVALID, "%u terms exceed the batch capacity %u", q_off[nq], bt->max_terms);
    if (bt->bigk) plan.route = Route::Exhaustive;
    else plan_route(bt, term_ids, q_off, nq, fast, many, n_dense, plan);
    if (fast && bt->stage_sel && nq && plan.route != Route::Exhaustive) {  // the selectors ride in the staged block: one upload command
        plan.staged.sel = plan.staged.end;
        plan.staged.end += 4ull * nq;
    }
    return commit_queries(bt, term_ids, q_off, nq, fast, plan);
}

// The batch holds no queries: run enqueues nothing, fetch writes nothing.  What a failed set_queries leaves (include/vbm25.h) -- also
// when it failed after committing part of the new set (an allocation, a copy): the next run must not launch on a mix of the old query
// set's descriptors and the new one's count.  Filter and growing segment stay attached.
void batch_clear_queries(vbm25_batch *bt) {
    bt->nq = 0;
    bt->plan = QueryPlan{};
    bt->qin_live = false;
    bt->win_nofuse = false;
    bt->win_fused_run = false;
}

int vbm25_batch_set_queries_impl(vbm25_batch *bt, const uint32_t *term_ids, const uint32_t *q_off,
                            uint32_t nq, bool fast) {
    int rc;
    try {
        rc = batch_set_queries_body(bt, term_ids, q_off, nq, fast);
    } catch (...) {  // (out of host memory: guarded() makes it the call's error code)
        if (bt) batch_clear_queries(bt);
        throw;
    }
    if (rc && bt) batch_clear_queries(bt);
    return rc;
}

// The per-launch state the routes without plan_kernel need zero -- threshold, histogram, counters and, beyond the one-launch route,
// the give-up flags and list counts -- unless the last run left it so.  Those routes leave it zero themselves, but only a run that was
// enqueued completely counts: the flag is cleared before anything is enqueued and set at the very end (an error return in between, or
// a run on the general route, forces the memsets next time).  Consecutive runs of one batch must use one stream.
static int reset_launch_state(vbm25_batch *bt, hipStream_t st, bool one_launch) {
    const bool clean = bt->state_clean;
    bt->state_clean = false;
    if (clean) return VBM25_OK;
    HIP_TRY(hipMemsetAsync(bt->hist.p, 0, 4ull * CUR_HB * bt->max_queries, st));
    HIP_TRY(hipMemsetAsync(bt->theta.p, 0, 8ull * bt->max_queries, st));
    HIP_TRY(hipMemsetAsync(bt->work_ctr.p, 0, 8, st));
    HIP_TRY(hipMemsetAsync(bt->fused_state.p, 0, 4ull * (bt->max_queries + 1), st));
    if (one_launch) return VBM25_OK;
    HIP_TRY(hipMemsetAsync(bt->fail_any.p, 0, 4, st));
    HIP_TRY(hipMemsetAsync(bt->item_failed.p, 0, 4ull * bt->max_items, st));
    HIP_TRY(hipMemsetAsync(bt->res_cnt.p, 0, 4ull * bt->max_items * bt->lpi, st));
    return VBM25_OK;
}

// timing on: the batch's next event pair, the first one recorded on st now; e1 is the second, for the caller to record where the timed
// region ends (nullptr with timing off)
static int take_events(vbm25_batch *bt, hipStream_t st, hipEvent_t &e1) {
    e1 = nullptr;
    if (!bt->timing) return VBM25_OK;
    if (bt->events_used == bt->events.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        bt->events.emplace_back(a, b);
    }
    e1 = bt->events[bt->events_used].second;
    HIP_TRY(hipEventRecord(bt->events[bt->events_used++].first, st));
    return VBM25_OK;
}

// The kernels' view of the batch as the general route sees it; the other routes change a few fields
static DevBatch dev_batch(const vbm25_batch *bt) {
    DevBatch db{};
    db.term_ids = bt->term_ids.as<uint32_t>();
    db.q_off = bt->q_off.as<uint32_t>();
    db.q_dense = bt->q_dense.as<uint8_t>();
    db.item_order = bt->item_order.as<uint32_t>();
    if (bt->qin_live) {  // the staged descriptors: one device block (upload_staged)
        const StagedLayout &L = bt->plan.staged;
        uint8_t *qp = bt->qin.as<uint8_t>();
        db.term_ids = reinterpret_cast<const uint32_t *>(qp);
        db.q_off = reinterpret_cast<const uint32_t *>(qp + L.off);
        db.q_dense = qp + L.dense;
        if (L.id16 > L.order)  // (the host's item order of the routes without plan_kernel, which writes its own into item_order)
            db.item_order = reinterpret_cast<uint32_t *>(qp + L.order);
    }
    db.nq = bt->nq;
    db.k = bt->k;
    db.items = bt->items.as<Item>();
    db.n_items = bt->n_items.as<uint32_t>();
    db.q_item_base = bt->q_item_base.as<uint32_t>();
    db.theta = bt->theta.as<unsigned long long>();
    db.res_score = bt->res_score.as<double>();
    db.res_doc = bt->res_doc.as<uint32_t>();
    db.res_cnt = bt->res_cnt.as<uint32_t>();
    db.hits = bt->hits.as<vbm25_hit>();
    db.n_hits = bt->n_hits.as<uint32_t>();
    if (bt->results_pinned_now) {
        db.n_hits = reinterpret_cast<uint32_t *>(bt->pin_out + 8);
        db.hits = reinterpret_cast<vbm25_hit *>(bt->pin_out + pin_out_records(bt->nq));
    }
    if (bt->filt_on) {
        db.filt_words = bt->filter->bits.as<unsigned long long>();
        db.filt_sel = bt->filt_sel.as<uint32_t>();
        if (bt->plan.staged.sel)  // staged with the queries (a run that reads them from pinned memory: run_one_launch)
            db.filt_sel = reinterpret_cast<const uint32_t *>(bt->qin.as<uint8_t>() + bt->plan.staged.sel);
        db.filt_stride = bt->filter->words;
    }
    db.error_flag = bt->error_flag.as<uint32_t>();
    db.item_failed = bt->item_failed.as<uint32_t>();
    db.prof = bt->prof.as<unsigned long long>();
    db.hist = bt->hist.as<uint32_t>();
    db.work_ctr = bt->work_ctr.as<uint32_t>();
    db.max_items = bt->max_items;
    db.dbg = bt->dbg.as<uint32_t>();
    db.lpi = bt->lpi;
    db.range_max_terms = bt->use_range ? 16u : 0u;
    db.ne_on = bt->tune.ne ? 1u : 0u;
    db.ne_ratio = std::max(1u, bt->tune.ne_ratio);
    db.dense_on = bt->use_dense ? 1u : 0u;
    db.win_dbg = bt->tune.dbg;
    db.fail_any = bt->fail_any.as<uint32_t>();
    db.q_failed = bt->q_failed.as<uint32_t>();
    db.theta_last = bt->theta_last.as<unsigned long long>();
    db.many_expected = bt->plan.need_many ? 1u : 0u;
    db.merge_clean = 0;
    db.order_on = 0;
    db.fused_state = bt->fused_state.as<uint32_t>();
    db.fused_g = 0;
    return db;
}

// k > 1024: per query, one accumulation launch per term, the filter's mask, a radix sort of the scores, the first k of them
static int run_exhaustive(vbm25_batch *bt, hipStream_t st) {
    const DevIndex &dix = bt->index->dev;
    const uint32_t n = bt->index->n_docs;
    for (uint32_t q = 0; q < bt->nq; ++q) {
        HIP_TRY(hipMemsetAsync(bt->bk_acc.p, 0, 8ull * n, st));
        for (uint32_t p = bt->h_off[q]; p < bt->h_off[q + 1]; ++p) {
            const uint32_t t = bt->h_terms[p];
            if (t >= bt->index->n_terms) continue;  // search.rs:59-61
            const uint32_t nb = (bt->index->term_df_host[t] + 127) / 128;
            bigk_accum_kernel<<<std::min<uint32_t>((nb + 3) / 4, 4096u), 256, 0, st>>>(dix, t, bt->bk_acc.as<double>());
        }
        if (bt->filt_on && bt->h_filt_sel[q] != UINT32_MAX)
            bigk_mask_kernel<<<std::min<uint32_t>((n + 255) / 256, 4096u), 256, 0, st>>>(
                bt->filter->bits.as<unsigned long long>() + size_t(bt->h_filt_sel[q]) * bt->filter->words, n, bt->bk_acc.as<double>());
        size_t tmp = bt->bk_tmp_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(bt->bk_tmp.p, tmp, bt->bk_acc.as<unsigned long long>(),
                                                              bt->bk_keys.as<unsigned long long>(), bt->bk_iota.as<uint32_t>(),
                                                              bt->bk_docs.as<uint32_t>(), (int)n, 0, 64, st));
        bigk_emit_kernel<<<(bt->k + 255) / 256, 256, 0, st>>>(dix, bt->bk_keys.as<unsigned long long>(), bt->bk_docs.as<uint32_t>(), n,
                                                              bt->k, bt->hits.as<vbm25_hit>() + size_t(q) * bt->k,
                                                              bt->n_hits.as<uint32_t>() + q);
    }
    HIP_TRY(hipGetLastError());
    return VBM25_OK;
}

// A handful of sparse queries (vbm25_search_batch): ONE launch -- scan_range_kernel plans, scans and merges, and leaves threshold,
// histogram and counters zero
static int run_one_launch(vbm25_batch *bt, hipStream_t st, DevBatch db) {
    const QueryPlan &plan = bt->plan;
    const DevIndex &ix = bt->index->dev;
    if (int rc = reset_launch_state(bt, st, true)) return rc;
    db.fused_g = plan.g;
    db.dense_on = 0;
    if (plan.fused_pinned) {  // queries read from, hits written to pinned host memory
        db.term_ids = reinterpret_cast<const uint32_t *>(bt->pin_in);
        db.q_off = reinterpret_cast<const uint32_t *>(bt->pin_in + plan.staged.off);
        if (bt->filt_on && plan.staged.sel) db.filt_sel = reinterpret_cast<const uint32_t *>(bt->pin_in + plan.staged.sel);
        db.n_hits = reinterpret_cast<uint32_t *>(bt->pin_out + 8);
        db.hits = reinterpret_cast<vbm25_hit *>(bt->pin_out + pin_out_records(bt->nq));
    }
    hipEvent_t e1;
    if (int rc = take_events(bt, st, e1)) return rc;
    const uint32_t fgrid = std::min<uint32_t>(bt->nq * plan.g, R_GRID);
    const int rcf = dispatch_k(bt->k, [&](auto kmax) {
        constexpr int KM = decltype(kmax)::value;
        if constexpr (KM <= REG_K) {
            if (plan.range_rt() == 8) scan_range_kernel<KM, 8, true><<<fgrid, RWG, 0, st>>>(ix, db);
            else scan_range_kernel<KM, 16, true><<<fgrid, RWG, 0, st>>>(ix, db);
            if (!plan.fused_pinned) {
                // an item the kernel gave up (rare) is redone by scan_many_kernel and its query merged by merge_kernel;
                // both find nothing to do otherwise.  (The pinned flavour leaves that to the host: rerun_and_fetch.)
                scan_many_kernel<KM><<<std::min<uint32_t>(bt->nq * plan.g, TARGET_ITEMS), WG, 0, st>>>(ix, db);
                if (bt->timing) (void)hipEventRecord(e1, st);
                DevBatch dm = db;
                dm.merge_marked = 1;
                merge_kernel<KM><<<bt->nq, 64, 0, st>>>(ix, dm);
            } else if (bt->timing) {
                (void)hipEventRecord(e1, st);
            }
        }
        return int(VBM25_OK);
    });
    if (rcf) return rcf;
    HIP_TRY(hipGetLastError());
    bt->state_clean = true;
    return VBM25_OK;
}

// Every query sparse, <= 8 terms of comparable length: scan_win_kernel (its waves make their work items themselves), then as on the
// plan-free route: scan_many_kernel leaves at once unless an item was given up, merge_kernel merges and cleans.
static int run_window(vbm25_batch *bt, hipStream_t st, DevBatch db) {
    const QueryPlan &plan = bt->plan;
    const DevIndex &ix = bt->index->dev;
    if (int rc = reset_launch_state(bt, st, false)) return rc;
    db.fused_g = plan.g;  // (merge_kernel: a query's lists are those of its g items)
    db.win_g = plan.g;
    {
        // a query's items: runs of windows of decreasing length (weights g + 1, g, ..., 2), handed out longest first -- the
        // last items drawn, which decide when the launch ends, are the short ones.  Equal runs when a run would exceed the
        // 63 windows an item can hold, or with more than 16 items per query.
        const uint32_t gq = plan.g, nwin = bt->index->n_win;
        std::memset(db.win_cut, 0, sizeof db.win_cut);
        if (plan.win_skew) {  // (the three kinds of waves: 59 / 52 / 42 of C3's 153 windows: the third wave of a SIMD takes 1.5 times the first one's time per window)
            db.win_cut[0] = 0;
            db.win_cut[1] = uint32_t(uint64_t(nwin) * uint32_t(bt->tune.win_cut1) / 1000u);
            db.win_cut[2] = uint32_t(uint64_t(nwin) * uint32_t(bt->tune.win_cut2) / 1000u);
            db.win_cut[3] = nwin;
            if (db.win_cut[1] > 63u || db.win_cut[2] - db.win_cut[1] > 63u || nwin - db.win_cut[2] > 63u) std::memset(db.win_cut, 0, sizeof db.win_cut);
        } else if (gq <= 16u && plan.win_len && uint64_t(plan.win_len) * (gq - 1u) < nwin) {
            // runs of win_len windows and a shorter rest (plan_route: every resident wave the same share of the windows)
            for (uint32_t p = 0; p < gq; ++p) db.win_cut[p] = plan.win_len * p;
            db.win_cut[gq] = nwin;
        }
    }
    db.lpi = 1;
    db.hist = nullptr;       // (this kernel keeps no histogram of accepted documents: merge_kernel has none to clean)
    db.dense_on = 0;
    db.many_expected = 0;
    db.merge_clean = 1;
    // (2: the skewed layout of queries in the caller's order is computed by the kernel itself, nobody loads item_order)
    db.order_on = plan.order_useful ? (plan.win_skew && plan.order_identity && bt->tune.win_order_arith ? 2u : 1u) : 0u;
    db.q_stride = plan.q_stride;
    hipEvent_t e1;
    if (int rc = take_events(bt, st, e1)) return rc;
    const uint32_t wmt = std::min(plan.range_mt, 8u), wpw = scan_win_wg(wmt, bt->k);
    const uint32_t wgrid = std::min<uint32_t>((bt->nq * plan.g + wpw - 1u) / wpw, bt->tune.win_grid ? bt->tune.win_grid : scan_win_resident_waves(wmt, bt->k) / wpw);
    // One launch (round 6): the wave that finishes a query's last item merges the query's lists, writes its records and leaves
    // the per-launch state zero.  A query with an item the kernel gave up comes back with the count NONE32: whoever hands the
    // records to the caller (vbm25_batch_fetch_impl) re-runs the batch with scan_many_kernel and merge_kernel behind the scan.
    // (only when every wave has at most one item: the kernel's merge sits behind its item loop)
    const bool fuse = bt->tune.win_fuse && !bt->win_nofuse && !bt->device_consumer && !bt->growing && uint64_t(bt->nq) * plan.g <= scan_win_resident_waves(wmt, bt->k) && !bt->tune.win_grid;
    db.win_fuse = fuse ? 1u : 0u;
    bt->win_fused_run = fuse;
    bt->win_order_on = db.order_on;
    if (plan.id16_decode) {
        // An index without the post_id16 plane: the ids of the batch's terms, unpacked from the blob into the batch's scratch
        // plane (decode_id16.h) -- inside the timed region: kernel_ms is the decode and the scan.
        const StagedLayout &L = plan.staged;
        db.id16_fb = bt->id16_fb.as<uint32_t>();
        if (bt->qin_live && (L.sel ? L.sel : L.end) > L.id16) db.id16_fb = reinterpret_cast<const uint32_t *>(bt->qin.as<uint8_t>() + L.id16);
        if (plan.n_term_pos) decode_id16_kernel<<<plan.n_term_pos, DI_WAVES * 64, 0, st>>>(ix, db.term_ids, db.id16_fb, bt->id16_tmp.as<uint32_t>());
        DevIndex ixw = ix;
        ixw.post_id16 = bt->id16_tmp.as<uint32_t>();
        HIP_TRY(scan_win_launch(ixw, db, wmt, wgrid, st));
    } else
    HIP_TRY(scan_win_launch(ix, db, wmt, wgrid, st));
    if (fuse) {
        if (bt->timing) (void)hipEventRecord(e1, st);
    } else
    (void)dispatch_k(bt->k, [&](auto kmax) {
        constexpr int KM = decltype(kmax)::value;
        if constexpr (KM <= REG_K) {
            scan_many_kernel<KM><<<64, WG, 0, st>>>(ix, db);
            if (bt->timing) (void)hipEventRecord(e1, st);
            merge_kernel<KM><<<bt->nq, 64, 0, st>>>(ix, db);
        }
        return int(VBM25_OK);
    });
    HIP_TRY(hipGetLastError());
    bt->state_clean = true;
    return VBM25_OK;
}

// Every query sparse, <= 16 terms: the scan kernel makes the work items itself (no plan_kernel), scan_many_kernel is a small grid that
// leaves at once unless an item was given up, merge_kernel merges and leaves the per-launch state zero.
static int run_plan_free(vbm25_batch *bt, hipStream_t st, DevBatch db) {
    const QueryPlan &plan = bt->plan;
    const DevIndex &ix = bt->index->dev;
    if (int rc = reset_launch_state(bt, st, false)) return rc;
    db.fused_g = plan.g;
    db.dense_on = 0;
    db.many_expected = 0;
    db.merge_clean = 1;
    db.order_on = 1;
    hipEvent_t e1;
    if (int rc = take_events(bt, st, e1)) return rc;
    const uint32_t agrid = std::min<uint32_t>(bt->nq * plan.g, std::max(1u, bt->tune.range_grid));
    const int rca = dispatch_k(bt->k, [&](auto kmax) {
        constexpr int KM = decltype(kmax)::value;
        if constexpr (KM <= REG_K) {
            if (plan.range_rt() == 8) scan_range_kernel<KM, 8><<<agrid, RWG, 0, st>>>(ix, db);
            else scan_range_kernel<KM, 16><<<agrid, RWG, 0, st>>>(ix, db);
            scan_many_kernel<KM><<<64, WG, 0, st>>>(ix, db);
            if (bt->timing) (void)hipEventRecord(e1, st);
            merge_kernel<KM><<<bt->nq, 64, 0, st>>>(ix, db);
        }
        return int(VBM25_OK);
    });
    if (rca) return rca;
    HIP_TRY(hipGetLastError());
    bt->state_clean = true;
    return VBM25_OK;
}

// plan_kernel makes the work items; the sparse, dense and many-term kernels scan them; merge_kernel merges every query's lists
static int run_general(vbm25_batch *bt, hipStream_t st, const DevBatch &db) {
    const QueryPlan &plan = bt->plan;
    const DevIndex &ix = bt->index->dev;
    const bool range = bt->use_range;
    bt->state_clean = false;
    if (range) HIP_TRY(hipMemsetAsync(bt->hist.p, 0, 4ull * CUR_HB * bt->nq, st));
    plan_kernel<<<1, PLAN_WG, 0, st>>>(ix, db, bt->max_items, bt->target_items, bt->min_chunk, plan.dense_c);
    hipEvent_t e1;
    if (int rc = take_events(bt, st, e1)) return rc;
    const uint32_t grid = std::min<uint32_t>(bt->max_items, TARGET_ITEMS);
    const int rc = dispatch_k(bt->k, [&](auto kmax) {
        constexpr int KM = decltype(kmax)::value;
        if constexpr (KM <= REG_K) {
            if (range) {  // persistent 8-wave workgroups
                if (plan.range_rt() == 8) scan_range_kernel<KM, 8><<<plan.range_grid, RWG, 0, st>>>(ix, db);
                else if (plan.range_rt() == 16) scan_range_kernel<KM, 16><<<plan.range_grid, RWG, 0, st>>>(ix, db);
            }
        }
        if constexpr (KM <= D_KMAX) {
            if (plan.has_dense) scan_dense_kernel<KM><<<plan.dense_grid, DWG, 0, st>>>(ix, db);
        }
        // many-term queries, every query of 256 < k <= 1024, and items the first-choice kernel gave up on (empty launch: 5 us)
        scan_many_kernel<decltype(kmax)::value><<<grid, WG, 0, st>>>(ix, db);
        if (bt->timing) HIP_TRY(hipEventRecord(e1, st));  // the events bracket every posting-scan kernel of the step
        merge_kernel<decltype(kmax)::value><<<bt->nq, 64, 0, st>>>(ix, db);
        return int(VBM25_OK);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return VBM25_OK;
}

int vbm25_batch_run_impl(vbm25_batch *bt, void *hip_stream) {
    if (!bt) return set_error(VBM25_ERR_INVALID, "batch is NULL");
    if (!bt->nq) return VBM25_OK;
    if (int rc = use_device(bt->index->device)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    bt->last_stream = st;
    bt->win_fused_run = false;
    bt->download_enqueued = false;
    bt->results_pinned_now = false;
    if (bt->index->n_docs == 0) {  // empty sealed segment: no hits (the growing segment is the shim's, search.rs:83-135)
        HIP_TRY(hipMemsetAsync(bt->n_hits.p, 0, 4ull * bt->nq, st));
        // no kernel runs, and the fetch copies all nq x k records out: zeros, not what the allocator left in the buffer
        if (bt->k) HIP_TRY(hipMemsetAsync(bt->hits.p, 0, sizeof(vbm25_hit) * size_t(bt->nq) * bt->k, st));
        return VBM25_OK;
    }
    const Route route = bt->plan.route;
    if (route == Route::Exhaustive) return run_exhaustive(bt, st);
    bt->results_pinned_now = bt->pinned_results && route != Route::OneLaunch && bt->lat_stream && bt->pin_out && !bt->growing;
    const DevBatch db = dev_batch(bt);
    switch (route) {
    case Route::OneLaunch: return run_one_launch(bt, st, db);
    case Route::Window: return run_window(bt, st, db);
    case Route::PlanFree: return run_plan_free(bt, st, db);
    default: return run_general(bt, st, db);
    }
}

// the last run's flag, counts and records to the batch's pinned buffer, behind the run on its private stream (vbm25_search_batch's
// and vbm25_multi_batch_run's general routes; the one-launch route has written them there itself)
int vbm25_batch_enqueue_download(vbm25_batch *bt) {
    if (bt->bigk || !bt->lat_stream || (bt->plan.route == Route::OneLaunch && bt->plan.fused_pinned)) return VBM25_OK;
    if (int rc = use_device(bt->index->device)) return rc;
    const size_t nh = sizeof(vbm25_hit) * size_t(bt->nq) * bt->k, rec = pin_out_records(bt->nq);
    if (int rc = pinned_fit(bt->pin_out, bt->pin_out_bytes, rec + nh)) return rc;
    HIP_TRY(hipMemcpyAsync(bt->pin_out, bt->error_flag.p, 4, hipMemcpyDeviceToHost, bt->lat_stream));
    if (bt->nq && !bt->results_pinned_now) {
        HIP_TRY(hipMemcpyAsync(bt->pin_out + 8, bt->n_hits.p, 4ull * bt->nq, hipMemcpyDeviceToHost, bt->lat_stream));
        HIP_TRY(hipMemcpyAsync(bt->pin_out + rec, bt->hits.p, nh, hipMemcpyDeviceToHost, bt->lat_stream));
    }
    bt->download_enqueued = true;
    return VBM25_OK;
}

static bool any_marked(const uint32_t *cnt, uint32_t nq) {
    for (uint32_t q = 0; q < nq; ++q)
        if (cnt[q] == UINT32_MAX) return true;
    return false;
}
// Records incomplete: a count of NONE32 marks a query with an item a one-launch kernel gave up (scan_win_kernel: more second arrivals in
// a window than its list holds, a term frequency above 255).  The batch is re-routed and run again on the same stream, before any
// record reaches the caller.  The pinned one-launch route moves to the general route, whose kernels read the staged block; the
// one-launch form of scan_win_kernel gets scan_many_kernel and merge_kernel behind it for the rest of this query set.
static int rerun_and_fetch(vbm25_batch *bt, vbm25_hit *hits, uint32_t *n_hits, bool fast) {
    if (bt->plan.route == Route::OneLaunch) {
        bt->plan.route = Route::General;
        if (int rc = upload_staged(bt, bt->plan.staged)) return rc;
    } else {
        bt->win_nofuse = true;
        bt->state_clean = false;  // (the one-launch run left fail_any set)
    }
    bt->download_enqueued = false;
    if (int rc = vbm25_batch_run_impl(bt, bt->last_stream)) return rc;
    return vbm25_batch_fetch_impl(bt, hits, n_hits, fast);
}
int vbm25_batch_fetch_impl(vbm25_batch *bt, vbm25_hit *hits, uint32_t *n_hits, bool fast) {
    if (!bt || (!hits && bt->nq) || (!n_hits && bt->nq)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = use_device(bt->index->device)) return rc;
    const size_t nh = sizeof(vbm25_hit) * size_t(bt->nq) * bt->k;
    if (fast && bt->lat_stream && bt->plan.route == Route::OneLaunch && bt->plan.fused_pinned) {
        // the kernel wrote counts and hits into the pinned buffer: one synchronisation
        HIP_TRY(hipStreamSynchronize(bt->lat_stream));
        const uint32_t *pin_cnt = reinterpret_cast<const uint32_t *>(bt->pin_out + 8);
        if (any_marked(pin_cnt, bt->nq)) return rerun_and_fetch(bt, hits, n_hits, fast);  // an item needs scan_many_kernel
        std::memcpy(n_hits, pin_cnt, 4ull * bt->nq);
        std::memcpy(hits, bt->pin_out + pin_out_records(bt->nq), nh);
        return VBM25_OK;
    }
    if (fast && bt->lat_stream) {  // flag, counts and hits come down asynchronously; one synchronisation
        if (!bt->download_enqueued)
            if (int rc = vbm25_batch_enqueue_download(bt)) return rc;
        bt->download_enqueued = false;
        HIP_TRY(hipStreamSynchronize(bt->lat_stream));
        uint32_t flag = 0;
        std::memcpy(&flag, bt->pin_out, 4);
        if (flag) {
            HIP_TRY(hipMemset(bt->error_flag.p, 0, 4));
            return set_error(VBM25_ERR_DEVICE, "device-side planner overflow (flag %u)", flag);
        }
        if (bt->nq) {
            const uint32_t *pin_cnt = reinterpret_cast<const uint32_t *>(bt->pin_out + 8);
            if (bt->win_fused_run && any_marked(pin_cnt, bt->nq)) return rerun_and_fetch(bt, hits, n_hits, fast);
            std::memcpy(n_hits, pin_cnt, 4ull * bt->nq);
            std::memcpy(hits, bt->pin_out + pin_out_records(bt->nq), nh);
        }
        return VBM25_OK;
    }
    // the batch's own stream, not the device: other streams of the process (a gather, another batch) keep running
    hipStream_t st = bt->last_stream;
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, bt->error_flag.p, 4, hipMemcpyDeviceToHost, st));
    if (bt->nq) {
        HIP_TRY(hipMemcpyAsync(hits, bt->hits.p, nh, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_hits, bt->n_hits.p, 4ull * bt->nq, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (flag) {
        HIP_TRY(hipMemsetAsync(bt->error_flag.p, 0, 4, st));
        HIP_TRY(hipStreamSynchronize(st));
        return set_error(VBM25_ERR_DEVICE, "device-side planner overflow (flag %u)", flag);
    }
    if (bt->nq && bt->win_fused_run && any_marked(n_hits, bt->nq)) return rerun_and_fetch(bt, hits, n_hits, fast);
    return VBM25_OK;
}


// the current queries' kernels make their work items themselves and merge_kernel cleans up behind them
static bool plan_free_kernels(const vbm25_batch *bt) { return bt->plan.route == Route::PlanFree || bt->plan.route == Route::Window; }


// The index's batch object for the one-shot entry points (slot: vbm25_search_batch's or the growing ones'), re-used while the shape
// and the tuning switches fit: device buffers of a batch are far more expensive to create than a search.  pinned_results: host
// buffers in, host buffers out -- nobody reads the batch's records on the device.
static int scratch_batch(vbm25_index *ix, vbm25_batch *vbm25_index::*slot, bool pinned_results, uint32_t nq, const uint32_t *q_off,
                         uint32_t k, vbm25_batch **out) {
    vbm25_batch *&bt = ix->*slot;
    const uint32_t n_terms = q_off[nq] ? q_off[nq] : 1;
    if (!bt || bt->k != k || bt->max_queries < nq || bt->max_terms < n_terms || bt->tune.generation != tuning_snapshot().generation) {
        if (bt) vbm25_batch_destroy(bt);
        if (int rc = vbm25_batch_create(ix, std::max(nq, 16u), std::max(n_terms, 256u), k, &bt)) return rc;  // (the slot is empty then)
        bt->pinned_results = pinned_results;
    }
    *out = bt;
    return VBM25_OK;
}

static int vbm25_search_batch_impl(vbm25_index *ix, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq,
                       uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    if (!ix || !q_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (nq == 0) return k ? VBM25_OK : set_error(VBM25_ERR_INVALID, "number of needed rows is set to 0");
    vbm25_batch *bt = nullptr;
    if (int rc = scratch_batch(ix, &vbm25_index::scratch, true, nq, q_off, k, &bt)) return rc;
    const bool fast = !bt->bigk;
    int rc = vbm25_batch_set_queries_impl(bt, term_ids, q_off, nq, fast);
    if (!rc) rc = vbm25_batch_run_impl(bt, fast ? bt->lat_stream : nullptr);
    if (!rc) rc = vbm25_batch_fetch_impl(bt, hits, n_hits, fast);
    return rc;
}


// the shard's part of vbm25_multi_batch_fetch: wait for the part's stream, copy out (an item a one-launch route gave up is redone
// first: rerun_and_fetch)
int vbm25_batch_finish_download(vbm25_batch *bt, vbm25_hit *hits, uint32_t *n_hits) {
    return vbm25_batch_fetch_impl(bt, hits, n_hits, !bt->bigk && bt->lat_stream);
}


// selectors: n_sel of them (query q takes q_filter[q]); the batch's other queries take none
static int batch_set_filter_impl(vbm25_batch *bt, const vbm25_filter *f, const uint32_t *q_filter, uint32_t n_sel) {
    if (!bt) return set_error(VBM25_ERR_INVALID, "batch is NULL");
    if (f && f->index != bt->index) return set_error(VBM25_ERR_INVALID, "the filter belongs to another index");
    if (f && bt->growing) {
        if (!f->grow_serial)
            return set_error(VBM25_ERR_UNSUPPORTED, "the batch has a growing segment and the filter has no growing bitmaps");
        if (f->grow_serial != bt->growing->serial)
            return set_error(VBM25_ERR_INVALID, "the filter's growing bitmaps belong to another upload than the batch's growing segment");
        if (int rc = filter_growing_count_check(f, bt->growing)) return rc;
    }
    if (f && !q_filter && n_sel) return set_error(VBM25_ERR_INVALID, "q_filter is NULL");
    bool on = false;
    if (f)
        if (int rc = filter_selector_check(f, q_filter, n_sel, &on)) return rc;
    if (int rc = use_device(bt->device)) return rc;
    if (int rc = batch_quiesce(bt)) return rc;  // a run in flight reads the selectors to its end
    bt->filter = on ? f : nullptr;
    bt->filt_on = on;
    if (!on) return VBM25_OK;
    bt->h_filt_sel.assign(bt->max_queries, UINT32_MAX);
    std::copy(q_filter, q_filter + n_sel, bt->h_filt_sel.begin());
    if (!bt->filt_sel.p)
        if (int rc = bt->filt_sel.alloc(4ull * bt->max_queries)) return rc;
    HIP_TRY(hipMemcpy(bt->filt_sel.p, bt->h_filt_sel.data(), 4ull * bt->max_queries, hipMemcpyHostToDevice));
    return VBM25_OK;
}

static int vbm25_search_batch_filtered_impl(vbm25_index *ix, const vbm25_filter *f, const uint32_t *q_filter, const uint32_t *term_ids,
                                            const uint32_t *q_off, uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    if (!ix || !f || (!q_filter && nq) || !q_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (f->index != ix) return set_error(VBM25_ERR_INVALID, "the filter belongs to another index");
    if (int rc = filter_selector_check(f, q_filter, nq, nullptr)) return rc;
    if (nq == 0) return k ? VBM25_OK : set_error(VBM25_ERR_INVALID, "number of needed rows is set to 0");
    // vbm25_search_batch on the index's batch object with the filter set for this call only
    vbm25_batch *bt = nullptr;
    if (int rc = scratch_batch(ix, &vbm25_index::scratch, true, nq, q_off, k, &bt)) return rc;
    if (int rc = batch_set_filter_impl(bt, f, q_filter, nq)) return rc;
    const int rc = vbm25_search_batch_impl(ix, term_ids, q_off, nq, k, hits, n_hits);
    const int rc2 = batch_set_filter_impl(bt, nullptr, nullptr, 0);
    return rc ? rc : rc2;
}


// ---------------------------------------------------------------------------
// The growing segment (growing.h): uploaded once per change of the relation's unsealed documents, merged into the records of every
// run of a batch it is attached to.  The sealed route of such a batch is the one vbm25_batch_device_results forces (complete records
// on the device after the scan: no one-launch scan_win_kernel run that leaves a query to the fetch, no records written straight into
// pinned host memory); the growing kernels read a copy of those records and write the merged ones in their place, so a re-run merges
// from the new sealed records again.  On vbm25_stream_* and vbm25_multi_* (k <= 1024) the merged records go straight into the batch's
// pinned output instead and the sealed records are read where they lie, without the copy (growing_enqueue).
// ---------------------------------------------------------------------------
// lists of growing_scan_kernel: workgroups per query for nq queries (G_MAX_WG in all, at least one per query, at most one per tile)
static uint32_t growing_gq(uint32_t nq, uint32_t n_tiles) {
    return std::max(1u, std::min(std::max(1u, n_tiles), G_MAX_WG / std::max(nq, 1u)));
}

// (no run of the batch may be in flight)
int batch_grow_buffer(DeviceBuffer &b, size_t bytes) {
    if (b.p && b.bytes >= bytes) return VBM25_OK;
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr;
    return b.alloc(bytes);
}

// k > 1024: the accumulator, the sort's arrays and the iota for n_grow documents.  Sized when the segment is attached and again by
// the first run after an append has outgrown them (bt->gr_n).
static int batch_growing_bigk_scratch(vbm25_batch *bt, uint32_t n_grow) {
    const size_t n = std::max<size_t>(n_grow, 1);
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                                         (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n));
    const bool new_iota = !bt->gr_iota.p || bt->gr_iota.bytes < 4 * n;
    int rc = 0;
    if ((rc = batch_grow_buffer(bt->gr_acc, 8 * n)) || (rc = batch_grow_buffer(bt->gr_keys, 8 * n)) || (rc = batch_grow_buffer(bt->gr_iota, 4 * n)) ||
        (rc = batch_grow_buffer(bt->gr_docs, 4 * n)) || (rc = batch_grow_buffer(bt->gr_tmp, tb)))
        return rc;
    bt->gr_tmp_bytes = bt->gr_tmp.bytes;
    if (new_iota) {
        bigk_iota_kernel<<<1024, 256>>>(bt->gr_iota.as<uint32_t>(), uint32_t(bt->gr_iota.bytes / 4));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    bt->gr_n = std::max(bt->gr_n, uint32_t(n));
    return VBM25_OK;
}

// the buffers a batch needs to merge `gs` in (sized by the batch's shape, the k > 1024 scratch by n_grow): no run of the batch may be
// in flight.  Nothing is allocated once they fit.
int batch_growing_buffers(vbm25_batch *bt, const vbm25_device_growing *gs) {
    const size_t mq = bt->max_queries, k = bt->k;
    int rc = 0;
    if ((rc = batch_grow_buffer(bt->gr_sealed, sizeof(vbm25_hit) * mq * k)) || (rc = batch_grow_buffer(bt->gr_sealed_cnt, 4 * mq))) return rc;
    if (bt->bigk) return std::max(gs->n_grow, 1u) > bt->gr_n ? batch_growing_bigk_scratch(bt, gs->n_grow) : int(VBM25_OK);
    const size_t lists = 4ull * std::max<size_t>(G_MAX_WG, mq);  // (nq gq <= max(G_MAX_WG, nq): growing_gq)
    if ((rc = batch_grow_buffer(bt->gr_ls, 8 * lists * k)) || (rc = batch_grow_buffer(bt->gr_lg, 4 * lists * k)) ||
        (rc = batch_grow_buffer(bt->gr_lc, 4 * lists)))
        return rc;
    return VBM25_OK;
}

static int batch_set_growing_impl(vbm25_batch *bt, const vbm25_device_growing *gs) {
    if (!bt) return set_error(VBM25_ERR_INVALID, "batch is NULL");
    if (gs && gs->index != bt->index) return set_error(VBM25_ERR_INVALID, "the growing segment belongs to another index");
    if (gs && bt->filt_on) {
        if (!bt->filter->grow_serial)
            return set_error(VBM25_ERR_UNSUPPORTED, "the batch has a filter without growing bitmaps");
        if (bt->filter->grow_serial != gs->serial)
            return set_error(VBM25_ERR_INVALID, "the batch's filter has growing bitmaps of another upload than this segment");
        if (int rc = filter_growing_count_check(bt->filter, gs)) return rc;
    }
    if (int rc = use_device(bt->device)) return rc;
    if (int rc = batch_quiesce(bt)) return rc;  // a run in flight reads the segment and the buffers to its end
    bt->growing = nullptr;
    if (!gs) return VBM25_OK;
    if (int rc = batch_growing_buffers(bt, gs)) return rc;
    bt->growing = gs;
    return VBM25_OK;
}

// the growing segment's part of a run, on the run's stream behind the sealed scan
static int growing_enqueue(vbm25_batch *bt, hipStream_t st) {
    const vbm25_device_growing *gs = bt->growing;
    const uint32_t nq = bt->nq, k = bt->k;
    const DevGrowing G = gs->dev();
    // vbm25_stream_* and vbm25_multi_* (k <= 1024): growing_merge_kernel writes the final counts and records straight into the slot's
    // pinned output, as merge_kernel does without a segment -- no download command on the step.  The merged records then do not
    // replace the sealed ones, so the two device-to-device copies in front of the scan go too: the growing kernels read the sealed
    // route's records where its last kernel left them.
    const bool pinned = bt->pinned_results && !bt->bigk && bt->lat_stream && st == bt->lat_stream && bt->pin_out &&
                        bt->pin_out_bytes >= pin_out_records(nq) + sizeof(vbm25_hit) * size_t(nq) * k;
    const vbm25_hit *sealed = bt->hits.as<vbm25_hit>();
    const uint32_t *sealed_cnt = bt->n_hits.as<uint32_t>();
    if (!pinned) {
        HIP_TRY(hipMemcpyAsync(bt->gr_sealed.p, bt->hits.p, sizeof(vbm25_hit) * size_t(nq) * k, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(bt->gr_sealed_cnt.p, bt->n_hits.p, 4ull * nq, hipMemcpyDeviceToDevice, st));
        sealed = bt->gr_sealed.as<vbm25_hit>();
        sealed_cnt = bt->gr_sealed_cnt.as<uint32_t>();
    }
    if (bt->bigk) {
        const uint32_t n = std::max(gs->n_grow, 1u);
        for (uint32_t q = 0; q < nq; ++q) {
            HIP_TRY(hipMemsetAsync(bt->gr_acc.p, 0, 8ull * n, st));
            for (uint32_t p = bt->h_off[q]; p < bt->h_off[q + 1]; ++p) {
                const uint32_t t = bt->h_terms[p];
                if (t >= bt->index->n_terms) continue;
                const uint32_t p0 = gs->term_start_host[t], np = gs->term_start_host[t + 1] - p0;
                if (np) grow_accum_kernel<<<std::min<uint32_t>((np + 255) / 256, 4096u), 256, 0, st>>>(G.post_g, G.post_c, p0, np, bt->gr_acc.as<double>());
            }
            if (bt->filt_on && bt->h_filt_sel[q] != UINT32_MAX && gs->n_grow)
                bigk_mask_kernel<<<std::min<uint32_t>((gs->n_grow + 255) / 256, 4096u), 256, 0, st>>>(
                    bt->filter->grow_bits.as<unsigned long long>() + size_t(bt->h_filt_sel[q]) * bt->filter->grow_stride, gs->n_grow,
                    bt->gr_acc.as<double>());
            size_t tmp = bt->gr_tmp_bytes;
            HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(bt->gr_tmp.p, tmp, bt->gr_acc.as<unsigned long long>(),
                                                                  bt->gr_keys.as<unsigned long long>(), bt->gr_iota.as<uint32_t>(),
                                                                  bt->gr_docs.as<uint32_t>(), (int)n, 0, 64, st));
            growing_final_kernel<<<(k + 255) / 256, 256, 0, st>>>(sealed + size_t(q) * k, sealed_cnt + q, bt->gr_keys.as<unsigned long long>(),
                                                                  bt->gr_docs.as<uint32_t>(), gs->n_grow, k, G.payload,
                                                                  bt->hits.as<vbm25_hit>() + size_t(q) * k, bt->n_hits.as<uint32_t>() + q);
        }
        HIP_TRY(hipGetLastError());
        return VBM25_OK;
    }
    GrowArgs a{};
    a.term_ids = bt->term_ids.as<uint32_t>();
    a.q_off = bt->q_off.as<uint32_t>();
    if (bt->qin_live) {  // the staged descriptors (upload_staged), as vbm25_batch_run_impl reads them
        a.term_ids = reinterpret_cast<const uint32_t *>(bt->qin.as<uint8_t>());
        a.q_off = reinterpret_cast<const uint32_t *>(bt->qin.as<uint8_t>() + bt->plan.staged.off);
    }
    a.nq = nq;
    a.k = k;
    a.gq = growing_gq(nq, gs->n_tiles);
    a.sealed = sealed;
    a.sealed_cnt = sealed_cnt;
    a.ls = bt->gr_ls.as<double>();
    a.lg = bt->gr_lg.as<uint32_t>();
    a.lc = bt->gr_lc.as<uint32_t>();
    a.hits = bt->hits.as<vbm25_hit>();
    a.n_hits = bt->n_hits.as<uint32_t>();
    if (pinned) {
        a.n_hits = reinterpret_cast<uint32_t *>(bt->pin_out + 8);
        a.hits = reinterpret_cast<vbm25_hit *>(bt->pin_out + pin_out_records(nq));
    }
    if (bt->filt_on) {  // (batch_run_growing_impl checked that the growing bitmaps are this segment's)
        a.filt_words = bt->filter->grow_bits.as<uint32_t>();
        a.filt_sel = bt->filt_sel.as<uint32_t>();
        if (bt->plan.staged.sel) a.filt_sel = reinterpret_cast<const uint32_t *>(bt->qin.as<uint8_t>() + bt->plan.staged.sel);
        a.filt_stride = 2u * bt->filter->grow_stride;
    }
    (void)dispatch_k(k, [&](auto kmax) {
        constexpr int KM = decltype(kmax)::value;
        if (bt->filt_on) growing_scan_kernel<KM, true><<<nq * a.gq, GWG, 0, st>>>(G, a);
        else growing_scan_kernel<KM, false><<<nq * a.gq, GWG, 0, st>>>(G, a);
        growing_merge_kernel<KM><<<nq, 64, 0, st>>>(G, a);
        return int(VBM25_OK);
    });
    HIP_TRY(hipGetLastError());
    bt->results_pinned_now = pinned;  // (vbm25_batch_enqueue_download: only the flag is copied)
    return VBM25_OK;
}

int batch_run_growing_impl(vbm25_batch *bt, void *hip_stream) {
    // the filter's growing half may have been replaced since the batch took it: nothing is enqueued, the batch stays as it was
    if (bt->filt_on && bt->filter->grow_serial != bt->growing->serial)
        return set_error(VBM25_ERR_INVALID, "the batch's filter has no growing bitmaps of its growing segment (set again since)");
    if (bt->filt_on)
        if (int rc = filter_growing_count_check(bt->filter, bt->growing)) return rc;
    if (!bt->nq) return VBM25_OK;
    if (int rc = use_device(bt->index->device)) return rc;
    if (bt->bigk && std::max(bt->growing->n_grow, 1u) > bt->gr_n) {  // the segment was appended to since the batch took it
        if (int rc = batch_quiesce(bt)) return rc;
        if (int rc = batch_growing_bigk_scratch(bt, bt->growing->n_grow)) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (bt->plan.route == Route::OneLaunch && bt->plan.fused_pinned) {
        // the one-launch route's own pinned write would publish unmerged sealed records: with a segment attached it reads the queries
        // from the device block and leaves its records on the device, where the growing kernels find them
        if (int rc = upload_staged(bt, bt->plan.staged)) return rc;
        bt->plan.fused_pinned = false;
    }
    // timed: the sealed scan through the final merge (the sealed route's own events are off for the run)
    const bool timing = bt->timing;
    hipEvent_t e1;
    if (int rc = take_events(bt, st, e1)) return rc;
    bt->timing = false;
    int rc = vbm25_batch_run_impl(bt, hip_stream);
    bt->timing = timing;
    if (rc) return rc;
    if ((rc = growing_enqueue(bt, st))) return rc;
    if (timing) HIP_TRY(hipEventRecord(e1, st));
    return VBM25_OK;
}

static int vbm25_search_batch_growing_impl(vbm25_index *ix, const vbm25_device_growing *gs, const uint32_t *term_ids, const uint32_t *q_off,
                                           uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    if (!ix || !gs || !q_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (gs->index != ix) return set_error(VBM25_ERR_INVALID, "the growing segment belongs to another index");
    if (nq == 0) return k ? VBM25_OK : set_error(VBM25_ERR_INVALID, "number of needed rows is set to 0");
    vbm25_batch *bt = nullptr;
    if (int rc = scratch_batch(ix, &vbm25_index::scratch_grow, false, nq, q_off, k, &bt)) return rc;  // (segment and filter: this call only)
    int rc = batch_set_growing_impl(bt, gs);
    if (!rc) rc = vbm25_batch_set_queries_impl(bt, term_ids, q_off, nq);
    if (!rc) rc = batch_run_growing_impl(bt, nullptr);
    if (!rc) rc = vbm25_batch_fetch_impl(bt, hits, n_hits);
    const int rc2 = batch_set_growing_impl(bt, nullptr);
    return rc ? rc : rc2;
}


static int vbm25_search_batch_growing_filtered_impl(vbm25_index *ix, const vbm25_device_growing *gs, const vbm25_filter *f,
                                                    const uint32_t *q_filter, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq,
                                                    uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    if (!ix || !gs || !f || (!q_filter && nq) || !q_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (gs->index != ix) return set_error(VBM25_ERR_INVALID, "the growing segment belongs to another index");
    if (f->index != ix) return set_error(VBM25_ERR_INVALID, "the filter belongs to another index");
    if (int rc = filter_selector_check(f, q_filter, nq, nullptr)) return rc;
    if (nq == 0) return k ? VBM25_OK : set_error(VBM25_ERR_INVALID, "number of needed rows is set to 0");
    vbm25_batch *bt = nullptr;
    if (int rc = scratch_batch(ix, &vbm25_index::scratch_grow, false, nq, q_off, k, &bt)) return rc;  // (segment and filter: this call only)
    int rc = batch_set_growing_impl(bt, gs);
    if (!rc) rc = batch_set_filter_impl(bt, f, q_filter, nq);
    if (!rc) rc = vbm25_batch_set_queries_impl(bt, term_ids, q_off, nq);
    if (!rc) rc = batch_run_growing_impl(bt, nullptr);
    if (!rc) rc = vbm25_batch_fetch_impl(bt, hits, n_hits);
    const int rc2 = batch_set_filter_impl(bt, nullptr, nullptr, 0);
    const int rc3 = batch_set_growing_impl(bt, nullptr);
    return rc ? rc : rc2 ? rc2 : rc3;
}

}  // namespace vbm25

using namespace vbm25;

extern "C" {

void vbm25_batch_destroy(vbm25_batch *bt) {
    if (!bt) return;
    (void)hipSetDevice(bt->device);
    delete bt;
}

int vbm25_batch_device_results(vbm25_batch *bt, void **hits, void **n_hits) {
    if (!bt) return set_error(VBM25_ERR_INVALID, "batch is NULL");
    if (hits) *hits = bt->hits.p;
    if (n_hits) *n_hits = bt->n_hits.p;
    // (whoever reads the records on the device gets them complete after every run: the one-launch form of scan_win_kernel, which
    // leaves a query whose item it gave up to vbm25_batch_fetch, is not used for this batch object any more)
    bt->device_consumer = true;
    return VBM25_OK;
}

// tuning / test aid (not declared in include/vbm25.h): process-wide switches, read when a batch object is created.
// Names: dense_x1000, dense, ne, fused, ne_ratio, dense_items, range_items, range_min_chunk, range_grid, dense_grid, fused_items, arith,
// win, win_force, win_items, win_planes, win_guided, win_grid, win_skew, id16_max_blocks, dbg; cast_wave_max and cast_group_max (read
// at the start of each vbm25_documents_cast and vbm25_caster_submit); cast_pack and cast_grid (read at each vbm25_caster_submit); eval_grid (read at the start of each vbm25_documents_bind / vbm25_evaluate_documents
// and each scorer call); fwd_grid, fwd_wave_max and fwd_group_max (read at the start of each vbm25_index_bind); rerank_part and rerank_buf (read at the start of each scorer call); tid_grid (read at each launch of
// tid_match_kernel) and tid_dir (read at each vbm25_tid_set_create); live_sort_max (read at each vbm25_reranker_sync).
int vbm25_tuning_set(const char *name, long long value) {
    if (!name) return set_error(VBM25_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> guard(g_tune_mutex);
    const std::string n(name);
    if (n == "dense_x1000") g_tune.dense_x1000 = value;
    else if (n == "dense") g_tune.dense = value != 0;
    else if (n == "ne") g_tune.ne = value != 0;
    else if (n == "fused") g_tune.fused = value != 0;
    else if (n == "ne_ratio") g_tune.ne_ratio = (uint32_t)std::max(1ll, value);
    else if (n == "dense_items") g_tune.dense_items = (uint32_t)std::max(256ll, value);
    else if (n == "range_items") g_tune.range_items = (uint32_t)std::max(256ll, value);
    else if (n == "range_min_chunk") g_tune.range_min_chunk = (uint32_t)std::max(128ll, value);
    else if (n == "range_grid") g_tune.range_grid = (uint32_t)std::max(1ll, value);
    else if (n == "dense_grid") g_tune.dense_grid = (uint32_t)std::max(1ll, value);
#ifdef VBM25_DEV
    else if (n == "dbg") g_tune.dbg = (uint32_t)value;  // (scan_win_kernel's timing experiments: development build only)
#endif
    else if (n == "fused_items") g_tune.fused_items = (uint32_t)std::max(0ll, value);
    else if (n == "arith") g_tune.arith = value != 0;
    else if (n == "win") g_tune.win = value != 0;
    else if (n == "win_force") g_tune.win_force = value != 0;
    else if (n == "win_items") g_tune.win_items = (uint32_t)std::max(0ll, value);
    else if (n == "win_planes") g_tune.win_planes = value != 0;
    else if (n == "win_guided") g_tune.win_guided = value != 0;
    else if (n == "rel16_plane") g_tune.rel16_plane = value != 0;
    else if (n == "id16_plane") g_tune.id16_plane = value != 0;
    else if (n == "win_order_arith") g_tune.win_order_arith = value != 0;
    else if (n == "win_grid") g_tune.win_grid = (uint32_t)std::max(0ll, value);
    else if (n == "win_skew") g_tune.win_skew = value != 0;
    else if (n == "win_cut1") g_tune.win_cut1 = int(std::min<long long>(std::max<long long>(value, 1), 998));
    else if (n == "win_cut2") g_tune.win_cut2 = int(std::min<long long>(std::max<long long>(value, 2), 999));
    else if (n == "win_fuse") g_tune.win_fuse = value != 0;
    else if (n == "id16_max_blocks") g_tune.id16_max_blocks = (uint32_t)std::min<long long>(std::max(2ll, value), 0x00ffffffll);
    else if (n == "cast_wave_max" || n == "cast_group_max" || n == "cast_pack" || n == "cast_grid") {  // (the cast's class bounds and the caster's kernel choice and grid cap: cast.hip keeps and reads them)
        if (int rc = vbm25::cast_tuning_set(name, value)) return rc;
    }
    else if (n == "eval_grid") {  // (the grid cap of vbm25_documents_bind / vbm25_evaluate_documents: evaluate.hip keeps and reads it)
        if (int rc = vbm25::evaluate_tuning_set(value)) return rc;
    }
    else if (n == "fwd_grid" || n == "fwd_wave_max" || n == "fwd_group_max") {  // (the grid cap and the class bounds of vbm25_index_bind: forward.hip keeps and reads them)
        if (int rc = vbm25::forward_tuning_set(name, value)) return rc;
    }
    else if (n == "rerank_part" || n == "rerank_buf") {  // (the parts and the buffer of vbm25_scorer_topk: rerank.hip keeps and reads them)
        if (int rc = vbm25::rerank_tuning_set(name, value)) return rc;
    }
    else if (n == "tid_grid" || n == "tid_dir") {  // (the match kernel's grid cap and a TID set's directory size: tid.hip keeps and reads them)
        if (int rc = vbm25::tid_tuning_set(name, value)) return rc;
    }
    else if (n == "live_sort_max") {  // (where vbm25_reranker_sync changes from the LDS sort of a delta to the radix sort: live.hip keeps and reads it)
        if (int rc = vbm25::live_tuning_set(value)) return rc;
    }
    else return set_error(VBM25_ERR_INVALID, "unknown tuning switch %s", name);
    ++g_tune.generation;
    return VBM25_OK;
}
void vbm25_tuning_reset(void) {
    std::lock_guard<std::mutex> guard(g_tune_mutex);
    const uint32_t gen = g_tune.generation + 1u;
    g_tune = Tuning();
    g_tune.generation = gen;
    vbm25::cast_tuning_reset();
    vbm25::evaluate_tuning_reset();
    vbm25::forward_tuning_reset();
    vbm25::rerank_tuning_reset();
    vbm25::tid_tuning_reset();
    vbm25::live_tuning_reset();
}

// tuning / test aid (not declared in include/vbm25.h): work items of the last run and how many of them the
// first-choice kernel handed to scan_many_kernel
int vbm25_batch_debug_counts(vbm25_batch *bt, uint32_t *n_items, uint32_t *n_failed) {
    if (!bt || !n_items || !n_failed) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *n_items = *n_failed = 0;
    if (bt->bigk) return VBM25_OK;  // (the exhaustive route makes no work items: no n_items / item_failed buffers)
    if (int rc = use_device(bt->index->device)) return rc;
    HIP_TRY(hipStreamSynchronize(bt->last_stream));
    if (plan_free_kernels(bt) && bt->state_clean) {  // merge_kernel has cleaned the flags and kept the counts per query
        *n_items = bt->nq * bt->plan.g;
        std::vector<uint32_t> qf(bt->nq);
        if (bt->nq) HIP_TRY(hipMemcpy(qf.data(), bt->q_failed.p, 4ull * bt->nq, hipMemcpyDeviceToHost));
        *n_failed = 0;
        for (uint32_t x : qf) *n_failed += x;
        return VBM25_OK;
    }
    HIP_TRY(hipMemcpy(n_items, bt->n_items.p, 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> f(*n_items);
    if (*n_items) HIP_TRY(hipMemcpy(f.data(), bt->item_failed.p, 4ull * *n_items, hipMemcpyDeviceToHost));
    *n_failed = 0;
    for (uint32_t x : f) *n_failed += x != 0;
    return VBM25_OK;
}

// test aid (not declared in include/vbm25.h): the route the current queries take -- 0 general (plan_kernel), 1 one launch,
// 2 plan-free scan_range_kernel, 3 scan_win_kernel, 4 exhaustive k > 1024
int vbm25_batch_debug_route(vbm25_batch *bt) {
    if (!bt) return -1;
    return int(bt->bigk ? Route::Exhaustive : bt->plan.route);  // (a k > 1024 batch without queries too)
}

// test / bench aid (not declared in include/vbm25.h): which kernel the current queries' work goes to.  out[0..2] = queries the host
// classed sparse (scan_win_kernel / scan_range_kernel), dense (scan_dense_kernel: postings >= 0.1 n_docs), many-term (> 16 indexed
// terms: scan_many_kernel); out[3..5] = work items of the last run on the general route by the same classes (0 on the routes whose
// kernels make their items themselves: all of them are the sparse kernel's)
int vbm25_batch_debug_routes(vbm25_batch *bt, uint32_t *out6) {
    if (!bt || !out6) return set_error(VBM25_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 6; ++i) out6[i] = 0;
    if (bt->bigk) return VBM25_OK;
    if (int rc = use_device(bt->index->device)) return rc;
    HIP_TRY(hipStreamSynchronize(bt->last_stream));
    for (uint32_t q = 0; q < bt->nq; ++q) out6[bt->h_dense[q] ? 1 : 0]++;
    if (bt->plan.route == Route::General) {
        uint32_t n = 0;
        HIP_TRY(hipMemcpy(&n, bt->n_items.p, 4, hipMemcpyDeviceToHost));
        n = std::min(n, bt->max_items);
        std::vector<Item> items(n);
        if (n) HIP_TRY(hipMemcpy(items.data(), bt->items.p, sizeof(Item) * size_t(n), hipMemcpyDeviceToHost));
        for (const Item &it : items) {
            const uint32_t m = it.m & ~ITEM_DENSE;
            out6[3 + (m > 16u ? 2 : (it.m & ITEM_DENSE) ? 1 : 0)]++;
        }
    }
    return VBM25_OK;
}

// test aid (not declared in include/vbm25.h): launches of the last run's scan -- 1: scan_win_kernel merged the queries' lists itself
// (win_fuse), 3: scan_win_kernel, scan_many_kernel, merge_kernel (also after a one-launch run that marked a query), 0: another route
int vbm25_batch_debug_win_launches(vbm25_batch *bt) {
    if (!bt || bt->plan.route != Route::Window) return 0;
    return bt->win_fused_run ? 1 : 3;
}

// test aid (not declared in include/vbm25.h): how the last run of scan_win_kernel handed a query's lists to the merging wave -- 2: inside
// the workgroup, through the LDS (the one-launch form in the arithmetic layout of three items per query: every query but the last
// nq mod 4), 1: the one-launch form through memory, 0: merge_kernel merges, or another route.  The kernel decides the same from
// win_fuse, order_on and win_g (scan_win.h, the item end).
int vbm25_batch_debug_win_handover(vbm25_batch *bt) {
    if (!bt || bt->plan.route != Route::Window || !bt->win_fused_run) return 0;
    return bt->win_order_on == 2u && bt->plan.g == 3u && bt->nq >= 4u ? 2 : 1;
}

// -DVBM25_CHECK builds (not declared in include/vbm25.h): the first violated assertion of the scan kernels, then reset.
// out[0] = check code (0: none), out[1] = offending value, out[2] = work item, out[3] = thread
int vbm25_batch_debug_check(vbm25_batch *bt, uint32_t *out4) {  // out4: 16 words
    if (!bt || !out4) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = use_device(bt->index->device)) return rc;
    HIP_TRY(hipStreamSynchronize(bt->last_stream));
    if (!bt->dbg.p) {
        std::memset(out4, 0, 64);
        return VBM25_OK;
    }
    HIP_TRY(hipMemcpy(out4, bt->dbg.p, 64, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(bt->dbg.p, 0, 64));
    return VBM25_OK;
}

// test aid (not declared in include/vbm25.h): the per-query thresholds the last run ended with (bits of a lower bound of
// each query's k-th best score; the merge drops list entries below them)
int vbm25_batch_debug_theta(vbm25_batch *bt, unsigned long long *out) {
    if (!bt || !out) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = use_device(bt->index->device)) return rc;
    HIP_TRY(hipStreamSynchronize(bt->last_stream));
    if (bt->nq && bt->theta.p)
        HIP_TRY(hipMemcpy(out, plan_free_kernels(bt) && bt->state_clean ? bt->theta_last.p : bt->theta.p, 8ull * bt->nq, hipMemcpyDeviceToHost));
    return VBM25_OK;
}

// test aid (not declared in include/vbm25.h): what merge_kernel read of query q after a run on the general route (the only route that
// keeps the lists: the others' merges clean them, and this entry refuses them) -- per list of the query's items, in merge_kernel's
// order, cnt[l] = min(res_cnt, k), the entries it loads, and surv[l] = those of them at or above the query's threshold, the ones it
// ranks.  *n_lists = the query's lists (items x lists per item); more than cap of them is an error.
int vbm25_batch_debug_lists(vbm25_batch *bt, uint32_t q, uint32_t *cnt, uint32_t *surv, uint32_t cap, uint32_t *n_lists) {
    if (!bt || !cnt || !surv || !n_lists) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *n_lists = 0;
    if (bt->bigk || bt->plan.route != Route::General) return set_error(VBM25_ERR_INVALID, "the lists are kept on the general route only");
    if (q >= bt->nq) return set_error(VBM25_ERR_INVALID, "query %u of %u", q, bt->nq);
    if (int rc = use_device(bt->index->device)) return rc;
    HIP_TRY(hipStreamSynchronize(bt->last_stream));
    uint32_t base[2] = {0, 0};
    unsigned long long theta = 0;
    HIP_TRY(hipMemcpy(base, bt->q_item_base.as<uint32_t>() + q, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&theta, bt->theta.as<unsigned long long>() + q, 8, hipMemcpyDeviceToHost));
    if (base[1] < base[0] || base[1] > bt->max_items) return set_error(VBM25_ERR_DEVICE, "query %u: items %u .. %u", q, base[0], base[1]);
    const size_t L0 = size_t(base[0]) * bt->lpi, NL = size_t(base[1] - base[0]) * bt->lpi;
    if (NL > cap) return set_error(VBM25_ERR_INVALID, "query %u has %zu lists, the caller's arrays hold %u", q, NL, cap);
    *n_lists = uint32_t(NL);
    if (!NL) return VBM25_OK;
    std::vector<uint32_t> rc(NL);
    std::vector<unsigned long long> sc(NL * bt->k);  // (the query's lists lie side by side: one copy)
    HIP_TRY(hipMemcpy(rc.data(), bt->res_cnt.as<uint32_t>() + L0, 4 * NL, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sc.data(), bt->res_score.as<double>() + L0 * bt->k, 8 * NL * bt->k, hipMemcpyDeviceToHost));
    for (size_t l = 0; l < NL; ++l) {
        cnt[l] = std::min(rc[l], bt->k);
        surv[l] = 0;
        for (uint32_t i = 0; i < cnt[l]; ++i) surv[l] += sc[l * bt->k + i] >= theta;
    }
    return VBM25_OK;
}

int vbm25_batch_set_timing(vbm25_batch *bt, int enabled) {
    if (!bt) return set_error(VBM25_ERR_INVALID, "batch is NULL");
    bt->timing = enabled != 0;
    bt->events_used = 0;
    return VBM25_OK;
}

int vbm25_batch_kernel_ms(vbm25_batch *bt, double *avg_ms, uint32_t *n_launches) {
    if (!bt || !avg_ms) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = use_device(bt->index->device)) return rc;
    double sum = 0;
    for (size_t i = 0; i < bt->events_used; ++i) {
        HIP_TRY(hipEventSynchronize(bt->events[i].second));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, bt->events[i].first, bt->events[i].second));
        sum += ms;
    }
    *avg_ms = bt->events_used ? sum / double(bt->events_used) : 0.0;
    if (n_launches) *n_launches = uint32_t(bt->events_used);
    bt->events_used = 0;
    return VBM25_OK;
}

#ifdef VBM25_PROFILE
// profiling builds only (not declared in include/vbm25.h): copy out the phase counters
int vbm25_batch_profile(vbm25_batch *bt, unsigned long long *out, uint32_t n_workgroups) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, bt->prof.p, 8ull * 16 * RNW * std::min<uint32_t>(n_workgroups, R_GRID), hipMemcpyDeviceToHost));
    return VBM25_OK;
}
#endif

int vbm25_batch_create(vbm25_index *ix, uint32_t max_queries, uint32_t max_total_terms, uint32_t k,
                       vbm25_batch **out) {
    return guarded([&] { return vbm25_batch_create_impl(ix, max_queries, max_total_terms, k, out); });
}

int vbm25_batch_set_queries(vbm25_batch *bt, const uint32_t *term_ids, const uint32_t *q_off,
                            uint32_t nq) {
    return guarded([&] { return vbm25_batch_set_queries_impl(bt, term_ids, q_off, nq); });
}

int vbm25_batch_run(vbm25_batch *bt, void *hip_stream) {
    return guarded([&] { return bt && bt->growing ? batch_run_growing_impl(bt, hip_stream) : vbm25_batch_run_impl(bt, hip_stream); });
}

int vbm25_batch_fetch(vbm25_batch *bt, vbm25_hit *hits, uint32_t *n_hits) {
    return guarded([&] { return vbm25_batch_fetch_impl(bt, hits, n_hits); });
}

int vbm25_search_batch(vbm25_index *ix, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq,
                       uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    return guarded([&] { return vbm25_search_batch_impl(ix, term_ids, q_off, nq, k, hits, n_hits); });
}

int vbm25_batch_set_filter(vbm25_batch *bt, const vbm25_filter *f, const uint32_t *q_filter) {
    return guarded([&] { return batch_set_filter_impl(bt, f, q_filter, bt && f ? bt->max_queries : 0u); });
}
int vbm25_search_batch_filtered(vbm25_index *ix, const vbm25_filter *f, const uint32_t *q_filter, const uint32_t *term_ids,
                                const uint32_t *q_off, uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    return guarded([&] { return vbm25_search_batch_filtered_impl(ix, f, q_filter, term_ids, q_off, nq, k, hits, n_hits); });
}
int vbm25_search_batch_growing_filtered(vbm25_index *ix, const vbm25_device_growing *gs, const vbm25_filter *f, const uint32_t *q_filter,
                                        const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, uint32_t k, vbm25_hit *hits,
                                        uint32_t *n_hits) {
    return guarded([&] {
        return vbm25_search_batch_growing_filtered_impl(ix, gs, f, q_filter, term_ids, q_off, nq, k, hits, n_hits);
    });
}
int vbm25_search_batch_growing(vbm25_index *ix, const vbm25_device_growing *gs, const uint32_t *term_ids, const uint32_t *q_off,
                               uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    return guarded([&] { return vbm25_search_batch_growing_impl(ix, gs, term_ids, q_off, nq, k, hits, n_hits); });
}
int vbm25_batch_set_growing(vbm25_batch *bt, const vbm25_device_growing *gs) {
    return guarded([&] { return batch_set_growing_impl(bt, gs); });
}

}  // extern "C"
