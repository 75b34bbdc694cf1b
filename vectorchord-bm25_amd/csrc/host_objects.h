// host_objects.h -- the host objects behind the handles of include/vbm25.h, defined once: the index, the filter, the device growing
// segment and the batch, with the tuning switches, the route and the staging layout a batch keeps, and the declarations of the functions
// one unit calls in another.  Included by index.hip, search.hip, growing.hip, filter.hip, stream.hip, multi.hip, tid.hip and forward.hip.  Not part of the ABI.
// The layouts do not depend on VBM25_PROFILE, VBM25_DEV or VBM25_CHECK: a unit built with one of them links with the others built without.
#ifndef VBM25_HOST_OBJECTS_H
#define VBM25_HOST_OBJECTS_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "vbm25_internal.h"
#include "hip_host.h"
#include "device_types.h"

namespace vbm25 {

// An HbmArray whose alloc and upload return the library's codes and set the error text, for the `(rc = a.alloc(..)) || (rc = b.upload(..))`
// chains of the units.  Nothing of its own to own: storage and destructor are HbmArray's.
struct DeviceBuffer : HbmArray {
    int alloc(size_t n) {  // (HbmArray::alloc, spelled out: a failure's text goes on naming hipMalloc and its size)
        bytes = n;
        HIP_TRY(hipMalloc(&p, n ? n : 16));
        return VBM25_OK;
    }
    int upload(const void *src, size_t n) {
        if (int rc = alloc(n)) return rc;
        if (n) HIP_TRY(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
        return VBM25_OK;
    }
};

// Tuning / test switches (not part of the ABI of include/vbm25.h; set through vbm25_tuning_set by tools and tests, read when a
// batch object is created).  No entry point of the library reads the environment.
struct Tuning {
    long long dense_x1000 = 100;   // a query with this many postings per 1000 documents is dense (0: every query)
    int dense = 1;                 // dense queries take scan_dense_kernel (0: the exhaustive scan_many_kernel)
    int ne = 1;                    // MaxScore split (non-essential lists looked up, not scanned)
    int fused = 1;                 // one-launch route for a handful of sparse queries
    uint32_t ne_ratio = 2;
    uint32_t dense_items = D_TARGET_ITEMS;
    uint32_t range_items = R_TARGET_ITEMS, range_min_chunk = R_MIN_CHUNK_POSTINGS;
    uint32_t range_grid = R_GRID, dense_grid = D_GRID;
    uint32_t dbg = 0;              // timing experiments of scan_win_kernel only (wrong results)
    uint32_t fused_items = 128;    // the one-launch route takes batches of up to this many work items
    int arith = 1;                 // batches of sparse queries beyond that: work items made by the scan kernel (no plan_kernel)
    int win = 1;                   // batches of sparse queries of <= 8 comparable terms, k <= 64: scan_win_kernel (the window formulation)
    int win_force = 0;             // tests: that route whatever the lists' lengths
    uint32_t win_items = 0;        // work items of a batch on that route (0: twice the resident waves)
    int win_planes = 1;            // read at index creation: derive the window planes (post_id16, win_off)
    int rel16_plane = 1;           // read at index creation: derive post_rel16 (0: the kernels decode the blob's delta streams themselves)
    int id16_plane = 1;            // read at index creation: derive post_id16 (0: the window tables only -- decode_id16_kernel unpacks the batch's
                                   // terms from the blob into the batch's scratch plane ahead of every scan_win_kernel launch)
    int win_guided = 0;            // scan_win_kernel's items of a query of decreasing length, handed out longest first (0: equal runs; measured
                                   // no better on C3 -- an item's setup costs more than the shorter tail saves)
    uint32_t win_grid = 0;         // its persistent workgroups (0: one per CU)
    int win_fuse = 1;              // scan_win_kernel merges the queries' lists itself: the batched route is one launch (0: scan_many_kernel and merge_kernel behind it)
    int win_cut1 = 392, win_cut2 = 730;  // ... where a query's three runs are cut, in thousandths of its windows (round 6, tools/skew_sweep.sh: 59 / 52 / 42 of C3's 153)
    int win_order_arith = 1;       // the skewed layout computed in the kernel when the queries keep their order (0: always the host's table)
    int win_skew = 1;              // one item per wave: a query's three runs of windows sized for the three kinds of waves of a SIMD
    uint32_t id16_max_blocks = 0x00ffffff;  // an index without post_id16: the most 256-byte blocks of a batch's terms its scratch plane takes
                                   // (a larger batch takes scan_range_kernel; tests lower it to cross the limit on a small corpus)
    uint32_t generation = 0;       // bumped by every vbm25_tuning_set / reset: vbm25_search_batch's batch object is rebuilt when it is stale
};
// the switches of the moment (search.hip owns them and their lock: vbm25_tuning_set / _reset write, this copies)
Tuning tuning_snapshot();

// The route a query set takes (the numbers are what vbm25_batch_debug_route returns)
enum class Route {
    General = 0,     // plan_kernel, the scan kernels, merge_kernel
    OneLaunch = 1,   // a handful of sparse queries: scan_range_kernel plans, scans and merges
    PlanFree = 2,    // every query sparse: scan_range_kernel makes the work items itself, merge_kernel cleans
    Window = 3,      // every query sparse, <= 8 terms of comparable length: scan_win_kernel
    Exhaustive = 4,  // k > 1024: one query at a time over a dense accumulator
};

// The staged descriptors, one block in pinned memory (pin_in) and on the device (qin): term ids at 0, then the byte offsets of the
// query offsets, the dense flags (padded to 8), the host's item order, the id16 block starts and the filter selectors (stage_sel), and
// the end of the block
struct StagedLayout {
    size_t off = 0, dense = 0, order = 0, id16 = 0, end = 0;
    size_t sel = 0;  // the filter selectors of a staged filtered query set (nq words in front of `end`), 0: none staged
};
inline StagedLayout staged_layout(uint32_t nq, uint32_t n_term_pos, size_t n_order, bool id16) {
    StagedLayout L;
    L.off = 4ull * n_term_pos;
    L.dense = L.off + 4ull * (nq + 1);
    L.order = L.dense + ((size_t(nq) + 7) & ~size_t(7));
    L.id16 = L.order + 4 * n_order;
    L.end = L.id16 + (id16 ? 4ull * n_term_pos : 0);
    return L;
}

// The pinned output block (pin_out): the error flag at 0, the counts at 8, the records at the first 8-byte boundary behind them
inline size_t pin_out_records(uint32_t nq) { return 8 + ((4ull * nq + 7) & ~size_t(7)); }

// What set_queries decided for the current query set.  A batch without queries holds QueryPlan{}.
struct QueryPlan {
    Route route = Route::General;
    uint32_t g = 0;               // OneLaunch, PlanFree, Window: work items per query (Window: runs of 2^16-document windows)
    uint32_t win_len = 0;         // Window: a query's runs are win_len windows each and a shorter rest (0: equal runs)
    bool win_skew = false;        // ... one item per wave, a query's three runs sized for the three kinds of waves of a SIMD
    bool order_identity = false;  // ... the queries keep the caller's order in the host's item order (no sort by length)
    bool order_useful = true;     // ... the queries differ enough in length for the longest-first order to matter
    uint32_t q_stride = 0;        // != 0: every query has this many terms
    uint32_t range_mt = 0;        // the most indexed terms of a sparse query of <= 16 (0: none, or k > REG_K)
    bool has_dense = false;       // some query takes scan_dense_kernel
    bool need_many = true;        // some query has items for scan_many_kernel (more than 16 terms, 256 < k, dense without the dense kernel)
    uint32_t dense_c = 0;         // items per dense query (0: chunks by postings, as the other queries)
    uint32_t range_grid = R_GRID, dense_grid = D_GRID;
    bool id16_decode = false;     // Window on an index without post_id16: the terms' ids go through the batch's scratch plane
    uint64_t id16_blocks = 0;     // ... its 256-byte blocks the terms need
    bool fused_pinned = false;    // OneLaunch with queries and hits in pinned host memory (vbm25_search_batch, <= 8 queries)
    uint32_t n_term_pos = 0;      // term positions (q_off[nq])
    StagedLayout staged;
    uint32_t range_rt() const { return range_mt == 0 ? 0u : range_mt <= 8u ? 8u : 16u; }  // scan_range_kernel's row stride
};

}  // namespace vbm25

struct vbm25_index {
    int device = 0;
    vbm25::DevIndex dev{};
    uint32_t n_docs = 0, n_terms = 0, n_blocks = 0;  // n_docs == 0: empty sealed segment, every search returns no hit
    std::vector<uint8_t> term_key;  // host copy for vbm25_lookup_terms
    std::vector<uint32_t> term_df_host;  // host copy for query routing
    vbm25_batch *scratch = nullptr;      // batch object re-used by vbm25_search_batch
    vbm25_batch *scratch_grow = nullptr; // ... and by vbm25_search_batch_growing
    vbm25::DeviceBuffer term_wand_tf, term_wand_fn, term_df, term_first_block, term_s0, blk_min_doc, blk_max_doc, blk_meta, blk_ub, blob,
        post_fn, post_rel16, post_tfn, doc_payload, s1, term_idf, fn_len, term_kth_ub, post_id16, win_off, term_win;
    std::vector<uint32_t> term_win_host;  // host copy of term_win (query routing); empty: the index has no window planes
    uint32_t n_win = 0;
    double k1 = 1.2, b = 0.75;
    uint64_t device_bytes = 0;
};

// F bitmaps over the documents of one index, in HBM on its device (vbm25_filter_create), and optionally F bitmaps over the documents
// of one uploaded growing segment (vbm25_filter_set_growing), named by the upload's serial number -- no pointer into the segment
struct vbm25_filter {
    const vbm25_index *index = nullptr;
    int device = 0;
    uint32_t n_bitmaps = 0;
    uint32_t words = 0;  // per bitmap: ceil(n_docs / 64)
    vbm25::DeviceBuffer bits;   // n_bitmaps x words
    uint64_t grow_serial = 0;  // the growing bitmaps' segment (vbm25_device_growing::serial), 0: none
    uint32_t grow_n = 0;       // ... its n_grow
    uint32_t grow_words = 0;   // per growing bitmap: ceil(grow_n / 64)
    // ... its capacity in words, >= grow_words: bitmap i starts at word i grow_stride (vbm25_filter_set_growing sizes it exactly,
    // vbm25_filter_extend_growing grows it geometrically).  Every bit at or beyond grow_n is zero, up to the capacity.
    uint32_t grow_stride = 0;
    vbm25::DeviceBuffer grow_bits;    // n_bitmaps x grow_stride
    vbm25::DeviceBuffer grow_stage;   // vbm25_filter_extend_growing: the delta words of one call
};

// The growing segment of one index in HBM on its device (vbm25_growing_upload; growing.h has the layout)
struct vbm25_device_growing {
    const vbm25_index *index = nullptr;
    int device = 0;
    uint64_t serial = 0;  // per upload, from a process-wide counter (never 0): a re-upload at the same address is another segment
    uint32_t n_grow = 0, n_tiles = 0, n_post = 0;
    vbm25::DeviceBuffer term_start, post_g, post_c, tab_idx, tab, payload;
    std::vector<uint32_t> term_start_host;  // (k > 1024: one accumulation launch per term)
    uint64_t device_bytes = 0;
    // vbm25_device_growing_append / _delete (growing_append.h).  An append writes the spare arrays and swaps them in at its end; the
    // postings, the payloads and the tables are buffers with room to spare (their `bytes` is the capacity, grown geometrically).
    vbm25::DeviceBuffer term_start2, post_g2, post_c2, tab_idx2, tab2;
    vbm25::DeviceBuffer term_key;  // the index's keys (from the first append on)
    vbm25::DeviceBuffer stage;     // the delta and the scratch of one call
    void count_bytes() {    // everything allocated, the room to spare included
        device_bytes = 0;
        for (const vbm25::DeviceBuffer *b : {&term_start, &post_g, &post_c, &tab_idx, &tab, &payload, &term_start2, &post_g2, &post_c2, &tab_idx2,
                                      &tab2, &term_key, &stage})
            if (b->p) device_bytes += b->bytes;
    }
    vbm25::DevGrowing dev() const {
        vbm25::DevGrowing g{};
        g.term_start = term_start.as<uint32_t>();
        g.post_g = post_g.as<uint32_t>();
        g.post_c = post_c.as<double>();
        g.tab_idx = tab_idx.as<uint32_t>();
        g.tab = tab.as<uint32_t>();
        g.payload = payload.as<uint16_t>();
        g.n_grow = n_grow;
        g.n_tiles = n_tiles;
        g.n_terms = index->n_terms;
        return g;
    }
};

struct vbm25_batch {
    vbm25_index *index = nullptr;
    int device = 0;  // the index's device ordinal: the batch can be destroyed after its index
    uint32_t max_queries = 0, max_terms = 0, k = 0, nq = 0, max_items = 0;
    vbm25::DeviceBuffer term_ids, q_off, items, n_items, q_item_base, theta, res_score, res_doc, res_cnt,
        hits, n_hits, error_flag, prof, q_dense, item_failed, item_order, work_ctr, hist, fused_state, dbg, fail_any, q_failed, theta_last;
    bool bigk = false;            // k > 1024: exhaustive path, one query at a time
    vbm25::DeviceBuffer bk_acc, bk_keys, bk_iota, bk_docs, bk_tmp;
    size_t bk_tmp_bytes = 0;
    std::vector<uint32_t> h_terms, h_off;  // host copy of the queries (bigk launches per term)
    // filtered search (vbm25_batch_set_filter): the filter and per query the bitmap it takes (max_queries selectors, on the device and,
    // for the k > 1024 path, on the host); filt_on: some selector names a bitmap (else the kernels see no filter at all)
    const vbm25_filter *filter = nullptr;
    vbm25::DeviceBuffer filt_sel;
    std::vector<uint32_t> h_filt_sel;
    bool filt_on = false;
    // vbm25_stream_* / vbm25_multi_*: the selectors of the query set being set (nq of them, host memory, for the duration of
    // set_queries): they go up in the staged block (StagedLayout::sel), not through filt_sel
    const uint32_t *stage_sel = nullptr;
    // growing segment (vbm25_batch_set_growing): merged into the records by every run (growing.h).  gr_*: the sealed records' copy,
    // the per-workgroup lists of growing_scan_kernel (k <= 1024) or the dense accumulator and its sort (k > 1024)
    const vbm25_device_growing *growing = nullptr;
    vbm25::DeviceBuffer gr_sealed, gr_sealed_cnt, gr_ls, gr_lg, gr_lc, gr_acc, gr_keys, gr_iota, gr_docs, gr_tmp;
    size_t gr_tmp_bytes = 0;
    uint32_t gr_n = 0;  // growing documents the k > 1024 scratch holds
    std::vector<uint8_t> h_dense;          // per query: dense (scratch of set_queries, sized once)
    std::vector<unsigned long long> h_postings;
    std::vector<uint32_t> h_order, h_order_q;  // set_queries: the longest-first item order of the routes without plan_kernel
    vbm25::Tuning tune;                  // the switches of the moment the batch was created
    bool timing = false;
    bool use_range = false;       // k <= REG_K: sparse queries of <= 16 terms take scan_range_kernel, dense ones scan_dense_kernel
    uint32_t lpi = 1;             // result lists per work item
    bool use_dense = false;       // dense queries of <= D_T terms take scan_dense_kernel
    vbm25::QueryPlan plan;               // the current queries' route (set_queries)
    // an index without the post_id16 plane: the batch's scratch plane (the low 16 bits of the ids of the current queries' terms, made by
    // decode_id16_kernel ahead of every scan_win_kernel launch) and, per term position, the term's first 256-byte block in it
    vbm25::DeviceBuffer id16_tmp, id16_fb;
    std::vector<uint32_t> h_id16_fb;
    vbm25::DeviceBuffer qin;             // the staged descriptors on the device (StagedLayout)
    bool qin_live = false;        // ... hold the current queries (set by upload_staged; a plain set_queries fills the separate buffers)
    bool device_consumer = false; // vbm25_batch_device_results was called: every run leaves complete records on the device
    bool win_nofuse = false;      // the last run's in-kernel merge marked a query (an item was given up): this query set runs with scan_many_kernel and merge_kernel
    bool win_fused_run = false;   // the last run was a one-launch run of scan_win_kernel (a count of NONE32 means: re-run, see rerun_and_fetch)
    uint32_t win_order_on = 0;    // ... and the item order it ran with (DevBatch::order_on; 2: a workgroup holds all three items of its four queries)
    bool state_clean = false;     // threshold / histogram / counters are zero (the routes without plan_kernel leave them so; the general one does not)
    uint32_t target_items = vbm25::TARGET_ITEMS;
    uint32_t min_chunk = vbm25::MIN_CHUNK_POSTINGS;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
    // vbm25_search_batch's low-latency route: pinned staging buffers and a private stream -- queries go up and
    // hits come down with asynchronous copies and ONE stream synchronisation
    hipStream_t lat_stream = nullptr;
    hipStream_t last_stream = nullptr;  // the stream of the last run: what fetch waits for (not the whole device)
    bool download_enqueued = false;     // the last run's records are already on their way to pin_out (vbm25_multi_batch_run)
    // vbm25_stream_*: merge_kernel writes counts and records straight into the pinned output buffer (posted writes over PCIe, no
    // download command on the step: only the 4-byte flag is copied); results_pinned_now: the last run did so.  With a growing segment
    // attached the sealed route writes device records and growing_merge_kernel the pinned ones (growing_enqueue).
    bool pinned_results = false, results_pinned_now = false;
    uint8_t *pin_in = nullptr, *pin_out = nullptr;
    size_t pin_in_bytes = 0, pin_out_bytes = 0;
    ~vbm25_batch() {
        if (lat_stream) (void)hipStreamDestroy(lat_stream);
        if (pin_in) (void)hipHostFree(pin_in);
        if (pin_out) (void)hipHostFree(pin_out);
        for (auto &e : events) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    }
};

namespace vbm25 {

// a run of the batch in flight reads its buffers, its selectors and its growing segment to its end: wait for it
inline int batch_quiesce(vbm25_batch *bt) {
    if (bt->lat_stream) HIP_TRY(hipStreamSynchronize(bt->lat_stream));
    HIP_TRY(hipStreamSynchronize(bt->last_stream));
    return VBM25_OK;
}

// index.hip
int clone_index(const vbm25_index *src, int device, vbm25_index **out);  // a replica on another device, copied GPU to GPU
// search.hip: the batch.  `fast`: staged in pinned memory and copied on the batch's own stream
int vbm25_batch_set_queries_impl(vbm25_batch *bt, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, bool fast = false);
void batch_clear_queries(vbm25_batch *bt);
int vbm25_batch_run_impl(vbm25_batch *bt, void *hip_stream);
int batch_run_growing_impl(vbm25_batch *bt, void *hip_stream);
int vbm25_batch_fetch_impl(vbm25_batch *bt, vbm25_hit *hits, uint32_t *n_hits, bool fast = false);
int vbm25_batch_enqueue_download(vbm25_batch *bt);
int vbm25_batch_finish_download(vbm25_batch *bt, vbm25_hit *hits, uint32_t *n_hits);
int batch_grow_buffer(DeviceBuffer &b, size_t bytes);
int batch_growing_buffers(vbm25_batch *bt, const vbm25_device_growing *gs);
// growing.hip: grow_delete_kernel over a deletion bitmap in HBM (tid.hip makes one from a TID set)
int growing_delete_by_bits(vbm25_device_growing *gs, const uint32_t *bits);
// filter.hip
int filter_growing_count_check(const vbm25_filter *f, const vbm25_device_growing *gs);
int filter_selector_check(const vbm25_filter *f, const uint32_t *sel, uint32_t n, bool *any);
// stream.hip: what a ring slot and a multi-device shard have in common
int batch_attach_check(const vbm25_batch *b, const vbm25_device_growing *gs, const vbm25_filter *f, const uint32_t *sel, uint32_t nq,
                       bool *on_out);
int batch_attach(vbm25_batch *b, const vbm25_device_growing *gs, const vbm25_filter *f, const uint32_t *sel, uint32_t nq, bool on);

}  // namespace vbm25

#endif
