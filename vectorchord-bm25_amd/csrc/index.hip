// index.hip -- vbm25_index: creation from a flattened sealed segment on the host or in HBM (the derive kernels of index_derive.h),
// the replica of an index on another device, the compaction's view of it (maintain.hip does the work), vbm25_lookup_terms, what
// resolve.hip, evaluate.hip and pages_device.hip read of an index (vbm25_internal.h), and vbm25_evaluate_batch.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "host_objects.h"
#include "index_derive.h"

namespace vbm25 {

// ---------------------------------------------------------------------------
// Batched `<&>`: bm25::evaluate (evaluate.rs:22-74) for many documents against one query -- the seq-scan
// form of the operator (src/index/operators.rs:22-55).  One thread per document: a merge of the document's
// elements with the query's terms, both ascending; result = sum of idf * tf in query key order.  idf comes
// from the host (libm log, bm25.rs:285-289), tf() is bm25.rs:291-295 with the index's s1 table (the same
// expression), the fieldnorm of the document is length_to_fieldnorm of its saturating sum of tfs.
// ---------------------------------------------------------------------------
struct EvalArgs {
    uint32_t n_docs, n_q, n_terms;
    const uint32_t *q_terms;     // ascending term ids; ids >= n_terms (unknown tokens) are skipped
    const uint64_t *doc_start;   // n_docs + 1
    const uint32_t *doc_term;    // per element: term id, NONE32 when the key is not in the index
    const uint32_t *doc_tf;
    const double *term_idf, *s1;
    const uint32_t *fn_len;      // FIELDNORM_TO_LENGTH, 256 entries
    double k1p1;
    double *out;
};
__global__ void __launch_bounds__(256) evaluate_kernel(EvalArgs a) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.n_docs) return;
    const uint64_t e0 = a.doc_start[d], e1 = a.doc_start[d + 1];
    unsigned long long length = 0;  // Document::length, vector.rs:77-83: saturating
    for (uint64_t e = e0; e < e1; ++e) {
        length += a.doc_tf[e];
        if (length > 0xffffffffull) length = 0xffffffffull;
    }
    uint32_t lo = 0, hi = 256;  // length_to_fieldnorm, bm25.rs:278-283: last entry <= length
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.fn_len[mid] <= (uint32_t)length) lo = mid; else hi = mid;
    }
    const double s1 = a.s1[lo];
    uint64_t cur = e0;
    double result = 0.0;
    for (uint32_t i = 0; i < a.n_q; ++i) {
        const uint32_t qt = a.q_terms[i];
        if (qt >= a.n_terms) continue;
        while (cur < e1 && (a.doc_term[cur] >= a.n_terms || a.doc_term[cur] < qt)) ++cur;
        if (!(cur < e1 && a.doc_term[cur] == qt)) continue;
        const double tf = (double)a.doc_tf[cur];
        const double tfv = (tf * a.k1p1) / (tf + s1);
        result += a.term_idf[qt] * tfv;
    }
    a.out[d] = result;
}

// every device array of an index (vbm25_multi_create copies them from GPU to GPU)
static DeviceBuffer vbm25_index::*const INDEX_BUFFERS[] = {
    &vbm25_index::term_wand_tf, &vbm25_index::term_wand_fn, &vbm25_index::term_df, &vbm25_index::term_first_block, &vbm25_index::term_s0,
    &vbm25_index::blk_min_doc, &vbm25_index::blk_max_doc, &vbm25_index::blk_meta, &vbm25_index::blk_ub, &vbm25_index::blob,
    &vbm25_index::post_fn, &vbm25_index::post_rel16, &vbm25_index::post_tfn, &vbm25_index::doc_payload, &vbm25_index::s1,
    &vbm25_index::term_idf, &vbm25_index::fn_len, &vbm25_index::term_kth_ub,
    &vbm25_index::post_id16, &vbm25_index::win_off, &vbm25_index::term_win};

static void fill_dev(vbm25_index *ix) {
    ix->dev.n_docs = ix->n_docs;
    ix->dev.n_terms = ix->n_terms;
    ix->dev.n_blocks = ix->n_blocks;
    ix->dev.term_df = ix->term_df.as<uint32_t>();
    ix->dev.term_first_block = ix->term_first_block.as<uint32_t>();
    ix->dev.term_s0 = ix->term_s0.as<double>();
    ix->dev.term_wand_tf = ix->term_wand_tf.as<uint32_t>();
    ix->dev.term_wand_fn = ix->term_wand_fn.as<uint8_t>();
    ix->dev.blk_min_doc = ix->blk_min_doc.as<uint32_t>();
    ix->dev.blk_max_doc = ix->blk_max_doc.as<uint32_t>();
    ix->dev.blk_meta = ix->blk_meta.as<uint4>();
    ix->dev.blk_ub = ix->blk_ub.as<double>();
    ix->dev.blob = ix->blob.as<uint8_t>();
    ix->dev.post_fn = ix->post_fn.as<uint8_t>();
    ix->dev.post_rel16 = ix->post_rel16.as<uint32_t>();
    ix->dev.post_tfn = ix->post_tfn.as<uint32_t>();
    ix->dev.doc_payload = ix->doc_payload.as<uint16_t>();
    ix->dev.s1 = ix->s1.as<double>();
    ix->dev.term_kth_ub = ix->term_kth_ub.as<double>();  // (NULL when the block maxima are not attained)
    ix->dev.post_id16 = ix->post_id16.as<uint32_t>();    // (the three of them NULL when the index has no window planes)
    ix->dev.win_off = ix->win_off.as<uint32_t>();
    ix->dev.term_win = ix->term_win.as<uint32_t>();
    ix->dev.n_win = ix->n_win;
}

// A flattened sealed segment as index creation sees it: the big arrays on the host (vbm25_index_desc) or in the HBM of the
// index's device (vbm25_device_segment); the vocabulary-sized ones the host computes with (libm log) always on the host.
struct RawSegment {
    bool on_device;
    uint32_t n_docs, n_terms, n_blocks;
    uint64_t sum_len, blob_bytes;
    double k1, b;
    const uint8_t *term_key;                                  // host
    const uint32_t *term_df_host, *term_first_block_host;     // host
    const uint32_t *term_df, *term_wand_tf, *term_first_block, *blk_min_doc, *blk_max_doc, *blk_wand_tf, *blk_off8;
    const uint8_t *term_wand_fn, *blk_n, *blk_wand_fn, *blk_meta_doc, *blk_meta_tf, *blob, *doc_fieldnorm;
    const uint16_t *doc_payload;
};

// `device` is one of the n_dev devices and a gfx950: made the calling thread's current one.  (How a failed device count is answered
// is the caller's: index creation has its own text for a machine without a device.)
static int use_gfx950_device(int device, int n_dev) {
    if (device < 0 || device >= n_dev)
        return set_error(VBM25_ERR_INVALID, "device %d out of range (%d devices)", device, n_dev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (!std::strstr(prop.gcnArchName, "gfx950"))
        return set_error(VBM25_ERR_DEVICE, "device %d is %s; this library is built for gfx950 only",
                         device, prop.gcnArchName);
    return use_device(device);
}

static int index_create_common(const RawSegment &r, int device, vbm25_index **out) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: the MI355X path has no CPU fallback");
    if (int rc = use_gfx950_device(device, n_dev)) return rc;

    auto ix = std::make_unique<vbm25_index>();
    ix->device = device;
    ix->n_docs = r.n_docs;
    ix->n_terms = r.n_terms;
    ix->n_blocks = r.n_blocks;
    ix->k1 = r.k1;
    ix->b = r.b;
    ix->term_key.assign(r.term_key, r.term_key + 16ull * r.n_terms);
    ix->term_df_host.assign(r.term_df_host, r.term_df_host + r.n_terms);
    const hipMemcpyKind kind = r.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    auto put = [&](DeviceBuffer &dst, const void *src, size_t bytes) -> int {
        if (int rc = dst.alloc(bytes)) return rc;
        if (bytes) HIP_TRY(hipMemcpy(dst.p, src, bytes, kind));
        return VBM25_OK;
    };
    const bool has_wand = r.blk_wand_fn && r.blk_wand_tf;

    // per-term s0 = idf (k1 + 1), idf (vbm25_evaluate_batch) -- host libm log, bm25.rs:285-289,348 -- and the s1 table of
    // bm25.rs:349-352
    std::vector<double> s0(r.n_terms), idf(r.n_terms);
    for (uint32_t t = 0; t < r.n_terms; ++t) {
        s0[t] = bm25_s0(r.n_docs, r.term_df_host[t], r.k1);
        idf[t] = std::log((double(r.n_docs) + 1.0) / (double(r.term_df_host[t]) + 0.5));
    }
    double s1[256];
    bm25_tables(r.n_docs, r.sum_len, r.k1, r.b, s1);
    // scan_win_kernel's planes: the low 16 bits of every id in posting order, and for every term with at least a posting per four
    // windows the table of its n_win + 1 window offsets (a rarer term's table would be larger than its list)
    const Tuning tune_now = tuning_snapshot();
    const bool win_planes = tune_now.win_planes != 0 && r.n_blocks != 0;
    // (`rel16_plane` = 0: no post_rel16 -- scan_range_kernel and scan_dense_kernel unpack the delta streams of the blob in the
    // kernel: 256 bytes per block less in HBM, more instructions per block; DESIGN.md section 1 has both measured)
    const bool rel16_plane = tune_now.rel16_plane != 0;
    const bool id16_plane = tune_now.id16_plane != 0;  // (0: the tables without the plane -- decode_id16.h)
    const uint32_t n_win = uint32_t((uint64_t(r.n_docs) + 65535u) >> 16);
    std::vector<uint32_t> term_win(win_planes ? r.n_terms : 0u, UINT32_MAX);
    uint64_t n_woff = n_win + 2u;  // (entries 0 .. n_win + 1: the NULL table -- a term without postings, what a query's missing terms read)
    if (win_planes) {
        // BUDGET (round-5 advisor): a table is n_win + 1 words whatever the term's length -- up to four words per posting at the
        // threshold -- so on a corpus of thousands of windows and hundreds of thousands of qualifying terms the tables would take
        // gigabytes nobody asked for.  They get at most a quarter of what post_id16 takes (64 bytes per block; never less than 4 MiB), the
        // longest lists first: the routing sends a query through the window kernel only when EVERY term has a table, and the terms it
        // wants there are the long ones (32 .. 232 postings per window).
        const uint64_t budget_words = std::max<uint64_t>(1ull << 20, 16ull * r.n_blocks);
        std::vector<uint32_t> cand;
        for (uint32_t t = 0; t < r.n_terms; ++t)
            if (uint64_t(r.term_df_host[t]) * 4u >= n_win) cand.push_back(t);
        if (uint64_t(cand.size()) * (n_win + 1u) > budget_words) {
            std::stable_sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) { return r.term_df_host[a] > r.term_df_host[b]; });
            cand.resize(size_t(budget_words / (n_win + 1u)));
            std::sort(cand.begin(), cand.end());  // (tables in term order, as without a budget)
        }
        for (uint32_t t : cand) {
            if (n_woff + n_win + 1u > 0xfffffff0ull) break;
            term_win[t] = uint32_t(n_woff);
            n_woff += n_win + 1u;
        }
    }
    // the raw per-block arrays the derivation reads: used where they are (device segment) or uploaded for its duration
    DeviceBuffer t_n, t_wfn, t_wtf, t_md, t_mt, t_off8, t_fieldnorm, t_raw, t_sorted, t_tmp, err;
    const uint8_t *p_n = r.blk_n, *p_wfn = r.blk_wand_fn, *p_md = r.blk_meta_doc, *p_mt = r.blk_meta_tf, *p_fieldnorm = r.doc_fieldnorm;
    const uint32_t *p_wtf = r.blk_wand_tf, *p_off8 = r.blk_off8;
    int rc = 0;
    if (!r.on_device) {
        if ((rc = t_n.upload(r.blk_n, r.n_blocks)) || (rc = t_md.upload(r.blk_meta_doc, r.n_blocks)) ||
            (rc = t_mt.upload(r.blk_meta_tf, r.n_blocks)) || (rc = t_off8.upload(r.blk_off8, 4ull * (r.n_blocks + 1ull))) ||
            (rc = t_fieldnorm.upload(r.doc_fieldnorm, r.n_docs)) ||
            (has_wand && ((rc = t_wfn.upload(r.blk_wand_fn, r.n_blocks)) || (rc = t_wtf.upload(r.blk_wand_tf, 4ull * r.n_blocks)))))
            return rc;
        p_n = t_n.as<uint8_t>();
        p_md = t_md.as<uint8_t>();
        p_mt = t_mt.as<uint8_t>();
        p_off8 = t_off8.as<uint32_t>();
        p_fieldnorm = t_fieldnorm.as<uint8_t>();
        p_wfn = t_wfn.as<uint8_t>();
        p_wtf = t_wtf.as<uint32_t>();
    }
    // slack: the scan kernels read whole 256-byte LDS-DMA slots / word pairs from a block's first byte
    const size_t blob_alloc = ((size_t(r.blob_bytes) + 15) & ~size_t(15)) + 512;
    if ((rc = put(ix->term_df, r.term_df, 4ull * r.n_terms)) ||
        (rc = put(ix->term_first_block, r.term_first_block, 4ull * (r.n_terms + 1ull))) ||
        (rc = ix->term_s0.upload(s0.data(), 8ull * r.n_terms)) ||
        (rc = ix->term_idf.upload(idf.data(), 8ull * r.n_terms)) ||
        (rc = ix->fn_len.upload(fieldnorm_lengths(), 4ull * 256)) ||
        (rc = put(ix->term_wand_tf, r.term_wand_tf, 4ull * r.n_terms)) ||
        (rc = put(ix->term_wand_fn, r.term_wand_fn, r.n_terms)) ||
        (rc = put(ix->blk_min_doc, r.blk_min_doc, 4ull * r.n_blocks)) ||
        (rc = put(ix->blk_max_doc, r.blk_max_doc, 4ull * r.n_blocks)) ||
        (rc = ix->blk_meta.alloc(16ull * r.n_blocks)) ||
        (rc = ix->blk_ub.alloc(8ull * r.n_blocks)) ||
        (rc = ix->blob.alloc(blob_alloc)) ||
        (rc = ix->post_fn.alloc(128ull * r.n_blocks)) ||
        (rel16_plane && (rc = ix->post_rel16.alloc(256ull * r.n_blocks))) ||
        (rc = ix->post_tfn.alloc(256ull * r.n_blocks + 1024)) ||  // (slack: scan_win_kernel's cold pass reads whole runs)
        (win_planes && ((id16_plane && (rc = ix->post_id16.alloc(256ull * r.n_blocks + 1024))) || (rc = ix->win_off.alloc(4ull * n_woff)) ||
                        (rc = ix->term_win.upload(term_win.data(), 4ull * r.n_terms)))) ||
        (rc = put(ix->doc_payload, r.doc_payload, 6ull * r.n_docs)) ||
        (rc = ix->s1.upload(s1, sizeof s1)) || (rc = err.alloc(4)))
        return rc;
    HIP_TRY(hipMemset(err.p, 0, 4));
    HIP_TRY(hipMemset(ix->blob.p, 0, blob_alloc));
    if (r.blob_bytes) HIP_TRY(hipMemcpy(ix->blob.p, r.blob, r.blob_bytes, kind));
    if (r.n_blocks) {
        if (has_wand && ((rc = t_raw.alloc(8ull * r.n_blocks)) || (rc = t_sorted.alloc(8ull * r.n_blocks)) ||
                         (rc = ix->term_kth_ub.alloc(8ull * KTH_LEVELS * r.n_terms))))
            return rc;
        DeriveArgs da{};
        da.n_blocks = r.n_blocks;
        da.n_terms = r.n_terms;
        da.has_wand = has_wand ? 1u : 0u;
        da.term_first_block = ix->term_first_block.as<uint32_t>();
        da.term_wand_tf = ix->term_wand_tf.as<uint32_t>();
        da.term_wand_fn = ix->term_wand_fn.as<uint8_t>();
        da.blk_min_doc = ix->blk_min_doc.as<uint32_t>();
        da.blk_max_doc = ix->blk_max_doc.as<uint32_t>();
        da.blk_off8 = p_off8;
        da.blk_wand_tf = p_wtf;
        da.blk_n = p_n;
        da.blk_meta_doc = p_md;
        da.blk_meta_tf = p_mt;
        da.blk_wand_fn = p_wfn;
        da.term_s0 = ix->term_s0.as<double>();
        da.s1 = ix->s1.as<double>();
        da.blk_meta = ix->blk_meta.as<uint4>();
        da.blk_ub = ix->blk_ub.as<double>();
        da.blk_raw = t_raw.as<double>();
        blk_derive_kernel<<<(r.n_blocks + 255) / 256, 256>>>(da);
        HIP_TRY(hipGetLastError());
        if (has_wand) {
            // per term the 2^i-th largest block maximum, i = 0..8 (the scan kernels' first threshold: with block WAND pairs
            // every block maximum is the score of a posting of its block -- post_fn_kernel verifies that -- so k distinct
            // documents of the term score at least the k-th largest of them): a segmented sort of the maxima by term
            const uint32_t *seg = ix->term_first_block.as<uint32_t>();
            HIP_TRY(with_cub_temp(t_tmp, [&](void *t, size_t &tb) {
                return hipcub::DeviceSegmentedRadixSort::SortKeysDescending(t, tb, t_raw.as<double>(), t_sorted.as<double>(), (int)r.n_blocks,
                                                                            (int)r.n_terms, seg, seg + 1);
            }));
            kth_pick_kernel<<<(r.n_terms * KTH_LEVELS + 255) / 256, 256>>>(r.n_terms, seg, t_sorted.as<double>(), ix->term_kth_ub.as<double>());
            HIP_TRY(hipGetLastError());
        }
        const uint32_t grid = (r.n_blocks + 3) / 4;
        PostFnArgs pa{};
        pa.n_blocks = r.n_blocks;
        pa.n_docs = r.n_docs;
        pa.n_terms = r.n_terms;
        pa.blk_meta = ix->blk_meta.as<uint4>();
        pa.blob = ix->blob.as<uint8_t>();
        pa.doc_fieldnorm = p_fieldnorm;
        pa.post_fn = ix->post_fn.as<uint8_t>();
        pa.post_rel16 = ix->post_rel16.as<uint32_t>();
        pa.post_tfn = ix->post_tfn.as<uint32_t>();
        pa.post_id16 = ix->post_id16.as<uint32_t>();
        pa.win_off = ix->win_off.as<uint32_t>();
        pa.term_win = ix->term_win.as<uint32_t>();
        pa.n_win = n_win;
        if (win_planes) HIP_TRY(hipMemset(ix->win_off.p, 0, 4ull * n_woff));
        pa.error_flag = err.as<uint32_t>();
        pa.term_first_block = ix->term_first_block.as<uint32_t>();
        pa.term_wand_tf = ix->term_wand_tf.as<uint32_t>();
        pa.term_wand_fn = ix->term_wand_fn.as<uint8_t>();
        pa.term_s0 = ix->term_s0.as<double>();
        pa.s1 = ix->s1.as<double>();
        pa.blk_ub = ix->blk_ub.as<double>();
        pa.blk_raw = has_wand ? t_raw.as<double>() : nullptr;
        post_fn_kernel<<<grid, 256>>>(pa);
        HIP_TRY(hipGetLastError());
    }
    uint32_t flag = 0;
    HIP_TRY(hipMemcpy(&flag, err.p, 4, hipMemcpyDeviceToHost));
    if (flag & 1u)
        return set_error(VBM25_ERR_CORRUPT,
                         "posting blocks do not decode to strictly increasing ids within "
                         "[min_doc, max_doc] below n_docs");
    if (flag & 2u)
        return set_error(VBM25_ERR_CORRUPT,
                         "a posting scores above its block's / token's WAND pair "
                         "(search.rs:363,377-380 prune with those bounds)");
    if (win_planes && !(flag & 8u)) {  // (flag 8: a short block inside a term -- postings are not at 128 block + i: no window planes)
        ix->term_win_host = std::move(term_win);
        ix->n_win = n_win;
    } else {
        for (DeviceBuffer *b : {&ix->post_id16, &ix->win_off, &ix->term_win}) b->release();
    }
    ix->dev.blk_ub_attained = has_wand && !(flag & 4u) ? 1u : 0u;
    if (!ix->dev.blk_ub_attained && ix->term_kth_ub.p) {  // the k-th largest maxima bound nothing then: kept out of the index (and its replicas)
        ix->term_kth_ub.release();
    }
    fill_dev(ix.get());
    ix->dev.blob_bytes = r.blob_bytes;
    ix->dev.blk_ub_attained = has_wand && !(flag & 4u) ? 1u : 0u;
    for (const DeviceBuffer *b : {&ix->term_df, &ix->term_first_block, &ix->term_s0, &ix->blk_min_doc,
                                  &ix->blk_max_doc, &ix->blk_meta, &ix->blk_ub, &ix->blob, &ix->post_fn,
                                  &ix->post_rel16, &ix->post_tfn, &ix->term_kth_ub, &ix->doc_payload, &ix->s1,
                                  &ix->post_id16, &ix->win_off, &ix->term_win})
        ix->device_bytes += b->bytes;
    *out = ix.release();
    return VBM25_OK;
}

static int vbm25_index_create_impl(const vbm25_index_desc *d, int device, vbm25_index **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = check_desc(d)) return rc;
    RawSegment r{};
    r.on_device = false;
    r.n_docs = d->n_docs;
    r.n_terms = d->n_terms;
    r.n_blocks = d->n_blocks;
    r.sum_len = d->sum_len;
    r.blob_bytes = d->blob_bytes;
    r.k1 = d->k1;
    r.b = d->b;
    r.term_key = d->term_key;
    r.term_df_host = r.term_df = d->term_df;
    r.term_first_block_host = r.term_first_block = d->term_first_block;
    r.term_wand_tf = d->term_wand_tf;
    r.term_wand_fn = d->term_wand_fn;
    r.blk_min_doc = d->blk_min_doc;
    r.blk_max_doc = d->blk_max_doc;
    r.blk_n = d->blk_n;
    r.blk_wand_fn = d->blk_wand_fn;
    r.blk_wand_tf = d->blk_wand_tf;
    r.blk_meta_doc = d->blk_meta_doc;
    r.blk_meta_tf = d->blk_meta_tf;
    r.blk_off8 = d->blk_off8;
    r.blob = d->blob;
    r.doc_fieldnorm = d->doc_fieldnorm;
    r.doc_payload = d->doc_payload;
    return index_create_common(r, device, out);
}

// The index of a segment that is already in HBM (vbm25_device_segment_synth / _build): device-to-device copies of the arrays the
// index keeps as they are, everything else derived where it lies.  The segment is left as it was.
static int vbm25_index_create_from_device_impl(const vbm25_device_segment *ds, vbm25_index **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ds) return set_error(VBM25_ERR_INVALID, "segment is NULL");
    RawSegment r{};
    r.on_device = true;
    r.n_docs = ds->n_docs;
    r.n_terms = ds->n_terms;
    r.n_blocks = ds->n_blocks;
    r.sum_len = ds->sum_len;
    r.blob_bytes = ds->blob_bytes;
    r.k1 = ds->k1;
    r.b = ds->b;
    r.term_key = ds->term_key.data();
    r.term_df_host = ds->term_df.data();
    r.term_first_block_host = ds->term_first_block.data();
    r.term_df = ds->d_term_df.as<uint32_t>();
    r.term_first_block = ds->d_term_first_block.as<uint32_t>();
    r.term_wand_tf = ds->d_term_wand_tf.as<uint32_t>();
    r.term_wand_fn = ds->d_term_wand_fn.as<uint8_t>();
    r.blk_min_doc = ds->d_blk_min.as<uint32_t>();
    r.blk_max_doc = ds->d_blk_max.as<uint32_t>();
    r.blk_n = ds->d_blk_n.as<uint8_t>();
    r.blk_wand_fn = ds->d_blk_wand_fn.as<uint8_t>();
    r.blk_wand_tf = ds->d_blk_wand_tf.as<uint32_t>();
    r.blk_meta_doc = ds->d_blk_meta_doc.as<uint8_t>();
    r.blk_meta_tf = ds->d_blk_meta_tf.as<uint8_t>();
    r.blk_off8 = ds->d_blk_off8.as<uint32_t>();
    r.blob = ds->d_blob.as<uint8_t>();
    r.doc_fieldnorm = ds->d_doc_fieldnorm.as<uint8_t>();
    r.doc_payload = ds->d_doc_payload.as<uint16_t>();
    return index_create_common(r, ds->device, out);
}

// VACUUM's compaction (csrc/maintain.hip): the index's blocks, keys and payloads are read, nothing of it is changed
// (in.dev: vbm25_index_maintain_device, the inputs in a vbm25_device_vacuum's planes)
static int vbm25_index_maintain_impl(const vbm25_index *ix, const MaintainInput &in, uint32_t *relabel, vbm25_device_segment **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ix) return set_error(VBM25_ERR_INVALID, "index is NULL");
    if (in.dev) {
        int n_dev = 0;  // before the handles are looked into: without a device there is neither
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
            return set_error(VBM25_ERR_DEVICE, "no HIP device: maintain has no CPU entry point");
    }
    MaintainSource s{};
    s.device = ix->device;
    s.k1 = ix->k1;
    s.b = ix->b;
    s.n_docs = ix->n_docs;
    s.n_terms = ix->n_terms;
    s.n_blocks = ix->n_blocks;
    s.term_key = ix->term_key.data();
    s.term_first_block = ix->term_first_block.as<uint32_t>();
    s.blk_meta = ix->blk_meta.as<uint4>();
    s.blob = ix->blob.as<uint8_t>();
    s.doc_payload = ix->doc_payload.as<uint16_t>();
    return maintain_device(s, in, relabel, out);
}

int clone_index(const vbm25_index *src, int device, vbm25_index **out) {
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (int rc = use_gfx950_device(device, n_dev)) return rc;
    if (device != src->device) {  // direct xGMI copies where the runtime allows them (staged through the host otherwise)
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device, src->device) == hipSuccess && can) {
            const hipError_t e = hipDeviceEnablePeerAccess(src->device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
        (void)hipGetLastError();
    }
    auto ix = std::make_unique<vbm25_index>();
    ix->device = device;
    ix->n_docs = src->n_docs;
    ix->n_terms = src->n_terms;
    ix->n_blocks = src->n_blocks;
    ix->term_key = src->term_key;
    ix->term_df_host = src->term_df_host;
    ix->term_win_host = src->term_win_host;
    ix->n_win = src->n_win;
    ix->k1 = src->k1;
    ix->b = src->b;
    ix->device_bytes = src->device_bytes;
    for (auto member : INDEX_BUFFERS) {
        const DeviceBuffer &from = src->*member;
        if (!from.p) continue;
        DeviceBuffer &to = (*ix).*member;
        if (int rc = to.alloc(from.bytes)) return rc;
        if (from.bytes) HIP_TRY(hipMemcpyPeerAsync(to.p, device, from.p, src->device, from.bytes, nullptr));
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    fill_dev(ix.get());
    ix->dev.blob_bytes = src->dev.blob_bytes;
    ix->dev.blk_ub_attained = src->dev.blk_ub_attained;
    *out = ix.release();
    return VBM25_OK;
}

static int vbm25_evaluate_batch_impl(vbm25_index *ix, const uint32_t *q_terms, uint32_t n_q, uint32_t n_docs,
                                     const uint64_t *doc_start, const uint32_t *doc_term, const uint32_t *doc_tf,
                                     double *scores) {
    if (!ix || (n_q && !q_terms) || !doc_start || (n_docs && !scores)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_docs == 0) return VBM25_OK;
    const uint64_t n_el = doc_start[n_docs];
    if (n_el && (!doc_term || !doc_tf)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    {  // Query::checked_new, vector.rs:106-110: keys strictly ascending; ids of unknown tokens (>= n_terms) stand
       // wherever their keys sorted and are skipped, so every known id is compared with the last KNOWN one
        bool have = false;
        uint32_t prev = 0;
        for (uint32_t i = 0; i < n_q; ++i) {
            if (q_terms[i] >= ix->n_terms) continue;
            if (have && q_terms[i] <= prev) return set_error(VBM25_ERR_INVALID, "query term ids must be strictly ascending");
            prev = q_terms[i];
            have = true;
        }
    }
    for (uint32_t d = 0; d < n_docs; ++d) {
        if (doc_start[d + 1] < doc_start[d]) return set_error(VBM25_ERR_INVALID, "doc_start not monotone at document %u", d);
        uint32_t prev = 0;
        bool first = true;
        for (uint64_t e = doc_start[d]; e < doc_start[d + 1]; ++e) {
            if (doc_tf[e] == 0) return set_error(VBM25_ERR_INVALID, "document %u: term frequency 0", d);  // Document::checked_new
            if (doc_term[e] >= ix->n_terms) continue;
            if (!first && doc_term[e] <= prev) return set_error(VBM25_ERR_INVALID, "document %u: keys must be strictly ascending", d);
            prev = doc_term[e];
            first = false;
        }
    }
    if (int rc = use_device(ix->device)) return rc;
    if (ix->n_docs == 0) {  // avgdl is 0 / 0 in the reference: NaN scores; report it instead
        return set_error(VBM25_ERR_INVALID, "evaluate on an index without sealed documents");
    }
    DeviceBuffer dq, ds, dt, df, dout;
    int rc = 0;
    if ((rc = dq.upload(q_terms, 4ull * n_q)) || (rc = ds.upload(doc_start, 8ull * (n_docs + 1))) ||
        (rc = dt.upload(doc_term, 4ull * n_el)) || (rc = df.upload(doc_tf, 4ull * n_el)) || (rc = dout.alloc(8ull * n_docs)))
        return rc;
    EvalArgs a{};
    a.n_docs = n_docs;
    a.n_q = n_q;
    a.n_terms = ix->n_terms;
    a.q_terms = dq.as<uint32_t>();
    a.doc_start = ds.as<uint64_t>();
    a.doc_term = dt.as<uint32_t>();
    a.doc_tf = df.as<uint32_t>();
    a.term_idf = ix->term_idf.as<double>();
    a.s1 = ix->dev.s1;
    a.fn_len = ix->fn_len.as<uint32_t>();
    a.k1p1 = ix->k1 + 1.0;
    a.out = dout.as<double>();
    evaluate_kernel<<<(n_docs + 255) / 256, 256>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(scores, dout.p, 8ull * n_docs, hipMemcpyDeviceToHost));
    return VBM25_OK;
}

// what the other units read of an index (vbm25_internal.h)
int index_device_and_docs(const vbm25_index *ix, int *device, uint32_t *n_docs) {
    *device = ix->device;
    *n_docs = ix->n_docs;
    return VBM25_OK;
}
int index_vocabulary(const vbm25_index *ix, int *device, uint32_t *n_terms, const uint8_t **term_key) {
    *device = ix->device;
    *n_terms = ix->n_terms;
    *term_key = ix->term_key.data();
    return VBM25_OK;
}
int index_evaluate_tables(const vbm25_index *ix, EvaluateTables *out) {
    *out = EvaluateTables{ix->device, ix->n_docs, ix->n_terms, ix->k1, ix->term_idf.as<double>(), ix->dev.s1};
    return VBM25_OK;
}
int index_payloads(const vbm25_index *ix, const uint16_t **payload, uint32_t *n_docs) {
    *payload = ix->doc_payload.as<uint16_t>();
    *n_docs = ix->n_docs;
    return VBM25_OK;
}

}  // namespace vbm25

using namespace vbm25;

extern "C" {

int vbm25_index_create(const vbm25_index_desc *d, int device, vbm25_index **out) {
    return guarded([&] { return vbm25_index_create_impl(d, device, out); });
}
int vbm25_index_create_from_device(const vbm25_device_segment *ds, vbm25_index **out) {
    return guarded([&] { return vbm25_index_create_from_device_impl(ds, out); });
}
int vbm25_index_maintain(const vbm25_index *ix, const uint64_t *sealed_deleted, const vbm25_growing_desc *growing, uint32_t *relabel,
                         vbm25_device_segment **out) {
    return guarded([&] { return vbm25_index_maintain_impl(ix, MaintainInput{sealed_deleted, growing, nullptr}, relabel, out); });
}
int vbm25_index_maintain_device(const vbm25_index *ix, const vbm25_device_vacuum *in, uint32_t *relabel, vbm25_device_segment **out) {
    if (out) *out = nullptr;
    if (out && !in) return set_error(VBM25_ERR_INVALID, "NULL argument");  // (a NULL handle is not "no inputs")
    return guarded([&] { return vbm25_index_maintain_impl(ix, MaintainInput{nullptr, nullptr, in}, relabel, out); });
}

void vbm25_index_destroy(vbm25_index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    if (ix->scratch) vbm25_batch_destroy(ix->scratch);
    if (ix->scratch_grow) vbm25_batch_destroy(ix->scratch_grow);
    delete ix;
}

uint64_t vbm25_index_device_bytes(const vbm25_index *ix) { return ix ? ix->device_bytes : 0; }

int vbm25_lookup_terms(const vbm25_index *ix, const uint8_t *keys, uint32_t n, uint32_t *term_ids) {
    if (!ix || (!keys && n) || (!term_ids && n)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t lo = 0, hi = ix->n_terms;
        const uint8_t *key = keys + 16ull * i;
        while (lo < hi) {
            uint32_t mid = (lo + hi) >> 1;
            if (std::memcmp(ix->term_key.data() + 16ull * mid, key, 16) < 0) lo = mid + 1; else hi = mid;
        }
        term_ids[i] = (lo < ix->n_terms && !std::memcmp(ix->term_key.data() + 16ull * lo, key, 16))
                          ? lo : UINT32_MAX;
    }
    return VBM25_OK;
}

int vbm25_evaluate_batch(vbm25_index *ix, const uint32_t *q_terms, uint32_t n_q, uint32_t n_docs,
                         const uint64_t *doc_start, const uint32_t *doc_term, const uint32_t *doc_tf, double *scores) {
    return guarded([&] { return vbm25_evaluate_batch_impl(ix, q_terms, n_q, n_docs, doc_start, doc_term, doc_tf, scores); });
}

}  // extern "C"
