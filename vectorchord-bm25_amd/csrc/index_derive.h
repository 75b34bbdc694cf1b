// index_derive.h -- index creation on the device: blk_derive_kernel and kth_pick_kernel (block metadata, the blocks' and the terms'
// bounds) and post_fn_kernel (the per-posting planes + validation of block structure and WAND bounds).
// Included by index.hip only (non-template kernels: one definition).
#ifndef VBM25_INDEX_DERIVE_H
#define VBM25_INDEX_DERIVE_H

#include "device_types.h"
#include "decode.h"

namespace vbm25 {

// ---------------------------------------------------------------------------
// Index preparation: fieldnorm of every posting + structural validation
// ---------------------------------------------------------------------------
struct PostFnArgs {
    uint32_t n_blocks, n_docs, n_terms;
    const uint4 *blk_meta;
    const uint8_t *blob, *doc_fieldnorm;
    uint8_t *post_fn;
    uint32_t *post_rel16, *post_tfn;
    uint32_t *post_id16, *win_off;   // scan_win_kernel's planes (device_types.h); term_win says which terms have a table
    const uint32_t *term_win;
    uint32_t n_win;
    uint32_t *error_flag;
    // upper bounds to verify: the scan kernels prune with them
    const uint32_t *term_first_block, *term_wand_tf;
    const uint8_t *term_wand_fn;
    const double *term_s0, *s1, *blk_ub;
    const double *blk_raw;  // the block maxima without the margin (NULL: no block WAND pairs): what "attained" is tested against
};
__global__ void __launch_bounds__(256) post_fn_kernel(PostFnArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t j = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (j >= a.n_blocks) return;
    const uint4 m = a.blk_meta[j];
    const uint32_t n = m.w & 0xff, md = (m.w >> 8) & 0xff, mt = (m.w >> 16) & 0xff;
    const uint8_t *body = a.blob + 8ull * m.z;
    uint32_t d0, d1;
    decode_doc_ids(body, md, n, m.x, lane, d0, d1);
    const uint32_t i0 = 2 * lane, i1 = i0 + 1;
    uint8_t f0 = 0, f1 = 0;
    bool bad = false;
    if (i0 < n) {
        bad |= d0 >= a.n_docs;
        if (d0 < a.n_docs) f0 = a.doc_fieldnorm[d0];
    }
    if (i1 < n) {
        bad |= d1 >= a.n_docs || d1 <= d0;
        if (d1 < a.n_docs) f1 = a.doc_fieldnorm[d1];
    }
    // strictly increasing across lanes, first = min_doc, last = max_doc
    const uint32_t prev = __shfl_up(d1, 1);
    if (lane > 0 && i0 < n) bad |= d0 <= prev;
    if (i0 == 0) bad |= d0 != m.x;
    if (i0 == n - 1) bad |= d0 != m.y;
    if (i1 == n - 1) bad |= d1 != m.y;
    if (bad) atomicOr(a.error_flag, 1u);
    reinterpret_cast<uchar2 *>(a.post_fn + 128ull * j)[lane] = make_uchar2(f0, f1);
    if (a.post_rel16) a.post_rel16[64ull * j + lane] = rel16_block(m.x, m.y, m.w) ? (d1 - m.x) << 16 | (d0 - m.x) : 0u;

    // The WAND pairs must bound every posting: Cache::evaluate of each posting against the block's
    // bound (blk_ub, margin included) and the token's (search.rs:363,377-380).
    uint32_t lo = 0, hi = a.n_terms;  // the term of block j: term_first_block[t] <= j < [t + 1]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.term_first_block[mid] <= j) lo = mid; else hi = mid;
    }
    // The window-major planes (scan_win_kernel): the low 16 bits of every id in posting order, and -- for the terms that have a
    // table -- the number of the term's postings below every multiple of 2^16 documents.  Posting i of block j is posting
    // 128 (j - first block) + i of its term: only a term's last block is short (flag 8 otherwise: the index then goes without
    // these planes).  Every boundary w << 16 lies between two consecutive postings of the term (or before its first / after its
    // last one): the later of the two writes entry w.
    // (an index made without post_id16 keeps the tables: decode_id16_kernel makes the batch's terms' ids per launch)
    if (a.post_id16) a.post_id16[64ull * j + lane] = (d1 & 0xffffu) << 16 | (d0 & 0xffffu);
    if (a.win_off) {
        const uint32_t fb = a.term_first_block[lo], fe = a.term_first_block[lo + 1];
        if (j + 1 < fe && n != 128u) atomicOr(a.error_flag, 8u);
        const uint32_t wb = a.term_win[lo];
        if (wb != NONE32 && !bad) {
            const long long before = j == fb ? -1ll : (long long)a.blk_meta[j - 1].y;  // last document of the term before this block
            if (lane == 0 && before >= (long long)d0) atomicOr(a.error_flag, 1u);  // a term's blocks must ascend
            const long long p0 = lane == 0 ? before : (long long)prev;
            const long long nw = (long long)a.n_win;
            const uint32_t at = 128u * (j - fb);
            if (i0 < n)
                for (long long w = (p0 >> 16) + 1; w <= min((long long)(d0 >> 16), nw); ++w) a.win_off[wb + w] = at + i0;
            if (i1 < n)
                for (long long w = (long long)(d0 >> 16) + 1; w <= min((long long)(d1 >> 16), nw); ++w) a.win_off[wb + w] = at + i1;
            if (j + 1 == fe && lane == (n - 1u) >> 1) {  // behind the term's last posting: all of them
                const uint32_t dl = ((n - 1u) & 1u) ? d1 : d0;
                for (long long w = (long long)(dl >> 16) + 1; w <= nw; ++w) a.win_off[wb + w] = at + n;
            }
        }
    }
    const double s0 = a.term_s0[lo];
    const double wtf = (double)a.term_wand_tf[lo];
    const double tub = ((wtf * s0) / (wtf + a.s1[a.term_wand_fn[lo]])) * (1.0 + 1e-12);
    const double bub = a.blk_ub[j];
    uint32_t t0, t1;
    decode_fields(body + ((payload_bytes(md, n) + 7u) & ~7u), mt, n, lane, t0, t1);
    // (the two term frequencies and fieldnorm bytes of the lane's postings.  scan_range_kernel / scan_dense_kernel read the word of
    // tfn_block blocks only; scan_win_kernel reads it for every posting -- tails included -- and takes a zero term frequency for
    // "wider than a byte")
    a.post_tfn[64ull * j + lane] = t0 <= 255u && t1 <= 255u ? t0 | t1 << 8 | (uint32_t)f0 << 16 | (uint32_t)f1 << 24 : 0u;
    // (attained: the very score the k-th largest maxima are taken from -- blk_raw, no margin: compared after the margin two scores
    // an ulp apart could round to the same value and a bound one ulp above every posting would pass)
    const bool braw_ok = a.blk_raw != nullptr;
    const double braw = braw_ok ? a.blk_raw[j] : 0.0;
    bool loose = false, attained = false;  // attained: the block's bound is the score of one of its postings (flag 4 if not: no error,
                                           // but the k-th largest block maxima are then no lower bound of anything)
    if (i0 < n) {
        const double tf = (double)t0, p = (tf * s0) / (tf + a.s1[f0]);
        loose |= p > bub || p > tub;
        attained |= braw_ok && p == braw;
    }
    if (i1 < n) {
        const double tf = (double)t1, p = (tf * s0) / (tf + a.s1[f1]);
        loose |= p > bub || p > tub;
        attained |= braw_ok && p == braw;
    }
    if (loose) atomicOr(a.error_flag, 2u);
    if (!__ballot(attained) && lane == 0) atomicOr(a.error_flag, 4u);
}

// ---------------------------------------------------------------------------
// Index creation: what the index derives from the raw block / token arrays, on the device (the arrays may never have been on
// the host: vbm25_index_create_from_device)
// ---------------------------------------------------------------------------
struct DeriveArgs {
    uint32_t n_blocks, n_terms, has_wand;
    const uint32_t *term_first_block, *term_wand_tf, *blk_min_doc, *blk_max_doc, *blk_off8, *blk_wand_tf;
    const uint8_t *term_wand_fn, *blk_n, *blk_meta_doc, *blk_meta_tf, *blk_wand_fn;
    const double *term_s0, *s1;
    uint4 *blk_meta;
    double *blk_ub;   // Cache::evaluate(block WAND pair) x (1 + 1e-12) (search.rs:377-380 evaluates it per visited block; here once)
    double *blk_raw;  // the same without the margin (has_wand): what the k-th largest block maxima of a term are taken from
};
__global__ void __launch_bounds__(256) blk_derive_kernel(DeriveArgs a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n_blocks) return;
    uint32_t lo = 0, hi = a.n_terms;  // the term of block j: term_first_block[t] <= j < [t + 1]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.term_first_block[mid] <= j) lo = mid; else hi = mid;
    }
    const uint32_t wfn = a.has_wand ? a.blk_wand_fn[j] : 0u;
    a.blk_meta[j] = make_uint4(a.blk_min_doc[j], a.blk_max_doc[j], a.blk_off8[j],
                               (uint32_t)a.blk_n[j] | (uint32_t)a.blk_meta_doc[j] << 8 | (uint32_t)a.blk_meta_tf[j] << 16 | wfn << 24);
    const double s0 = a.term_s0[lo];
    double ub;
    if (a.has_wand) {
        const double tf = (double)a.blk_wand_tf[j];
        ub = (tf * s0) / (tf + a.s1[wfn]);
        a.blk_raw[j] = ub;
    } else {
        const double wtf = (double)a.term_wand_tf[lo];
        ub = (wtf * s0) / (wtf + a.s1[a.term_wand_fn[lo]]);
    }
    a.blk_ub[j] = ub * (1.0 + 1e-12);  // margin: another posting's evaluate may round one ulp higher
}
// sorted: every term's block maxima in descending order (segmented sort) -> the 2^i-th largest, i = 0..8 (0 when fewer)
__global__ void __launch_bounds__(256) kth_pick_kernel(uint32_t n_terms, const uint32_t *term_first_block, const double *sorted, double *kth) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_terms * 9u) return;
    const uint32_t t = e / 9u, i = e - 9u * t;
    const uint32_t b0 = term_first_block[t], nb = term_first_block[t + 1] - b0, at = (1u << i) - 1u;
    kth[e] = at < nb ? sorted[b0 + at] : 0.0;
}

}  // namespace vbm25

#endif
