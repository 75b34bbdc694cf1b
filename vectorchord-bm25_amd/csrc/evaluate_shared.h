// evaluate_shared.h -- what evaluate.hip (vbm25_evaluate_documents) and rerank.hip (the scorer handle) have in common: the bound
// documents, the argument checks of a scoring call, the scoring kernel's arguments and its launch.  Both translation units score the
// same way from the same checked inputs; neither copies the other's text.  HIP-only, not part of the ABI.
#ifndef VBM25_EVALUATE_SHARED_H
#define VBM25_EVALUATE_SHARED_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "vbm25_internal.h"
#include "hip_host.h"

// Cast documents bound to one index's vocabulary: per document the ascending ids of its known elements with their tfs, and the
// fieldnorm code the cast gave it.  Only ever read after it is made, except by vbm25_doc_terms_append / _append_documents (live.hip),
// which write behind the documents it holds: from the first append on the arrays' `bytes` are capacities, and no consumer reads them
// for a length.
struct vbm25_doc_terms {
    const vbm25_index *index = nullptr;
    int device = 0;
    uint32_t n_docs = 0;
    uint64_t n_known = 0;
    bool from_index = false;  // made by vbm25_index_bind: its first base_docs documents are the index's own sealed documents, in the index's order
    vbm25::HbmArray d_start, d_term, d_tf, d_fieldnorm;
    // the documents the handle was bound with; documents base_docs .. n_docs were appended
    uint32_t base_docs = 0;
    // the appended documents' payloads, 6 bytes each (document base_docs + i at 3 i), when the appends carry them.  tail_decided: the
    // first append has been made, and tail_payload says whether it -- and so every later one -- carried payloads.
    bool tail_decided = false, tail_payload = false;
    vbm25::HbmArray d_tail_payload;
    // the deletion bitmap (vbm25_doc_terms_delete*, live.hip): one bit a document, document d at bit d & 63 of word d >> 6, set = dead.
    // NULL until the first delete that names a document; then words for the fieldnorm array's capacity, the bits at and beyond n_docs
    // zero.  Read by rerank_part_kernel and cand_lookup_kernel only.
    vbm25::HbmArray d_dead;
    uint32_t n_dead = 0;
};

namespace vbm25 {
namespace evl {

struct ScoreArgs {
    const unsigned long long *start;  // n_docs + 1
    const uint32_t *term, *tf;        // the known elements
    const uint8_t *fieldnorm;         // n_docs
    const double *term_idf, *s1;      // the index's tables
    double k1p1;
    uint32_t n_terms;
    const uint32_t *q_ids, *q_off;
    const unsigned long long *q_cand;  // nq + 1; NULL: every query scores documents 0 .. cross_docs
    const uint32_t *cand_doc;
    uint32_t cross_docs;
    const uint32_t *item_start;  // nq + 1: query q owns items item_start[q] .. item_start[q + 1], 64 candidates each
    uint32_t nq, n_items;
    double *scores;
};

// a double of lane `j` (the same j in every lane) to every lane, through the scalar unit
__device__ __forceinline__ double lane_double(double v, uint32_t j) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(b)), int(j))), hi = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(b >> 32)), int(j)));
    return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}

// The checks of vbm25_evaluate_documents, in its order and with its messages, before anything is enqueued.  `out` is the call's
// result array (only looked at for NULL).  VBM25_OK with *n_pairs == 0: nothing to score (nq == 0, or no query has a candidate).
// docs_later: the candidates' document indices are made on the device behind the call (the reranker's ctid lists), so cand_doc is
// not looked at; everything else is checked alike.
int check_score_call(const vbm25_doc_terms *t, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                     const uint32_t *cand_doc, const void *out, EvaluateTables *ix, uint64_t *n_pairs, bool docs_later = false);
// the handle's arrays and the index's tables into `a` (the call's own arrays are the caller's to fill)
void fill_score_tables(const vbm25_doc_terms *t, const EvaluateTables &ix, ScoreArgs *a);
// eval_score_kernel on `stream`, its grid capped by eval_grid as read now
hipError_t launch_eval_score(const ScoreArgs &a, hipStream_t stream);
// eval_grid of vbm25_tuning_set as it stands
uint32_t eval_grid_cap();
// The bind's steps on `stream`, grids capped by eval_grid as read now: vbm25_documents_bind and the appends of live.hip run the same
// kernels.  keys / doc_start / tf are a cast's arrays; ids has one entry an element, counts one a document.
//   lookup   ids[e] = the term id of key e in the vocabulary, or NOT_FOUND
//   count    counts[d] = the known elements of document d
//   compact  (id, tf) of document d's known elements to out_term / out_tf at start[d] .., in element order
hipError_t launch_bind_lookup(const void *keys, uint32_t n_el, const void *vocab, uint32_t n_terms, uint32_t *ids, hipStream_t stream);
hipError_t launch_bind_count(const uint32_t *ids, const unsigned long long *doc_start, uint32_t n_docs, uint32_t *counts, hipStream_t stream);
hipError_t launch_bind_compact(const uint32_t *ids, const uint32_t *tf, const unsigned long long *doc_start, const unsigned long long *start,
                               uint32_t n_docs, uint32_t *out_term, uint32_t *out_tf, hipStream_t stream);
int use_eval_device(int device);

}  // namespace evl
}  // namespace vbm25

#endif
