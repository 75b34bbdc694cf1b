// vbm25_internal.h -- shared between the host (.cpp) and device (.hip) units of libvbm25.  Not part of the ABI.
#ifndef VBM25_INTERNAL_H
#define VBM25_INTERNAL_H

#include <cstddef>
#include <cstdint>
#include <exception>
#include <new>
#include <vector>

#include "../../include/vbm25.h"

namespace vbm25 {

// Thread-local error text; returns `code` so callers can `return set_error(...)`.
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// The calling thread's error text copied out and put back, ERROR_TEXT_BYTES either way (error.cpp keeps the text: a worker thread's
// error becomes its caller's, multi.hip)
constexpr size_t ERROR_TEXT_BYTES = 512;
void error_text_read(char *out);
void error_text_write(const char *in);

// No C++ exception may cross the C ABI (the reference's crate is #![deny(ffi_unwind_calls)], src/lib.rs:16):
// every entry point that allocates runs its body through this.
template <class F>
int guarded(F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return set_error(VBM25_ERR_NOMEM, "out of host memory");
    } catch (const std::exception &e) {
        return set_error(VBM25_ERR_INVALID, "internal error: %s", e.what());
    } catch (...) {
        return set_error(VBM25_ERR_INVALID, "internal error");
    }
}

// bm25.rs:15-283
const uint32_t *fieldnorm_lengths();
uint8_t length_to_fieldnorm(uint32_t length);
// Cache::new (bm25.rs:340-354): the per-index s1[256] table and the per-term s0
void bm25_tables(uint32_t n_docs, uint64_t sum_len, double k1, double b, double *s1_256);
double bm25_s0(uint32_t n_docs, uint32_t df, double k1);

int check_desc(const vbm25_index_desc *d);
// BLAKE3 hash (key32 == NULL) or keyed hash of `in`; out_len bytes of output
void blake3(const uint8_t *key32, const uint8_t *in, size_t len, uint8_t *out, size_t out_len);

// Host copy of a flattened sealed segment (the arrays of vbm25_index_desc).
struct Segment {
    uint32_t n_docs = 0, n_terms = 0, n_blocks = 0;
    uint64_t sum_len = 0;
    double k1 = 1.2, b = 0.75;
    std::vector<uint8_t> term_key;
    std::vector<uint32_t> term_df;
    std::vector<uint8_t> term_wand_fn;
    std::vector<uint32_t> term_wand_tf;
    std::vector<uint32_t> term_first_block;
    std::vector<uint32_t> blk_min_doc, blk_max_doc;
    std::vector<uint8_t> blk_n, blk_wand_fn;
    std::vector<uint32_t> blk_wand_tf;
    std::vector<uint8_t> blk_meta_doc, blk_meta_tf;
    std::vector<uint32_t> blk_off8;
    std::vector<uint8_t> blob;
    std::vector<uint8_t> doc_fieldnorm;
    std::vector<uint16_t> doc_payload;
    std::vector<uint32_t> token_term;  // synthetic corpora only: token number -> term id
    void desc(vbm25_index_desc *d) const;
};

// The growing segment's CSR in HBM on the index's device (vbm25_growing_desc's arrays, start[0] == 0): what the device reader of the
// vectors tape (pages_device.hip) hands to the builder of the device growing segment (growing.hip)
struct GrowingDeviceArrays {
    uint32_t n_docs;
    uint64_t n_elements;
    const uint64_t *start;
    const uint8_t *key;
    const uint32_t *tf;
    const uint8_t *fieldnorm, *deleted;
    const uint16_t *payload;
};
int index_device_and_docs(const vbm25_index *ix, int *device, uint32_t *n_docs);
// the index's device and its host copy of the vocabulary (16 bytes a term, ascending): what a resolver (resolve.hip) uploads at create
int index_vocabulary(const vbm25_index *ix, int *device, uint32_t *n_terms, const uint8_t **term_key);
// the device half of vbm25_growing_upload; synchronous, the arrays may be freed when it returns
int growing_from_device_arrays(vbm25_index *ix, const GrowingDeviceArrays &a, vbm25_device_growing **out);
// vbm25_tuning_set's cast_wave_max / cast_group_max (cast.hip keeps them: the class bounds of vbm25_documents_cast, 0 = class off,
// values over the built-in bounds refused), cast_pack (0 .. 2) and cast_grid (0 .. 2048) of vbm25_caster_submit, and their reset
int cast_tuning_set(const char *name, long long value);
void cast_tuning_reset();
// What the evaluate operator on bound documents (evaluate.hip) reads of a resolver (resolve.hip fills it in): its index, the
// index's device and the vocabulary's keys in HBM (16 bytes a term, ascending; complete once vbm25_resolver_create has returned)
struct ResolverVocabulary {
    const vbm25_index *index;
    int device;
    uint32_t n_terms;
    const void *keys;
};
int resolver_vocabulary(const vbm25_resolver *r, ResolverVocabulary *out);
// ... and of an index (index.hip fills it in): the per-term idf and the s1 table vbm25_evaluate_batch scores with, both in HBM
struct EvaluateTables {
    int device;
    uint32_t n_docs, n_terms;
    double k1;
    const double *term_idf, *s1;
};
int index_evaluate_tables(const vbm25_index *ix, EvaluateTables *out);
// ... and the index's payload plane in HBM (6 bytes a sealed document): what a reranker made on an index-bound handle builds its
// ctid directory from (reranker.hip)
int index_payloads(const vbm25_index *ix, const uint16_t **payload, uint32_t *n_docs);
// vbm25_tuning_set's fwd_grid (the most workgroups of vbm25_index_bind's kernels, 0 .. 2048, 0 = no cap), fwd_wave_max and
// fwd_group_max (its class bounds, 0 = class off, values over the built-in bounds refused); forward.hip keeps them and reads them at
// the start of each bind
int forward_tuning_set(const char *name, long long value);
void forward_tuning_reset();
// vbm25_tuning_set's eval_grid (evaluate.hip keeps it: the most workgroups of a bind's or a score's kernels, 1 .. 2048) and its reset
int evaluate_tuning_set(long long value);
void evaluate_tuning_reset();
// vbm25_tuning_set's rerank_part (candidates a part of a scorer's top-k, 64 .. 2^20 in 64s) and rerank_buf (the selection buffer as a
// multiple of k, 2 .. 8); rerank.hip keeps them and reads them at the start of each scorer call
int rerank_tuning_set(const char *name, long long value);
void rerank_tuning_reset();
// vbm25_tuning_set's tid_grid (the most workgroups of tid_match_kernel, 1 .. 2048, read at each launch) and tid_dir (log2 of a TID
// set's directory entries, 0 .. 12, read at each vbm25_tid_set_create); tid.hip keeps them
int tid_tuning_set(const char *name, long long value);
void tid_tuning_reset();
// vbm25_tuning_set's live_sort_max (the most rows of a delta that vbm25_reranker_sync sorts in one workgroup's LDS, 0 .. 4096, 0 = always
// the radix sort; read at each sync); live.hip keeps it
int live_tuning_set(long long value);
void live_tuning_reset();
// tid_dir as it stands (the reranker's payload directory is built under it, as a TID set's is)
uint32_t tid_dir_now();
// tid_grid as it stands, and what a match kernel outside tid.hip reads of a TID set (tid.hip fills it in; live.hip's
// vbm25_doc_terms_delete_tids): the sorted distinct keys and the directory over them, in HBM on `device`
uint32_t tid_grid_now();
struct TidSetView {
    int device;
    uint64_t n_keys;
    uint32_t n_dir, stride;
    const unsigned long long *keys, *dir;
};
void tid_set_view(const vbm25_tid_set *s, TidSetView *out);

}  // namespace vbm25

struct vbm25_segment : vbm25::Segment {};

// Host copy of the growing segment's CSR (vbm25_growing_from_pages; vbm25_device_growing_from_pages' `csr`)
struct vbm25_growing {
    std::vector<uint64_t> start{0};
    std::vector<uint8_t> key;
    std::vector<uint32_t> tf;
    std::vector<uint8_t> fieldnorm;
    std::vector<uint16_t> payload;
    std::vector<uint8_t> deleted;
};

#endif
