/*
 * vbm25.h -- C ABI of the MI355X-native BM25 top-k scorer (libvbm25.so).
 *
 * Drop-in boundary: this library replaces ONE call of the reference,
 *     bm25::search(&index, k, &query, filter)
 * made at /root/reference/src/index/bm25/scanners/default.rs:117-129 and defined
 * at crates/bm25/src/search.rs:28-36, plus the index flattening that feeds it.
 * INTEGRATION.md shows the Rust `extern "C"` block and the replacement body of
 * DefaultBuilder::build a maintainer would add.
 *
 * Conventions: plain pointers and sizes, caller-owned
 * outputs, no callbacks, no exceptions or longjmp across the boundary.  Every
 * function returns 0 on success or a negative vbm25_status; the message for the
 * last failure on the calling thread is available from vbm25_last_error().
 * One handle may be used from one thread at a time.
 */
#ifndef VBM25_H
#define VBM25_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vbm25_status {
    VBM25_OK = 0,
    VBM25_ERR_INVALID = -1,     /* bad argument (reference: pgrx::error! at default.rs:114-116 etc.) */
    VBM25_ERR_CORRUPT = -2,     /* index arrays inconsistent (reference: panic "data corruption") */
    VBM25_ERR_DEVICE = -3,      /* HIP runtime failure / no gfx950 device */
    VBM25_ERR_UNSUPPORTED = -4, /* valid request outside what the GPU path covers */
    VBM25_ERR_NOMEM = -5
} vbm25_status;

/* One result: replaces (Reverse<Score>, AlwaysEqual<[u16; 3]>) of search.rs:33.
 * score is the positive f64 (the SQL operator negates it, operators.rs:54);
 * payload is the heap ctid key (fetcher.rs:218-232). */
typedef struct vbm25_hit {
    double score;
    uint32_t doc_id;
    uint16_t payload[3];
    uint16_t _pad;
} vbm25_hit;

/* Flattened sealed segment: the values flush.rs:40-158 writes to the Token /
 * Summary / Block / Document tapes (tuples.rs:756-1069), as arrays.
 * All pointers are host memory, borrowed for the duration of the call. */
typedef struct vbm25_index_desc {
    uint32_t n_docs;              /* JumpTuple.number_of_documents */
    uint32_t n_terms;
    uint32_t n_blocks;
    uint32_t _pad;
    uint64_t sum_len;             /* JumpTuple.sum_of_document_lengths */
    uint64_t blob_bytes;
    double k1, b;                 /* MetaTuple.k1 / b */
    const uint8_t *term_key;          /* n_terms x 16, ascending (TokenTuple.id) */
    const uint32_t *term_df;          /* TokenTuple.number_of_documents */
    const uint8_t *term_wand_fn;      /* TokenTuple.wand_fieldnorm */
    const uint32_t *term_wand_tf;     /* TokenTuple.wand_term_frequency */
    const uint32_t *term_first_block; /* n_terms + 1; summaries of a token are contiguous */
    const uint32_t *blk_min_doc;      /* SummaryTuple.min_document_id */
    const uint32_t *blk_max_doc;      /* SummaryTuple.max_document_id */
    const uint8_t *blk_n;             /* SummaryTuple.number_of_documents (1..128) */
    const uint8_t *blk_wand_fn;       /* SummaryTuple.wand_fieldnorm */
    const uint32_t *blk_wand_tf;      /* SummaryTuple.wand_term_frequency */
    const uint8_t *blk_meta_doc;      /* BlockTuple.metadata_document_ids */
    const uint8_t *blk_meta_tf;       /* BlockTuple.metadata_term_frequencies */
    const uint32_t *blk_off8;         /* n_blocks + 1: block body offset in blob, units of 8 B */
    const uint8_t *blob;              /* per block: doc-id bytes, pad to 8, tf bytes, pad to 8 */
    const uint8_t *doc_fieldnorm;     /* DocumentTuple.fieldnorm, n_docs */
    const uint16_t *doc_payload;      /* DocumentTuple.payload, n_docs x 3 */
} vbm25_index_desc;

const char *vbm25_last_error(void);
const char *vbm25_version(void);

/* ------------------------------------------------------------------------
 * Host side: sealed-segment construction (replaces flush.rs:40-158 for the
 * benchmark / test harness; CPU, multi-threaded, byte-identical output).
 * ---------------------------------------------------------------------- */
typedef struct vbm25_segment vbm25_segment;

/* Segment = records (length, payload) in doc-id order + mappings sorted by
 * (token key, doc id) in CSR form (segment.rs:19-50). threads <= 0: all cores. */
int vbm25_segment_build(double k1, double b, uint32_t n_docs, const uint32_t *doc_len,
                        const uint16_t *doc_payload, uint32_t n_terms, const uint8_t *term_key,
                        const uint64_t *term_start, const uint32_t *post_doc,
                        const uint32_t *post_tf, int threads, vbm25_segment **out);

/* The same construction on the device (csrc/flush.hip): one wave per 128-posting block (bit
 * width = OR of the deltas, 4-lane vertical packing, first-maximiser WAND pairs).  Same arguments, same
 * vbm25_segment, byte for byte; needs a gfx950 device (VBM25_ERR_DEVICE otherwise -- no silent fallback). */
int vbm25_segment_build_device(int device, double k1, double b, uint32_t n_docs, const uint32_t *doc_len,
                               const uint16_t *doc_payload, uint32_t n_terms, const uint8_t *term_key,
                               const uint64_t *term_start, const uint32_t *post_doc,
                               const uint32_t *post_tf, vbm25_segment **out);

/* The same from mappings in ANY order -- (token rank, document, term frequency) triples as the tokenizer emits them:
 * the device radix-sorts them into the (token, document) order of segment.rs:41-45 (the reference merges sorted
 * runs, io.rs:244-282) and encodes.  Byte-identical to vbm25_segment_build on the sorted CSR form.  Errors: a token
 * rank >= n_terms, a token without mappings, a repeated (token, document) pair, tf = 0 (VBM25_ERR_INVALID). */
int vbm25_segment_build_device_unsorted(int device, double k1, double b, uint32_t n_docs, const uint32_t *doc_len,
                                        const uint16_t *doc_payload, uint32_t n_terms, const uint8_t *term_key,
                                        uint64_t n_mappings, const uint32_t *map_term, const uint32_t *map_doc,
                                        const uint32_t *map_tf, vbm25_segment **out);

/* Synthetic corpus of SURVEY section 8(d), generated per token so that 10M-50M
 * documents stream: every document is `len` i.i.d. token draws (uniform, or
 * Zipf(s) over token rank when zipf_s > 0); token t's key is its ASCII decimal,
 * zero padded (vector.rs:21-24 short path).  len_mode 0: every document has
 * mean_len draws; 1: clamp(round(LogNormal(ln(0.8*mean_len), 0.6)), 8, 2000). */
typedef struct vbm25_synth_params {
    uint32_t n_docs;
    uint32_t vocab;
    uint32_t mean_len;
    uint32_t len_mode;
    double zipf_s;
    double k1, b;
    uint64_t seed;
    int threads;
    int _pad;
} vbm25_synth_params;
int vbm25_segment_synth(const vbm25_synth_params *params, vbm25_segment **out);
/* token number -> term id (rank of its key among the keys present), UINT32_MAX if absent */
int vbm25_segment_synth_token_terms(const vbm25_segment *, const uint32_t *tokens, uint32_t n,
                                    uint32_t *term_ids);

int vbm25_segment_desc(const vbm25_segment *, vbm25_index_desc *out);
void vbm25_segment_free(vbm25_segment *);
/* Serialise / load the flattened arrays (bench.py: rank 0 builds, other ranks load). */
int vbm25_segment_save(const vbm25_segment *, const char *path);
int vbm25_segment_load(const char *path, vbm25_segment **out);

/* Algorithmic bytes of one query, SURVEY section 8(d) (exhaustive evaluation:
 * block bodies + 16 B block header + 24 B summary per block + 1 fieldnorm byte
 * per posting + 14 B per returned hit). term ids >= n_terms are ignored. */
uint64_t vbm25_query_bytes(const vbm25_index_desc *, const uint32_t *term_ids, uint32_t n_terms,
                           uint32_t k);

/* FIELDNORM_TO_LENGTH (bm25.rs:15-272; 256 entries) and the term-independent half of Cache::new, s1[f] = k1 * (1 - b +
 * b * FIELDNORM_TO_LENGTH[f] / avgdl) with avgdl = sum_len / n_docs (bm25.rs:349-352), exactly as the library uses them. */
int vbm25_fieldnorm_table(uint32_t *lengths256);
int vbm25_cache_s1(uint32_t n_docs, uint64_t sum_len, double k1, double b, double *s1_256);

/* ------------------------------------------------------------------------
 * Host side of the shim: the growing (unsealed) segment, search.rs:83-135.
 * Documents inserted since the last VACUUM live in VectorTuples, not in
 * posting lists; the reference scores every one of them on the CPU before the
 * WAND loop, and so does the shim -- these two functions are that code.
 *
 * vbm25_growing_search: `query_keys` = the Query's sorted 16-byte keys; keys
 * without a TokenTuple are dropped (search.rs:59-61) and the others get the
 * sealed segment's statistics (Cache::new, search.rs:69-75).  Documents are
 * given as CSR over their elements (VectorTuple `Element{key, value}`, in
 * tuple order): score = sum of Cache::evaluate(fieldnorm, tf) over the elements
 * whose key is in the query, in element order; deleted documents are skipped; a
 * document enters only if threshold < score (so zero-score documents never
 * do, and a document tying the k-th score does not replace it).  Output: at
 * most k hits, best first, ties by document order; doc_id = 0xFFFFFFFF - index
 * of the document in the growing list (not a sealed document id).
 *
 * vbm25_merge_hits: top-k of the union of two best-first lists (sealed hits from
 * the device, growing hits from above); on equal scores sealed hits come first
 * (the reference leaves ties to BinaryHeap; unpinned).
 * ---------------------------------------------------------------------- */
int vbm25_growing_search(const vbm25_index_desc *desc, const uint8_t *query_keys, uint32_t n_keys,
                         uint32_t k, uint32_t n_grow, const uint64_t *g_start, const uint8_t *g_key,
                         const uint32_t *g_tf, const uint8_t *g_fieldnorm, const uint16_t *g_payload,
                         const uint8_t *g_deleted, vbm25_hit *hits, uint32_t *n_hits);
int vbm25_merge_hits(const vbm25_hit *sealed, uint32_t n_sealed, const vbm25_hit *grow, uint32_t n_grow,
                     uint32_t k, vbm25_hit *out, uint32_t *n_out);

/* bm25::evaluate (evaluate.rs:22-74): one document against one query with the sealed segment's
 * statistics -- what `tsvector <&> bm25query` computes when it runs as a plain function
 * (operators.rs:48-54, which returns the negated value).  Host code, as in the reference.  The
 * document's elements (key, tf) must be in ascending key order (vector.rs:50-75); its length is the
 * saturating sum of the tfs; result = sum over the query's keys found in both the document and the
 * index of idf(N, df) * tf(fieldnorm, tf, k1, b, avgdl), in key order (bm25.rs:285-295). */
int vbm25_evaluate(const vbm25_index_desc *desc, const uint8_t *doc_key, const uint32_t *doc_tf,
                   uint32_t n_doc_elements, const uint8_t *query_keys, uint32_t n_keys, double *score);

/* ------------------------------------------------------------------------
 * Host side: reading a bm25 index relation in the reference's own on-disk
 * format (PostgreSQL 8 KiB pages), the step between PostgreSQL and the GPU.
 *
 * `read_page(ctx, page_id)` returns the 8192-byte image of one page of the index
 * relation (the shim wraps ReadBuffer / a snapshot of the relation file), or
 * NULL.  Page layout: src/index/storage.rs:49-170 over PostgreSQL's page header
 * (24 B) + 4-byte line pointers (slots are 1-based) + 8-byte special area
 * Opaque{next, flags} (crates/bm25/src/lib.rs:41-46).
 *
 * vbm25_segment_from_pages walks what search() reads, in the order maintain.rs
 * :104-161 walks it: Meta (page 0, slot 1: magic "vchordbm", version 1, k1, b,
 * ptr_jump) -> Jump -> documents tape -> tokens tape -> summaries tape ->
 * blocks tape (tuples.rs:48-94,141-203,756-781,833-862,900-934,973-1025), and
 * checks while flattening that every token's summaries and every summary's
 * block sit where the WAND pointers say.  The result is an ordinary
 * vbm25_segment: vbm25_segment_desc + vbm25_index_create put it on the GPU
 * with no re-encoding (block bodies are copied byte for byte).  Anything the
 * reference would panic on ("data corruption", bad magic / version) returns
 * VBM25_ERR_CORRUPT.
 *
 * vbm25_growing_from_pages collects the unsealed documents of the same relation
 * (vectors tape from Jump.ptr_vectors; VectorTuple _2 / _1 / _0, tuples.rs
 * :326-426, state machine of search.rs:83-135) in the CSR form
 * vbm25_growing_search takes.
 * ---------------------------------------------------------------------- */
typedef const uint8_t *(*vbm25_read_page_fn)(void *ctx, uint32_t page_id);
int vbm25_segment_from_pages(vbm25_read_page_fn read_page, void *ctx, vbm25_segment **out);

typedef struct vbm25_growing vbm25_growing;
typedef struct vbm25_growing_desc {
    uint32_t n_docs;
    uint32_t _pad;
    uint64_t n_elements;
    const uint64_t *start;     /* n_docs + 1 */
    const uint8_t *key;        /* n_elements x 16 */
    const uint32_t *tf;        /* n_elements */
    const uint8_t *fieldnorm;  /* n_docs */
    const uint16_t *payload;   /* n_docs x 3 */
    const uint8_t *deleted;    /* n_docs */
} vbm25_growing_desc;
int vbm25_growing_from_pages(vbm25_read_page_fn read_page, void *ctx, vbm25_growing **out);
/* The sealed documents' `deleted` flags (DocumentTuple.deleted, byte 0 of the tuple; the reference's Bool: != 0), which neither
 * reader of the sealed segment keeps: Meta -> Jump -> the documents tape with vbm25_segment_from_pages' checks and its
 * VBM25_ERR_CORRUPT cases.  Bit d % 64 of words[d / 64] is set for every deleted document d and the other bits of the first
 * ceil(n_docs / 64) words are cleared: DELETED polarity, the form vbm25_index_maintain and vbm25_filter_remap take.
 * *n_docs receives the relation's document count, *n_deleted (may be NULL) the number of flags set.  words == NULL only counts
 * (n_words is not looked at), so the caller can size the buffer; n_words < ceil(n_docs / 64) -> VBM25_ERR_INVALID and nothing
 * written.  NULL read_page or n_docs -> VBM25_ERR_INVALID.  Host only; vbm25_device_vacuum_from_pages (below) reads the same
 * words on the device, for the consumers that take them there. */
int vbm25_sealed_deleted_from_pages(vbm25_read_page_fn read_page, void *ctx, uint64_t *words, uint32_t n_words, uint32_t *n_docs,
                                    uint32_t *n_deleted);
/* Cache key of the HBM copy of a relation's sealed segment: 32 bytes hashed (BLAKE3) over the Meta and Jump
 * tuples.  VACUUM replaces the sealed segment by rewriting the Jump tuple (maintain.rs:268-298: new tape
 * pointers, document count, sum of lengths), REINDEX rewrites Meta (new seed): either changes the fingerprint,
 * and the shim rebuilds its vbm25_index.  Inserts only append to the vectors tape and leave it unchanged
 * (the growing segment is read per query). */
int vbm25_pages_fingerprint(vbm25_read_page_fn read_page, void *ctx, uint8_t *out32);
/* MetaTuple.seed (tuples.rs:48-57): the key of vbm25_intern's hash for this index. */
int vbm25_pages_seed(vbm25_read_page_fn read_page, void *ctx, uint8_t *seed32);

/* intern (vector.rs:19-35): a lexeme -> its 16-byte token key.  Shorter than 16 bytes and without NUL: the
 * bytes, zero padded (seed32 may be NULL).  Otherwise the first 16 bytes of blake3::keyed_hash(seed, lexeme)
 * (blake3 1.8.4; implemented in csrc/blake3.cpp from the specification), last byte forced non-zero. */
int vbm25_intern(const uint8_t *seed32, const uint8_t *string, size_t len, uint8_t *key16);
int vbm25_growing_get_desc(const vbm25_growing *, vbm25_growing_desc *out);
void vbm25_growing_free(vbm25_growing *);

/* ------------------------------------------------------------------------
 * Device side
 * ---------------------------------------------------------------------- */
typedef struct vbm25_index vbm25_index; /* owns the HBM copy of one sealed segment */
typedef struct vbm25_batch vbm25_batch; /* owns query / result buffers for one batch shape */

/* Validates the arrays, uploads them to HBM on `device` (HIP ordinal) and
 * derives the GPU-side structures (per-posting fieldnorm stream, per-term s0,
 * the shared s1[256] table of bm25.rs:340-354). */
int vbm25_index_create(const vbm25_index_desc *desc, int device, vbm25_index **out);
void vbm25_index_destroy(vbm25_index *);
/* HBM bytes held by the index. */
uint64_t vbm25_index_device_bytes(const vbm25_index *);

/* address_tokens::read (address_tokens.rs:61-98) for n keys at once: term id of
 * each 16-byte key, or UINT32_MAX when the token is not in the index (such
 * tokens are ignored by search, search.rs:59-61). */
int vbm25_lookup_terms(const vbm25_index *, const uint8_t *keys, uint32_t n, uint32_t *term_ids);

/* bm25::search for nq queries at once (filter == true, sealed segment only).
 * Query q is term_ids[q_off[q] .. q_off[q+1]), strictly ascending (Query::new,
 * vector.rs:101-110); ids >= n_terms are ignored.  k = bm25.limit (1..=65535,
 * gucs.rs:37-46); k == 0 -> VBM25_ERR_INVALID like default.rs:114-116.
 * hits: nq x k, caller owned; n_hits: nq.  Results per query are best first:
 * score descending, ties by ascending doc id.  Synchronous. */
int vbm25_search_batch(vbm25_index *, const uint32_t *term_ids, const uint32_t *q_off,
                       uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits);

/* Same computation with the batch resident in HBM: create once, upload
 * queries, run (asynchronous on `hip_stream`, NULL = default stream), fetch. */
int vbm25_batch_create(vbm25_index *, uint32_t max_queries, uint32_t max_total_terms, uint32_t k,
                       vbm25_batch **out);
void vbm25_batch_destroy(vbm25_batch *);
/* A failed vbm25_batch_set_queries leaves the batch holding no queries: run enqueues nothing, fetch writes
 * nothing and returns VBM25_OK, and the next successful set_queries works as on a new batch (filter and growing
 * segment stay attached). */
int vbm25_batch_set_queries(vbm25_batch *, const uint32_t *term_ids, const uint32_t *q_off,
                            uint32_t nq);
int vbm25_batch_run(vbm25_batch *, void *hip_stream);
int vbm25_batch_fetch(vbm25_batch *, vbm25_hit *hits, uint32_t *n_hits);
/* Device address of the nq x k vbm25_hit array / the nq counts (valid after run; a batch object whose device
 * addresses were asked for leaves complete records there after EVERY run -- without this call a run may leave a
 * query to vbm25_batch_fetch, which then repeats the scan for it before it returns). */
int vbm25_batch_device_results(vbm25_batch *, void **hits, void **n_hits);
/* When enabled, run() brackets the posting-scan kernel with HIP events on the
 * launch stream; kernel_ms() synchronises and returns the average duration of
 * the launches recorded since the last call. */
int vbm25_batch_set_timing(vbm25_batch *, int enabled);
int vbm25_batch_kernel_ms(vbm25_batch *, double *avg_ms, uint32_t *n_launches);

/* Filtered search: bm25::search's `filter` (search.rs:217-236) for filters that are document sets known before the
 * query runs (deleted documents, a visibility map, one tenant's rows, an evaluated WHERE clause).
 * A filter holds F bitmaps over the index's document ids in HBM on the index's device: bitmap i is ceil(n_docs / 64)
 * uint64_t words, bit d % 64 (counted from the least significant bit) of word d / 64 = 1 means document d may be
 * returned.  Each query names one bitmap by its selector, or UINT32_MAX for none.  The records of a filtered query
 * are byte-identical to the first min(k, n) entries of the unfiltered full ranking with the rejected documents
 * removed (n = matching accepted documents), in the same order; there is no depth limit.  A query with selector
 * UINT32_MAX gets the records vbm25_search_batch gives it.
 *   vbm25_filter_create        words: F x ceil(n_docs / 64), or NULL for all bits zero.  Bits set at or beyond n_docs
 *                              -> VBM25_ERR_INVALID (as in vbm25_filter_update).
 *   vbm25_filter_update        replaces bitmap i from host memory; synchronous (waits for the device first).
 *   vbm25_filter_device_words  device address of bitmap i, for callers that build the bits on the GPU (their work
 *                              must be complete before the next run; bits at or beyond n_docs are never read).
 *   vbm25_filter_destroy       the filter must not be destroyed while a batch refers to it (set its filter to NULL).
 *   vbm25_search_batch_filtered  vbm25_search_batch with q_filter[q] (nq selectors) for query q.
 *   vbm25_batch_set_filter     q_filter: max_queries selectors (query q of every later query set takes entry q);
 *                              the batch keeps filter and selectors until they are set again; NULL filter: none.
 *                              Changed bits (update, device_words) take effect at the next run.
 * A filter of another index, or a selector >= F other than UINT32_MAX -> VBM25_ERR_INVALID.
 * The pipelined ring takes a filter through vbm25_stream_set_filter / vbm25_stream_submit_filtered and the multi-GPU batch through
 * vbm25_multi_batch_set_filter (both below). */
typedef struct vbm25_filter vbm25_filter;
int vbm25_filter_create(vbm25_index *, uint32_t n_bitmaps, const uint64_t *words, vbm25_filter **out);
int vbm25_filter_update(vbm25_filter *, uint32_t i, const uint64_t *words);
int vbm25_filter_device_words(vbm25_filter *, uint32_t i, void **dev);
void vbm25_filter_destroy(vbm25_filter *);
int vbm25_search_batch_filtered(vbm25_index *, const vbm25_filter *, const uint32_t *q_filter,
                                const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, uint32_t k,
                                vbm25_hit *hits, uint32_t *n_hits);
int vbm25_batch_set_filter(vbm25_batch *, const vbm25_filter *, const uint32_t *q_filter);

/* The growing segment on the device: bm25::search's first half (search.rs:83-135), the documents inserted since the last
 * VACUUM, scored on the GPU and merged into the records of a batch.  A device growing segment is uploaded for one index from
 * the CSR of vbm25_growing_desc (vbm25_growing_from_pages / vbm25_growing_get_desc, or assembled by the caller).  For query q
 * the records are byte for byte
 *     vbm25_merge_hits(the records vbm25_search_batch gives q,
 *                      vbm25_growing_search(the index's desc, the keys of q's term ids, k, the growing arrays), k):
 * the sealed segment's statistics score every growing document, elements whose key the sealed segment lacks never score,
 * a document's score is summed in element (= key = term id) order from 0.0, deleted documents are skipped, a document
 * enters only with a score > 0; growing hits rank by (score desc, growing index g asc), doc_id = 0xFFFFFFFF - g with the
 * document's payload; on equal scores sealed hits come first.  Every k of 1 .. 65535 is served.
 *   vbm25_growing_upload       builds the inverted form in HBM on the index's device (synchronous); the caller's arrays are
 *                              not kept.  VBM25_ERR_INVALID: a document whose keys are not strictly ascending
 *                              (vector.rs:56-61), a start array that is not monotone or reaches beyond n_elements,
 *                              n_docs(sealed) + n_docs(growing) > 2^32 (the doc id ranges would collide).
 *   vbm25_device_growing_free  must not be called while a batch refers to the segment (set it to NULL first).
 *   vbm25_device_growing_append  `delta` is a CSR of the NEW documents only, in the form vbm25_growing_upload takes (start may
 *                              begin anywhere): document i of the delta becomes growing document g = n_grow + i.  Afterwards the
 *                              segment searches exactly as an upload of the old documents followed by the delta's would.  Only
 *                              the delta crosses the host link (plus O(n_terms) words back, and once per segment, at its first
 *                              append, the index's term keys); the merge into the term-major postings runs on the device.
 *                              Validation is upload's, applied to the delta (VBM25_ERR_INVALID; the postings the segment holds
 *                              reaching 2^31 -> VBM25_ERR_UNSUPPORTED), and it and every allocation come before anything a search
 *                              reads is changed: a failed append leaves the segment exactly as it was.  An empty delta changes
 *                              nothing.  Synchronous: it waits for the device first, so a run in flight ends on the old arrays.
 *                              The handle and its upload stay the same: a batch that holds the segment sees the new documents at
 *                              its next run with no setter call.  A filter's growing bitmaps are stale after an append (below).
 *   vbm25_device_growing_delete  g[0 .. n): growing indices to drop (any order, repeats and already deleted ones allowed); any
 *                              g[i] >= n_grow -> VBM25_ERR_INVALID and nothing changed.  Afterwards the segment searches as an
 *                              upload with deleted[g] = 1 would; later appends keep the documents deleted.  Their postings stay
 *                              in HBM (scoring nothing) until the next compaction.  Synchronous.  Growing bitmaps stay valid.
 *                              Neither call may run while another host thread runs a batch that holds the segment.
 *   vbm25_device_growing_docs  n_grow now (0 for NULL).
 *   vbm25_device_growing_bytes what the segment has allocated: after an append that includes the second copy of the postings the
 *                              merge writes into and the room to spare of the buffers (they grow geometrically).
 *   vbm25_search_batch_growing   vbm25_search_batch with the growing segment merged in.
 *   vbm25_batch_set_growing    every later run of the batch merges the segment in (NULL detaches: the batch behaves exactly
 *                              as without); vbm25_batch_device_results then points at the merged records, and kernel_ms
 *                              covers the sealed scan through the final merge.
 * A growing segment of another index -> VBM25_ERR_INVALID.  A batch with both a filter and a growing segment needs the filter's
 * growing bitmaps of that segment (below).  vbm25_stream_set_growing and vbm25_multi_batch_set_growing (below) attach a segment to
 * the pipelined ring and to the multi-GPU batch. */
typedef struct vbm25_device_growing vbm25_device_growing;
int vbm25_growing_upload(vbm25_index *, const vbm25_growing_desc *, vbm25_device_growing **out);
/* The device reader of the vectors tape: *out is what vbm25_growing_from_pages + vbm25_growing_get_desc + vbm25_growing_upload(index,
 * ...) give, an ordinary device growing segment on the index's device (searched, appended to, deleted from and attached like any
 * other; every search returns the same records byte for byte), without the host touching a tuple.  The host follows Meta -> Jump ->
 * Jump.ptr_vectors -> Opaque.next (one header check and one copy into pinned staging per page, uploaded in chunks while the walk
 * goes on; read_page is called once per page, from the calling thread); kernels classify the tuples, run the state machine of
 * search.rs:83-135 as scans (an insert that did not reach its _0 is validated and dropped), copy the elements into the CSR's planes
 * and check it (csrc/pages_device.hip, csrc/vectors_parse.h); vbm25_growing_upload's device half builds the segment from there.
 *   csr: NULL, or *csr receives the CSR copied back from the device, byte for byte vbm25_growing_from_pages' six arrays (what
 *   vbm25_index_maintain later takes; vbm25_growing_get_desc, vbm25_growing_free).  With csr == NULL no element array comes back.
 *   Whatever vbm25_growing_from_pages refuses is VBM25_ERR_CORRUPT here, message "data corruption: ... (page N)": with several
 *   damages the first in tape order, inside a tuple in the host reader's order (line pointer, too short, tag, no start, element
 *   range); a refusal of the page walk (unreadable page, page header, special area, page linked twice) may come before a tuple's
 *   on an earlier page.  What the reader accepts and vbm25_growing_upload refuses has upload's code: keys not strictly ascending
 *   -> VBM25_ERR_INVALID naming the first such document, 2^31 elements or more (or 2^31 - 1 tuples) -> VBM25_ERR_UNSUPPORTED,
 *   colliding document ranges -> VBM25_ERR_INVALID.  No HIP device -> VBM25_ERR_DEVICE (no host fallback); NULL index, read_page
 *   or out -> VBM25_ERR_INVALID.  On every refusal *out and *csr are NULL, the HBM and pinned memory of the call is released and
 *   the index and the device are as usable as before.  A tape of pages without tuples is a valid segment of 0 documents.
 *   Synchronous; it uses a stream of its own until the segment's build, which is vbm25_growing_upload's. */
int vbm25_device_growing_from_pages(vbm25_index *index, vbm25_read_page_fn read_page, void *ctx, vbm25_device_growing **out,
                                    vbm25_growing **csr);
void vbm25_device_growing_free(vbm25_device_growing *);
uint64_t vbm25_device_growing_bytes(const vbm25_device_growing *);
int vbm25_device_growing_append(vbm25_device_growing *, const vbm25_growing_desc *delta);
int vbm25_device_growing_delete(vbm25_device_growing *, const uint32_t *g, uint32_t n);
uint32_t vbm25_device_growing_docs(const vbm25_device_growing *);
int vbm25_search_batch_growing(vbm25_index *, const vbm25_device_growing *, const uint32_t *term_ids, const uint32_t *q_off,
                               uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits);
int vbm25_batch_set_growing(vbm25_batch *, const vbm25_device_growing *);

/* Filters on the growing segment: besides its F sealed bitmaps a filter can hold F growing bitmaps for ONE uploaded growing segment.
 * Growing bitmap i is ceil(n_grow / 64) uint64_t words, bit g % 64 (least significant first) of word g / 64 = 1 means growing
 * document g (its position in the uploaded CSR) may be returned.  Query q's selector s names sealed bitmap s AND growing bitmap s;
 * UINT32_MAX filters neither.  For a selector s != UINT32_MAX the records are byte for byte
 *     vbm25_merge_hits(the records vbm25_search_batch_filtered gives q,
 *                      vbm25_growing_search(..., deleted = deleted OR NOT growing bit s of g), k)
 * -- sealed hits first on equal scores, doc_id = 0xFFFFFFFF - g, the sealed segment's statistics, every k of 1 .. 65535.
 *   vbm25_filter_set_growing   words: F x ceil(n_grow / 64), or NULL for all bits zero; a NULL segment removes the growing
 *                              bitmaps.  Synchronous.  Bits at or beyond n_grow, a segment of another index -> VBM25_ERR_INVALID.
 *                              The filter names the segment by its upload (each vbm25_growing_upload is a new one, also at a
 *                              re-used address) and keeps no pointer to it: freeing the segment stays legal, the bitmaps then
 *                              match no segment.  A re-upload needs the bitmaps set again; after an append the bitmaps are stale
 *                              (they cover the n_grow they were set at) until they are set again or extended (deletes leave them valid).
 *   vbm25_filter_extend_growing        after vbm25_device_growing_append: extends the F growing bitmaps to the segment's new document
 *                              count, in place on the device.  The filter must hold growing bitmaps of this upload and n_grow(segment)
 *                              >= the count they cover (else VBM25_ERR_INVALID).  With d = the difference, words = F x ceil(d / 64)
 *                              words: bit j of delta bitmap i belongs to growing document (old count + j); NULL = all zero; bits set at
 *                              or beyond d -> VBM25_ERR_INVALID.  Only the delta crosses the host link: the device ORs it, shifted by
 *                              (old count % 64), into each bitmap's boundary word and writes the words behind it.  The bitmaps have
 *                              room to spare that grows geometrically, so most calls touch the tail words only and a growth step
 *                              re-strides all F bitmaps on the device.  d = 0: VBM25_OK, nothing changes.  Every failure leaves the
 *                              filter exactly as it was.  Synchronous: waits for the device first, so a run in flight ends on the old
 *                              bits.  Afterwards the filter is, for every search, what vbm25_filter_set_growing of the concatenated
 *                              bitmaps would be.  The addresses vbm25_filter_growing_device_words returns may change across the call:
 *                              ask again.
 *   vbm25_filter_update_growing        replaces growing bitmap i from host memory (as vbm25_filter_update).
 *   vbm25_filter_growing_device_words  device address of growing bitmap i (as vbm25_filter_device_words).
 *   (both: VBM25_ERR_INVALID when the filter has no growing bitmaps)
 *   vbm25_search_batch_growing_filtered  vbm25_search_batch_growing with q_filter[q] (nq selectors) for query q.
 * A batch holds a filter and a growing segment together only when the filter's growing bitmaps are that segment's; the second
 * setter (vbm25_batch_set_filter / vbm25_batch_set_growing, either order) returns VBM25_ERR_UNSUPPORTED when the filter has no
 * growing bitmaps and VBM25_ERR_INVALID when they belong to another upload or to another document count (the segment was appended
 * to since).  vbm25_batch_run checks again (the filter's growing bitmaps may have been set, or the segment appended to, since): on
 * a mismatch it returns VBM25_ERR_INVALID, enqueues nothing and leaves the batch as it was. */
int vbm25_filter_set_growing(vbm25_filter *, const vbm25_device_growing *, const uint64_t *words);
int vbm25_filter_update_growing(vbm25_filter *, uint32_t i, const uint64_t *words);
int vbm25_filter_extend_growing(vbm25_filter *, const vbm25_device_growing *, const uint64_t *words);
int vbm25_filter_growing_device_words(vbm25_filter *, uint32_t i, void **dev);
int vbm25_search_batch_growing_filtered(vbm25_index *, const vbm25_device_growing *, const vbm25_filter *,
                                        const uint32_t *q_filter, const uint32_t *term_ids, const uint32_t *q_off,
                                        uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits);

/* The same boundary PIPELINED (the caller hands over host buffers and gets host buffers back, as bm25::search
 * returns a Vec, search.rs:28-36): up to `depth` batches are in flight at once, each on its own stream with its
 * own pinned staging -- the upload of batch n + 1 and the records of batch n - 1 (written straight into pinned memory
 * by the last kernel of its scan) overlap the scan of batch n, and the host never waits for the device between a
 * submit and the matching collect.  One host thread drives a stream object (two threads: two objects).
 *   vbm25_stream_submit   copies the queries into pinned memory and enqueues upload and scan; returns at
 *                         once.  VBM25_ERR_INVALID when `depth` batches are already in flight (collect first).
 *   vbm25_stream_collect  waits for the OLDEST batch in flight and writes its records (nq x k hits, nq counts, in
 *                         submission order -- first in, first out); *nq_out = its number of queries.
 *                         VBM25_ERR_INVALID when nothing is in flight.
 * Records are byte-identical to vbm25_search_batch's.
 *
 * A live table on the ring: a growing segment and a filter can be attached to the ring itself.
 *   vbm25_stream_set_growing    batches submitted afterwards merge the segment in (NULL detaches).
 *   vbm25_stream_set_filter     batches submitted afterwards with vbm25_stream_submit_filtered take their bitmaps from this filter
 *                               (NULL detaches).
 *                               Neither setter waits for anything: a slot of the ring picks up the ring's current segment and filter at
 *                               its next submit, when it is idle; batches in flight finish with what they were submitted with.  A
 *                               segment or filter of another index -> VBM25_ERR_INVALID, and the ring keeps what it had.  A segment or
 *                               filter must not be freed while a batch submitted with it is in flight.
 *   vbm25_stream_submit_filtered  vbm25_stream_submit with q_filter[q] (nq selectors) for query q.  The selectors go up in the slot's
 *                               one staged block beside the queries: a filtered step has the same single upload command.  Without a
 *                               filter set -> VBM25_ERR_INVALID; a selector >= F other than UINT32_MAX -> VBM25_ERR_INVALID.
 *   vbm25_stream_submit         on a ring that holds a filter filters nothing (every selector UINT32_MAX); it still merges an
 *                               attached segment.
 * Pairing, checked at submit with the rules and codes of vbm25_batch_set_filter / vbm25_batch_set_growing: a submit whose selectors
 * name a bitmap while a segment is attached needs the filter's growing bitmaps of that upload and that document count
 * (VBM25_ERR_UNSUPPORTED without growing bitmaps, VBM25_ERR_INVALID for another upload or a stale count after an append).  A refused
 * submit enqueues nothing, leaves vbm25_stream_in_flight as it was and the ring usable.
 * Records: byte for byte what vbm25_search_batch_growing_filtered (with only one of the two attached: _growing, _filtered) returns
 * for the query set against the state at submit time, for every k of 1 .. 65535.  With a segment attached a k <= 1024 step still has
 * no download command: the growing merge writes counts and records into the slot's pinned output.
 * The snapshot rule: vbm25_device_growing_append, _delete, vbm25_filter_update*, vbm25_filter_set_growing and
 * vbm25_filter_extend_growing wait for the device before they change anything.  A batch submitted before such a call is searched
 * against the old state, a batch submitted after it against the new one, whenever they are collected. */
typedef struct vbm25_stream vbm25_stream;
int vbm25_stream_create(vbm25_index *, uint32_t depth, uint32_t max_queries, uint32_t max_total_terms, uint32_t k,
                        vbm25_stream **out);
void vbm25_stream_destroy(vbm25_stream *);
int vbm25_stream_submit(vbm25_stream *, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq);
int vbm25_stream_collect(vbm25_stream *, vbm25_hit *hits, uint32_t *n_hits, uint32_t *nq_out);
int vbm25_stream_set_growing(vbm25_stream *, const vbm25_device_growing *);
int vbm25_stream_set_filter(vbm25_stream *, const vbm25_filter *);
int vbm25_stream_submit_filtered(vbm25_stream *, const uint32_t *q_filter, const uint32_t *term_ids, const uint32_t *q_off,
                                 uint32_t nq);
int vbm25_stream_in_flight(const vbm25_stream *);

/* The Query step on the device (csrc/resolve.hip): cast_tsvector_to_query (src/datatype/tsvector.rs:96-105: intern every lexeme, sort,
 * dedup) followed by the key lookup of bm25::search (search.rs:59-61: keys the index lacks are dropped), for a batch of queries.
 * Lexemes or 16-byte keys in; out comes what every search entry point takes: per query the ascending term ids, as a CSR
 * term_ids / q_off with q_off[0] == 0.  The vocabulary is ascending by key, so the ascending distinct found ids ARE the sorted,
 * de-duplicated, known keys -- array for array what vbm25_intern + sort + dedup + vbm25_lookup_terms + drop gives on the host.
 *
 * A resolver is a ring like vbm25_stream: `depth` (1 .. 16) slots, each with pinned input and output, one HIP stream of its own; no
 * call synchronises the device or touches the index's batches.  It holds the vocabulary's keys in HBM (16 bytes a term, uploaded once
 * at create; vbm25_index_device_bytes does not count them, vbm25_resolver_device_bytes does).  It is valid for ITS index: after a
 * compaction the caller makes a new one.  On several GPUs a resolver on any replica serves all of them, because term ids are the same
 * on every replica.  One host thread drives a resolver (two threads: two resolvers, also on one index).
 *   seed32         MetaTuple.seed (vbm25_pages_seed), copied.  NULL: lexemes that need the hash (16 bytes or more, or a NUL inside) are
 *                  refused at submit, with the words of vbm25_intern's error.
 *   capacities     a batch has at most max_queries queries, max_lexemes lexemes (or keys) and max_bytes lexeme bytes.
 *   submit_lexemes query q = lexemes q_lex[q] .. q_lex[q+1]; lexeme i = bytes[lex_off[i] .. lex_off[i+1]), any length, any alignment.
 *                  Copies the arrays into the slot's pinned block and enqueues; returns at once.
 *   submit_keys    the same from interned keys (16 bytes each): query q = keys q_key[q] .. q_key[q+1].
 *   collect        waits for the OLDEST batch in flight: q_off (nq + 1 entries) and term_ids (q_off[nq] ids; the caller provides room
 *                  for as many as it submitted lexemes); *nq_out = its number of queries.  First in, first out.
 * Refused with VBM25_ERR_INVALID and a message, before anything is enqueued and with the ring unchanged: NULL arguments, q_lex[0] != 0,
 * offsets that are not monotone, counts or bytes over capacity, depth outside 1 .. 16, a lexeme that needs the hash without a seed, a
 * submit on a full ring, a collect on an empty one.  A query may resolve to more ids than a scan takes; the resolver does not judge
 * that, the search entry point refuses it as it always did.
 * Every query of a batch at most 64 lexemes long: one wave a query ranks the ids by cross-lane compares; otherwise a radix sort of
 * (query, id) takes any length.  Both give identical bytes.
 *   vbm25_intern_batch_device   the intern step alone, synchronous, on `device`: keys16 = n_lex x 16 bytes, byte for byte
 *                               vbm25_intern's.  For the documents a shim interns for vbm25_device_growing_append.
 *   vbm25_search_batch_lexemes  resolve, then vbm25_search_batch: bm25::search from the lexemes of tsvectors in one synchronous call.  It
 *                               makes and frees a resolver per call; a caller with many batches keeps one and pipelines it in front of
 *                               vbm25_stream_submit. */
typedef struct vbm25_resolver vbm25_resolver;
int vbm25_resolver_create(vbm25_index *, const uint8_t *seed32, uint32_t depth, uint32_t max_queries, uint32_t max_lexemes,
                          uint64_t max_bytes, vbm25_resolver **out);
void vbm25_resolver_destroy(vbm25_resolver *);
uint64_t vbm25_resolver_device_bytes(const vbm25_resolver *);
int vbm25_resolver_submit_lexemes(vbm25_resolver *, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex, uint32_t nq);
int vbm25_resolver_submit_keys(vbm25_resolver *, const uint8_t *keys16, const uint32_t *q_key, uint32_t nq);
int vbm25_resolver_collect(vbm25_resolver *, uint32_t *term_ids, uint32_t *q_off, uint32_t *nq_out);
int vbm25_resolver_in_flight(const vbm25_resolver *);
int vbm25_intern_batch_device(int device, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off, uint32_t n_lex,
                              uint8_t *keys16);
int vbm25_search_batch_lexemes(vbm25_index *, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off,
                               const uint32_t *q_lex, uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits);

/* bm25::evaluate (evaluate.rs:22-74) for n_docs documents against ONE query on the device: the seq-scan
 * form of `tsvector <&> bm25query` (src/index/operators.rs:22-55), batched.  Everything is in term-id space
 * (vbm25_lookup_terms): q_terms = the query's ids, strictly ascending; ids >= the index's term count (tokens
 * that are not in the index) are ignored.  Document i is the elements doc_start[i] .. doc_start[i+1]: term id
 * (ascending in key order; UINT32_MAX for a key that is not in the index -- it still counts for the document's
 * length) and term frequency (> 0).  scores[i] = sum of idf * tf in query key order, bit-identical to
 * vbm25_evaluate / the reference (idf through the host's libm log).  The SQL operator negates the value. */
int vbm25_evaluate_batch(vbm25_index *, const uint32_t *q_terms, uint32_t n_q_terms, uint32_t n_docs,
                         const uint64_t *doc_start, const uint32_t *doc_term, const uint32_t *doc_tf,
                         double *scores);

/* ------------------------------------------------------------------------
 * Device-resident build (SURVEY 8(f)-1 without the round trip): the sealed segment is encoded in HBM and STAYS there
 * (vbm25_device_segment); vbm25_index_create_from_device makes the index of it with device-to-device copies and
 * device-side derivation -- no posting crosses the PCIe link.  (flush.rs:40-158, io.rs:244-282.)
 *
 * vbm25_device_segment_build: arguments and result of vbm25_segment_build_device, kept on `device`.
 * vbm25_device_segment_synth: the synthetic corpus of vbm25_segment_synth GENERATED on the device (same model, same
 * counter-based generator; the device's log / exp round differently from libm's in a handful of draws per billion, and
 * the head tokens of a Zipf law are drawn in several independent parts per chunk, so the corpus has the same distribution
 * but is not bit for bit the host generator's).
 * vbm25_device_segment_download: the host copy (a vbm25_segment like any other: byte-identical to what the host builder
 * makes of the same mappings).  _token_terms / _query_bytes: as vbm25_segment_synth_token_terms / vbm25_query_bytes.
 * ---------------------------------------------------------------------- */
typedef struct vbm25_device_segment vbm25_device_segment;
int vbm25_device_segment_build(int device, double k1, double b, uint32_t n_docs, const uint32_t *doc_len,
                               const uint16_t *doc_payload, uint32_t n_terms, const uint8_t *term_key,
                               const uint64_t *term_start, const uint32_t *post_doc, const uint32_t *post_tf,
                               vbm25_device_segment **out);
int vbm25_device_segment_synth(const vbm25_synth_params *params, int device, vbm25_device_segment **out);
int vbm25_device_segment_download(const vbm25_device_segment *, vbm25_segment **out);
int vbm25_device_segment_token_terms(const vbm25_device_segment *, const uint32_t *tokens, uint32_t n, uint32_t *term_ids);
uint64_t vbm25_device_segment_query_bytes(const vbm25_device_segment *, const uint32_t *term_ids, uint32_t n_terms, uint32_t k);
int vbm25_device_segment_info(const vbm25_device_segment *, uint32_t *n_docs, uint32_t *n_terms, uint32_t *n_blocks,
                              uint64_t *n_postings);
void vbm25_device_segment_free(vbm25_device_segment *);
/* The device reader: vbm25_segment_from_pages whose result is a device segment on `device` -- the relation's sealed segment read into
 * HBM without a host copy of the index.  Same accept / refuse contract as vbm25_segment_from_pages (Meta -> Jump -> the documents,
 * tokens, summaries and blocks tapes; not the vectors tape, not the address trees, not DocumentTuple.deleted), and
 * vbm25_device_segment_download of the result is byte for byte what vbm25_segment_from_pages returns.  The host follows the page
 * chains (one header check and one copy into pinned staging per page, uploaded in chunks while the walk goes on); every tuple is
 * parsed, validated and flattened by kernels (csrc/pages_device.hip).  read_page is called once per page, from the calling thread;
 * a page image is not read again after the callback for the next page was made.
 *   What vbm25_segment_from_pages refuses as VBM25_ERR_CORRUPT is refused with that code here, message "data corruption: ...
 *   (page N)", and so is everything vbm25_index_create's structural check refuses on the flattened arrays; k1 / b out of range
 *   -> VBM25_ERR_INVALID; no HIP device -> VBM25_ERR_DEVICE (no host fallback); NULL argument -> VBM25_ERR_INVALID.  On every
 *   refusal *out is NULL, the HBM and pinned memory of the call is released and the device is as usable as before.
 *   An empty sealed segment (n_docs == 0) is valid: its index returns nothing.  Synchronous; one host thread. */
int vbm25_device_segment_from_pages(vbm25_read_page_fn read_page, void *ctx, int device, vbm25_device_segment **out);

/* The device writer, the inverse of the device reader: a device segment goes out as the 8192-byte page images flush.rs:40-158
 * writes (tuple layouts: tuples.rs; page layout: PageInit with the 8-byte special area {next, flags = 0}, 4-byte line pointers,
 * tuples MAXALIGNed downwards, every other byte zero).  Kernels compute where every tuple goes and fill the images
 * (csrc/pages_write.hip, csrc/pages_emit.h); the host moves finished images through pinned staging to write_page, 1024 at a time,
 * and assembles the two small address trees.  write_page is called once per page from the calling thread; `image` is valid only
 * during the call; a non-zero return stops the write.
 *   vbm25_device_segment_page_count  the pages flush() allocates for the segment: the documents, tokens, summaries and blocks tapes
 *                                    and both address tapes
 *   vbm25_device_segment_write_pages flush() with its i-th page allocation getting page_ids[i] (page_ids == NULL: first_page + i).
 *                                    Allocation order: the documents tape's first page and its overflow pages; the first pages of
 *                                    the tokens, summaries and blocks tapes; the overflow pages of those three in the order the
 *                                    pushes meet them (per term and block: the block, then its summary; after the term's last
 *                                    block: its token); address_documents (one page at create, one after every tuple: its head ends
 *                                    empty and is free_documents); address_tokens likewise.  *out: what maintain.rs:282-296 /
 *                                    build.rs:49-66 put into the Jump tuple
 *   vbm25_device_segment_write_relation  build.rs:22-71: a whole fresh relation -- the Meta page 0 (k1 and b of the segment, seed32 or
 *                                    zeros), the flush into pages 1 .., the empty vectors tape, the Jump page, the lock page;
 *                                    *n_pages (may be NULL): pages written
 *   VBM25_ERR_INVALID: a NULL segment, callback or output; n_page_ids different from the page count (page_ids != NULL); an id equal
 *   to 0xFFFFFFFF or repeated; first_page + count beyond 2^32 - 1; a callback that returned non-zero (the message names the page).
 *   VBM25_ERR_DEVICE without a gfx950 device: no host fallback.  After any refusal the segment and the device are as usable as
 *   before.  On success every page id was handed to the callback exactly once.  Synchronous; calls on different threads are
 *   independent. */
typedef int (*vbm25_write_page_fn)(void *ctx, uint32_t page_id, const uint8_t *image);
typedef struct vbm25_flushed {
    uint32_t number_of_documents, _pad;
    uint64_t sum_of_document_lengths;
    uint16_t width_1_documents, width_0_documents;
    uint32_t depth_documents, start_documents, free_documents;
    uint32_t depth_tokens, start_tokens, free_tokens;
    uint32_t ptr_documents, ptr_tokens, ptr_summaries, ptr_blocks;
} vbm25_flushed;
int vbm25_device_segment_page_count(const vbm25_device_segment *, uint32_t *n_pages);
int vbm25_device_segment_write_pages(const vbm25_device_segment *, const uint32_t *page_ids, uint32_t n_page_ids, uint32_t first_page,
                                     vbm25_write_page_fn write_page, void *ctx, vbm25_flushed *out);
int vbm25_device_segment_write_relation(const vbm25_device_segment *, const uint8_t *seed32, vbm25_write_page_fn write_page, void *ctx,
                                        uint32_t *n_pages);
/* The index of a device segment, on the segment's device; the segment is left as it was. */
int vbm25_index_create_from_device(const vbm25_device_segment *, vbm25_index **out);

/* VACUUM's compaction (maintain.rs:27-298) on the device: an index, the deletes of its sealed documents and its growing segment
 * become ONE new sealed segment in HBM on the index's device, byte for byte what vbm25_segment_build(k1 and b of the index, ...)
 * makes of the records and mappings maintain.rs writes:
 *   1. sealed documents in id order: a kept document d gets new id = the number of kept sealed documents before d, record
 *      (length 0, its payload); a deleted one gets no id and no record;
 *   2. every posting of a kept sealed document becomes the mapping (token key, new id, tf) and adds 1 to that document's length
 *      (maintain.rs:344-362).  A kept sealed document's new length is therefore the NUMBER OF DISTINCT TOKENS it holds, not the sum
 *      of its tfs: the sealed segment keeps only fieldnorm codes, the real length is gone.  Its fieldnorm code is recomputed from that
 *      count and changes wherever a tf > 1.  This is the reference's behaviour, kept on purpose;
 *   3. the growing documents in desc order: the non-deleted ones get ids n_kept_sealed + 0, 1, ..., record (Document::length() = the
 *      saturating sum of their tfs, payload) (vector.rs:77-83), and every element becomes a mapping, keys the sealed vocabulary lacks
 *      included (they become new tokens).  The desc's fieldnorm array is not read;
 *   4. the mappings sorted by (key, document) and flushed with the index's k1 and b: a token with no mapping left is absent, n_docs
 *      and sum_len are recomputed;
 *   5. nothing left: the empty segment (n_docs 0, no tokens, no blocks), which vbm25_index_create_from_device takes and every search
 *      of returns no hit.  More than 2^32 - 1 documents (io.rs:53-56) -> VBM25_ERR_INVALID.
 * index: any index (host arrays, pages or a device segment, with or without the derived planes); its blob, block metadata,
 *   term_first_block, payloads and keys are read, nothing of it changes and it stays usable.
 * sealed_deleted: NULL (nothing deleted) or ceil(n_docs / 64) words, bit d % 64 of word d / 64 set = sealed document d is DELETED
 *   (DocumentTuple.deleted) -- the opposite polarity of a filter's keep bits.  Bits at or beyond n_docs -> VBM25_ERR_INVALID.
 * growing: NULL or n_docs 0 = no growing documents.  Validated as vbm25_growing_upload does (keys strictly ascending inside a
 *   document, start monotone), and tf 0 is rejected; deleted NULL = none deleted.
 * relabel: NULL, or n_docs(sealed) + n_docs(growing) entries: every old sealed document, then every growing index, -> its new id or
 *   UINT32_MAX (to carry filters and payload maps across).
 * Failure leaves *out NULL and nothing allocated.  The serving loop: compact, vbm25_index_create_from_device, swap the index in,
 * upload an empty growing segment, carry the filters across with vbm25_filter_remap (below; relabel is for what the caller keeps
 * by document id on the host). */
int vbm25_index_maintain(const vbm25_index *index, const uint64_t *sealed_deleted, const vbm25_growing_desc *growing,
                         uint32_t *relabel, vbm25_device_segment **out);

/* Filters across a compaction.  vbm25_filter_remap makes, on the device, the filter of the compacted index out of the filter of
 * the old one: no relabel table and no bitmap crosses the host link, only the two deletion inputs go up.
 *   old: a filter of the index that was compacted, with the growing bitmaps of the growing segment that was compacted in (if
 *     any).  It is only read and stays valid: batches still running on the old index keep using it.
 *   sealed_deleted, growing_deleted: the SAME deletion inputs vbm25_index_maintain got -- NULL or ceil(n_docs / 64) words, DELETED
 *     polarity; NULL or n_grow bytes (vbm25_growing_desc.deleted), nonzero = deleted.  The relabel is the monotone compaction the
 *     two define.  n_grow: the growing documents the compaction took (0: none, the filter's growing bitmaps are then ignored).
 *   new_index: the index made of the compacted segment (vbm25_index_create_from_device, or a replica of
 *     vbm25_multi_create_from_device), on the old filter's device.
 * *out: a new filter on new_index with the same number of bitmaps.  Its bitmap i is two bit runs back to back: old sealed bitmap
 * i's bits of the kept sealed documents in id order, then old growing bitmap i's bits of the live growing documents in growing
 * order -- in the filter's own packing (bit d % 64 of word d / 64, least significant first), bits at or beyond the new n_docs
 * zero.  It has no growing bitmaps: the caller sets them for the fresh growing segment as usual.
 * Synchronous: waits for the device before it reads.  On any failure *out is NULL and nothing is allocated:
 *   NULL old, new_index or out; new_index on another device; sealed_deleted bits at or beyond the old n_docs -> VBM25_ERR_INVALID
 *   n_grow > 0 and old has no growing bitmaps -> VBM25_ERR_UNSUPPORTED; they cover another document count -> VBM25_ERR_INVALID
 *   kept sealed + live growing documents != new_index's n_docs (another compaction's index) -> VBM25_ERR_INVALID
 * A new index of 0 documents is valid: a filter of zero words.
 * vbm25_filter_read copies a bitmap back to the host (checkpoints of bitmaps only ever extended on the device): growing == 0:
 * sealed bitmap i, ceil(n_docs / 64) words; growing != 0: growing bitmap i, ceil(covered documents / 64) words
 * (VBM25_ERR_INVALID when the filter has none).  Synchronous. */
int vbm25_filter_remap(const vbm25_filter *old, const uint64_t *sealed_deleted, uint32_t n_grow, const uint8_t *growing_deleted,
                       vbm25_index *new_index, vbm25_filter **out);
int vbm25_filter_read(const vbm25_filter *, uint32_t i, int growing, uint64_t *words);

/* VACUUM's inputs read on the device.  A vbm25_device_vacuum holds a relation's compaction inputs in HBM on the index's device: the
 * sealed documents' deleted flags as ceil(n_docs / 64) words in DELETED polarity (what vbm25_sealed_deleted_from_pages gives, bits at
 * or beyond n_docs zero) and the growing segment's CSR (what vbm25_growing_from_pages gives: the six arrays of vbm25_growing_desc,
 * keys the sealed vocabulary lacks included).  It is only ever read, with one exception: vbm25_device_vacuum_bulkdelete (below) sets
 * deletion flags in it and must not run beside a compaction or a remap that reads the handle.  Otherwise one handle serves any number
 * of compactions and remaps.
 *   vbm25_device_vacuum_from_pages   index: the resident index of the relation's sealed segment (its device, its document count).
 *     The host reads Meta and Jump once and follows the documents tape, then the vectors tape, by Opaque.next: one header check and
 *     one copy into pinned staging per page, uploaded in chunks while the walk goes on; read_page is called once per page, from the
 *     calling thread, and no tuple is touched on the host.  Kernels read byte 0 of every DocumentTuple (!= 0: deleted) into the words
 *     and build the CSR as vbm25_device_growing_from_pages does (no vbm25_device_growing is made).  Refusals, in this order:
 *       1. what vbm25_sealed_deleted_from_pages refuses on this relation, with its code and its message ("data corruption: ... (page
 *          N)"): with several damages the first in tape order, a refusal of the page walk after the tuples in front of it;
 *       2. what vbm25_device_growing_from_pages refuses, in its documented order and with its codes;
 *       3. a Jump document count different from the index's -> VBM25_ERR_INVALID (the index of another relation).
 *     NULL index, read_page or out -> VBM25_ERR_INVALID; no HIP device -> VBM25_ERR_DEVICE (no host fallback).  On any failure *out
 *     is NULL, nothing stays allocated, and the index and the device are as usable as before.  Synchronous, on a stream of its own.
 *   vbm25_device_vacuum_info   the counts (any pointer may be NULL): sealed documents and how many are deleted, growing documents
 *     and how many are deleted, the CSR's elements.  No device work.
 *   vbm25_device_vacuum_read   the two deletion inputs copied back (checkpoints, tests): ceil(n_sealed / 64) words and n_grow bytes;
 *     either pointer may be NULL.  The CSR itself comes back through vbm25_device_growing_from_pages(..., csr).
 *   vbm25_device_vacuum_free   NULL is a no-op.
 *   vbm25_index_maintain_device   vbm25_index_maintain(index, words, desc, relabel, out) with words and desc taken from the handle:
 *     the same segment and relabel, byte for byte, and the same refusals (tf 0 -> VBM25_ERR_INVALID "growing document %u: tf 0"
 *     naming the first such document: the reader accepts tf 0, the compaction does not; more than 2^32 - 1 documents; more than 2^32
 *     tokens); the empty result is the empty segment.  The kernels read the handle's planes in place: nothing proportional to the
 *     documents or the elements crosses the host link (the index's term keys go up; the new vocabulary's keys, starts and block
 *     boundaries, O(terms), come down and go up as in vbm25_index_maintain; relabel when asked for).  A handle of another document
 *     count or on another device -> VBM25_ERR_INVALID.
 *   vbm25_filter_remap_device   vbm25_filter_remap(old, words, n_grow, growing_deleted, new_index, out) with the three deletion
 *     arguments taken from the handle: same words, codes and failure behaviour; no array crosses the host link (two counts come down).
 * The VACUUM loop is then: vbm25_device_vacuum_from_pages, vbm25_index_maintain_device, vbm25_device_segment_write_pages,
 * vbm25_index_create_from_device, vbm25_filter_remap_device. */
typedef struct vbm25_device_vacuum vbm25_device_vacuum;
int vbm25_device_vacuum_from_pages(vbm25_index *index, vbm25_read_page_fn read_page, void *ctx, vbm25_device_vacuum **out);
int vbm25_device_vacuum_info(const vbm25_device_vacuum *, uint32_t *n_sealed, uint32_t *n_sealed_deleted, uint32_t *n_grow,
                             uint32_t *n_grow_deleted, uint64_t *n_elements);
int vbm25_device_vacuum_read(const vbm25_device_vacuum *, uint64_t *sealed_deleted_words, uint8_t *growing_deleted);
void vbm25_device_vacuum_free(vbm25_device_vacuum *);
int vbm25_index_maintain_device(const vbm25_index *index, const vbm25_device_vacuum *in, uint32_t *relabel, vbm25_device_segment **out);
int vbm25_filter_remap_device(const vbm25_filter *old, const vbm25_device_vacuum *in, vbm25_index *new_index, vbm25_filter **out);

/* TID sets (csrc/tid.hip): which documents does a set of heap rows refer to?  bulkdelete.rs:20-112 calls callback(payload) for every
 * growing and every sealed document and search.rs:122,230 filter(payload) the same way; what PostgreSQL holds in both cases is a set
 * of TIDs (VACUUM's dead-TID store, the TID bitmap of a bitmap heap scan).  A vbm25_tid_set keeps such a set in the HBM of one device
 * as sorted distinct 48-bit keys -- payload[0] << 32 | payload[1] << 16 | payload[2], so ascending keys are ascending ctids
 * (fetcher.rs:218-232) -- with a directory of evenly spaced keys; one kernel answers, for every document of a payload plane, one bit
 * in the packing of the filters and the deletion words (bit d % 64 of word d / 64), a wave of 64 lanes one word with one ballot.
 *   vbm25_tid_set_create   tids: n x 3 uint16_t in any order, repeats allowed; uploaded, packed, sorted and de-duplicated on the
 *             device.  n == 0 is a valid empty set that matches nothing (tids may then be NULL).  n > 2^32 - 1 -> VBM25_ERR_UNSUPPORTED,
 *             checked before tids is read or anything is allocated; NULL out, or NULL tids with n > 0 -> VBM25_ERR_INVALID; no HIP
 *             device -> VBM25_ERR_DEVICE.  A failure leaves *out NULL and nothing allocated.  Synchronous.  The set is only ever read
 *             afterwards: one set serves any number of calls and threads.
 *   vbm25_tid_set_info     the distinct TIDs and the device (either pointer may be NULL).
 *   vbm25_tid_set_read     the distinct TIDs back on the host, n_unique x 3, ascending.
 *   vbm25_tid_set_device_bytes   what the set holds of the device (0 for NULL).
 *   vbm25_tid_set_free     NULL is a no-op.
 *   vbm25_tid_set_match_index / _match_growing   words: host memory for ceil(n / 64) words over the index's n_docs sealed documents
 *             (the segment's n_grow growing documents); bit = 1: the document's payload is in the set; bits at or beyond n are zero.
 *             *n_match: the documents matched.  Either output pointer may be NULL.  A growing document's payload is matched whether
 *             or not the document is deleted.  0 documents give zero words and VBM25_OK.  A set on another device than the index's
 *             (the segment's) -> VBM25_ERR_INVALID.  Synchronous.
 *   vbm25_filter_set_tids  sealed bitmap i becomes the match words of the filter's index, complemented below n_docs when invert != 0:
 *             exactly what vbm25_filter_update(f, i, words) with those words would leave, and no bitmap crosses the host link.
 *             gs == NULL: the growing bitmaps are untouched.  gs != NULL: growing bitmap i is set likewise from the segment's
 *             payloads (bits at or beyond n_grow stay zero); the filter must hold growing bitmaps of that upload at its current
 *             document count, else the codes of vbm25_batch_set_filter: VBM25_ERR_UNSUPPORTED without growing bitmaps,
 *             VBM25_ERR_INVALID for another upload or a stale count after an append.  i >= the filter's bitmaps, or a set on another
 *             device -> VBM25_ERR_INVALID.  Every refusal leaves both bitmaps as they were.  Synchronous: it waits for the device
 *             first, as vbm25_filter_extend_growing does.
 *   vbm25_device_growing_delete_tids   afterwards the segment searches exactly as after vbm25_device_growing_delete of every g whose
 *             payload is in the set.  *n_match (may be NULL): the documents matched -- the device does not know which of them were
 *             deleted already, so this is not the number of documents newly deleted.  Synchronous; the threading rule of
 *             vbm25_device_growing_delete.  A set on another device -> VBM25_ERR_INVALID.
 *   vbm25_device_vacuum_bulkdelete   bulkdelete.rs on the handle: the sealed deleted words |= the match of index's payloads, the
 *             growing deleted flags |= the match of the handle's growing payloads; the handle's counts follow.  *n_sealed_new /
 *             *n_grow_new (either may be NULL): the documents that were live before and are deleted now (the reference skips tuples
 *             already deleted).  index must be the one the handle was read for: another device or document count ->
 *             VBM25_ERR_INVALID, as is a set on another device; a refusal leaves the handle as it was.  Every allocation comes
 *             before the first word changes.  Afterwards vbm25_device_vacuum_read, _info, vbm25_index_maintain_device and
 *             vbm25_filter_remap_device see the new flags.  The one call that writes a vbm25_device_vacuum: it must not run beside
 *             a compaction or a remap that reads the handle.  The flags are not written back into page images. */
typedef struct vbm25_tid_set vbm25_tid_set;
int vbm25_tid_set_create(int device, const uint16_t *tids, uint64_t n, vbm25_tid_set **out);
int vbm25_tid_set_info(const vbm25_tid_set *, uint64_t *n_unique, int *device);
int vbm25_tid_set_read(const vbm25_tid_set *, uint16_t *tids);
uint64_t vbm25_tid_set_device_bytes(const vbm25_tid_set *);
void vbm25_tid_set_free(vbm25_tid_set *);
int vbm25_tid_set_match_index(const vbm25_tid_set *, const vbm25_index *, uint64_t *words, uint32_t *n_match);
int vbm25_tid_set_match_growing(const vbm25_tid_set *, const vbm25_device_growing *, uint64_t *words, uint32_t *n_match);
int vbm25_filter_set_tids(vbm25_filter *, uint32_t i, const vbm25_tid_set *, int invert, const vbm25_device_growing *gs);
int vbm25_device_growing_delete_tids(vbm25_device_growing *, const vbm25_tid_set *, uint32_t *n_match);
int vbm25_device_vacuum_bulkdelete(vbm25_device_vacuum *, const vbm25_index *, const vbm25_tid_set *, uint32_t *n_sealed_new,
                                   uint32_t *n_grow_new);

/* ------------------------------------------------------------------------
 * Several GPUs of one node: independent queries shard
 * across the devices, the index is replicated.  vbm25_multi_create uploads the
 * flattened segment to devices[0] ONCE and makes the other replicas GPU to GPU
 * (hipMemcpyPeerAsync over xGMI, derived arrays included; a device may be
 * listed more than once).  A batch is cut into contiguous, balanced shards --
 * the first nq % n devices get one query more --, every device searches its
 * shard on its own stream, and the 24-byte hit records go from every device
 * straight into the caller's host arrays in query order (the caller is the
 * host: a device-side gather would only add a hop).  Same results, record for
 * record, as vbm25_search_batch on one device.  Every device has its own host
 * thread inside the library (they belong to the vbm25_multi); a handle may be
 * used from one thread at a time, and calls on DIFFERENT vbm25_multi_batch
 * objects of one vbm25_multi from several threads are serialised by the library.
 * ---------------------------------------------------------------------- */
typedef struct vbm25_multi vbm25_multi;
typedef struct vbm25_multi_batch vbm25_multi_batch;
int vbm25_multi_create(const vbm25_index_desc *desc, const int *devices, int n_devices,
                       vbm25_multi **out);
/* The replicas of a device segment (a compacted one: vbm25_index_maintain): the first is vbm25_index_create_from_device on the
 * segment's device -- devices[0] must be that device, else VBM25_ERR_INVALID --, the others are copied from it GPU to GPU; the segment
 * is left as it was and nothing goes through the host.  The handle is a vbm25_multi like any other.  After a compaction: compact
 * replica 0, make the new vbm25_multi of the device segment, vbm25_filter_remap per replica against vbm25_multi_index(new, i),
 * upload empty growing segments, destroy the old handle. */
int vbm25_multi_create_from_device(const vbm25_device_segment *, const int *devices, int n_devices, vbm25_multi **out);
void vbm25_multi_destroy(vbm25_multi *);
int vbm25_multi_device_count(const vbm25_multi *);
/* The replica on devices[i] (borrowed: e.g. for vbm25_lookup_terms, which is the same on every replica). */
int vbm25_multi_index(vbm25_multi *, int i, vbm25_index **out);
/* bm25::search for nq queries, sharded; arguments and results as vbm25_search_batch.  Synchronous. */
int vbm25_multi_search_batch(vbm25_multi *, const uint32_t *term_ids, const uint32_t *q_off,
                             uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits);
/* The same with the shards resident on their devices: create once, set the queries, run (asynchronous:
 * every device's scan and the download of its records are enqueued on that device's stream), fetch (waits for
 * all devices and fills the caller's arrays).  run may be repeated. */
int vbm25_multi_batch_create(vbm25_multi *, uint32_t max_queries, uint32_t max_total_terms, uint32_t k,
                             vbm25_multi_batch **out);
void vbm25_multi_batch_destroy(vbm25_multi_batch *);
/* A failed vbm25_multi_batch_set_queries leaves every shard holding no queries, as vbm25_batch_set_queries does. */
int vbm25_multi_batch_set_queries(vbm25_multi_batch *, const uint32_t *term_ids, const uint32_t *q_off,
                                  uint32_t nq);
/* A live table on several GPUs: the caller builds one growing segment and one filter PER REPLICA, on vbm25_multi_index(m, i), and
 * hands over the arrays of handles (one entry per replica; a NULL array detaches).  Entry i must belong to replica i's index: otherwise
 * VBM25_ERR_INVALID and nothing changes on any replica.  The pairing rules and codes are vbm25_batch_set_growing's and
 * vbm25_batch_set_filter's, applied per replica, before anything changes.
 *   vbm25_multi_batch_set_growing  every later run merges replica i's segment into shard i's records.
 *   vbm25_multi_batch_set_filter   q_filter: max_queries selectors (query q of every later query set takes entry q; a selector must
 *                                  be below every filter's bitmap count or UINT32_MAX).  The selectors are cut by the same shard bounds
 *                                  as the queries when vbm25_multi_batch_set_queries fixes nq, and travel with the shard's queries: a
 *                                  filter takes effect at the next vbm25_multi_batch_set_queries.  A NULL array removes the filter at
 *                                  once.
 * vbm25_multi_batch_set_queries and vbm25_multi_batch_run check the growing bitmaps again (VBM25_ERR_INVALID after an append without
 * an extend).  Records are byte-identical to vbm25_search_batch_growing_filtered on one device. */
int vbm25_multi_batch_set_growing(vbm25_multi_batch *, const vbm25_device_growing *const *per_device);
int vbm25_multi_batch_set_filter(vbm25_multi_batch *, const vbm25_filter *const *per_device, const uint32_t *q_filter);
int vbm25_multi_batch_run(vbm25_multi_batch *);
int vbm25_multi_batch_fetch(vbm25_multi_batch *, vbm25_hit *hits, uint32_t *n_hits);

/* The Document step on the device (csrc/cast.hip): cast_tsvector_to_document (src/datatype/tsvector.rs:84-94: intern every lexeme, sort
 * the elements by key, sum equal keys saturating) for a batch of tsvectors, the result kept in the HBM of `device` -- what ambuild
 * (am_build.rs:722) and aminsert (am/mod.rs:284) make of a tuple before anything else happens to it.
 *   input     document i = lexemes doc_lex[i] .. doc_lex[i+1]; lexeme j = bytes[lex_off[j] .. lex_off[j+1]), any length, any alignment,
 *             with lex_count[j] positions (vbm25_resolver_submit_lexemes' packing plus the counts).  Repeated lexemes in a document and
 *             lexemes whose keys collide are allowed.  doc_payload: n_docs x 3, or NULL for documents nobody will index or append.
 *   result    byte for byte the reference's: key = intern(seed, lexeme); a document's elements strictly ascending in memcmp order of
 *             the key; equal keys merged, tf = the saturating u32 sum; length = the saturating u32 sum of the tfs (vector.rs:76-83);
 *             fieldnorm = length_to_fieldnorm(length).  A document without lexemes is kept, with 0 elements and length 0.
 *   download  the arrays as a vbm25_growing (vbm25_growing_get_desc: start, key, tf, fieldnorm, payload -- NULL when none was given --,
 *             deleted all 0: a legal vbm25_growing_desc) and, when doc_len is not NULL, the n_docs lengths.
 * Refused before anything is enqueued, *out == NULL: VBM25_ERR_INVALID for a NULL argument, doc_lex[0] != 0, offsets that are not
 * monotone, a lexeme with count 0 (the message names the first; the reference panics there) and a lexeme that needs the hash when
 * seed32 == NULL (vbm25_intern's words); VBM25_ERR_UNSUPPORTED for 2^31 lexemes or 2^31 - 1 documents or more; VBM25_ERR_DEVICE without a HIP
 * device (there is no host fallback).  n_docs == 0 gives a valid handle of 0 documents.
 * Synchronous, on a stream of the call's own: it issues no device-wide synchronisation and touches no index; freeing its staging
 * and scratch at return does wait for the device's other streams, as every hipFree does.  Two threads may cast at once.  Per document one of three sorts, by its number of lexemes: one wave (<= 64), one workgroup in LDS (<= 2048), radix
 * passes (any length); all three give identical bytes.
 *   vbm25_device_segment_build_documents   what ambuild + io.rs + flush.rs make of the documents: document i becomes doc id i, the
 *             vocabulary is the distinct keys ascending, every element a mapping.  The result is the device segment
 *             vbm25_device_segment_build makes of the same vocabulary and mappings; no posting crosses the host link.
 *             VBM25_ERR_INVALID for a handle without payloads or of 0 documents; k1, b and the rest as the encode refuses them.
 *   vbm25_device_growing_append_documents  vbm25_device_growing_append with the delta read from the handle's arrays in HBM: the same
 *             result, refusals and guarantee (a failed append leaves the segment as it was; a handle of 0 documents changes
 *             nothing).  VBM25_ERR_INVALID for a handle on another device than the segment's or without payloads. */
typedef struct vbm25_documents vbm25_documents;
int vbm25_documents_cast(int device, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *lex_count,
                         const uint32_t *doc_lex, uint32_t n_docs, const uint16_t *doc_payload, vbm25_documents **out);
int vbm25_documents_info(const vbm25_documents *, uint32_t *n_docs, uint64_t *n_elements, int *device);
int vbm25_documents_download(const vbm25_documents *, vbm25_growing **csr, uint32_t *doc_len);
uint64_t vbm25_documents_device_bytes(const vbm25_documents *);
void vbm25_documents_free(vbm25_documents *);
int vbm25_device_segment_build_documents(const vbm25_documents *, double k1, double b, vbm25_device_segment **out);
int vbm25_device_growing_append_documents(vbm25_device_growing *, const vbm25_documents *);

/* A caster (csrc/cast.hip): the Document step as a ring that keeps everything a cast needs between calls, modelled on the resolver.
 * `depth` slots (1 .. 16), each with its own non-blocking stream, two events, a pinned staging block, its device scratch and its
 * result arrays, all allocated by vbm25_caster_create for the capacities given there: batches of up to max_docs documents,
 * max_lexemes lexemes and max_bytes lexeme bytes, of which up to max_long_lexemes lexemes may sit in documents of the general class
 * (more than 2048 lexemes; it sizes the radix scratch, 0 = none).  One host thread drives a caster; several casters, and a caster
 * beside any other handle, may run at once.  submit, collect, info and in_flight issue no device-wide synchronisation; create and
 * free allocate and free device and pinned memory, which waits for the device's other streams, as every hipMalloc and hipFree may.
 *   device bytes   per slot, with D = max_docs, L = max_lexemes, B = max_bytes, G = max_long_lexemes; the staged input is one
 *             array whose nine parts are each rounded up to a multiple of 16, every other term is an array of exactly that size:
 *             staged input   4(D+1) + 8(L+1) + 4L + 4D + 4(D+1) + 1024 + 6D + 8D + B
 *             scratch        16L (keys) + 16L + 4L (survivors) + 4(D+1) (counts) + hipcub's temporary storage
 *                            + (G > 0: 44G + 4) (the general class)
 *             results        8(D+1) + 16L + 4L + 4D + D + 6D
 *             vbm25_caster_device_bytes = depth x that sum (0 for NULL); the pinned host block is the staged input's size.
 *   vbm25_caster_info      depth, device and `allocations`: every allocation and creation (device, pinned, stream, event) the handle
 *             has made.  It does not move after create: submit and collect allocate, create and free nothing.
 *   vbm25_caster_submit    vbm25_documents_cast's input (the seed is the caster's).  Every refusal of that call comes first and in the
 *             same words; then VBM25_ERR_INVALID for a full ring and for documents, lexemes, bytes or general-class lexemes over the
 *             capacities, VBM25_ERR_UNSUPPORTED with max_long_lexemes == 0 for a batch with a document of the general class (the
 *             message names the first).  A refused submit enqueues nothing and leaves the ring as it was.  Otherwise the input is
 *             copied into the slot's pinned block (the caller's arrays are free at return), the batch is enqueued and the call
 *             returns.  There is no wait in the middle: the slot's key / tf arrays have room for max_lexemes elements, and the
 *             number of elements comes home with the batch.
 *             The wave class (documents of <= 64 lexemes) is packed: the host plans runs of consecutive such documents with at
 *             most 64 lexemes and 64 documents a run, one wave takes a run, one lane a lexeme; a key in two documents of a run
 *             never merges.  A batch without a longer document interns its lexemes in the same lanes.
 *   vbm25_caster_collect   waits for the oldest batch, first in first out, and hands out a vbm25_documents that belongs to its slot,
 *             with n_docs, n_elements and has_payload of that batch.  Everything that takes a const vbm25_documents * takes it;
 *             vbm25_documents_free on it does nothing.  Valid until the submit that takes its slot again -- `depth` submits
 *             after its own -- or vbm25_caster_free.  Its bytes are vbm25_documents_cast's for the same input, array for array.
 *             VBM25_ERR_INVALID, *out == NULL, on an empty ring.
 *   vbm25_caster_in_flight   batches submitted and not collected (0 for NULL).
 *   vbm25_caster_free      waits for what is in flight, then frees everything.
 *   vbm25_documents_extend appends src's documents behind dst's on the device (start rebased by a kernel, the other arrays copied
 *             device to device), so a bulk load cast in chunks still ends in one handle.  dst is an owned handle (a
 *             vbm25_documents_cast of 0 documents makes an empty one, with or without payloads); its arrays grow geometrically.
 *             The result equals one cast of the concatenated input.  Refused, dst as it was: VBM25_ERR_INVALID for a NULL
 *             argument, dst == src, a dst that belongs to a caster, different devices, one handle with payloads and one without;
 *             VBM25_ERR_UNSUPPORTED for 2^31 - 1 documents or 2^31 elements or more in the sum. */
typedef struct vbm25_caster vbm25_caster;
int vbm25_caster_create(int device, const uint8_t *seed32, uint32_t depth, uint32_t max_docs, uint32_t max_lexemes,
                        uint64_t max_bytes, uint32_t max_long_lexemes, vbm25_caster **out);
void vbm25_caster_free(vbm25_caster *);
uint64_t vbm25_caster_device_bytes(const vbm25_caster *);
int vbm25_caster_info(const vbm25_caster *, uint32_t *depth, int *device, uint64_t *allocations);
int vbm25_caster_submit(vbm25_caster *, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *lex_count,
                        const uint32_t *doc_lex, uint32_t n_docs, const uint16_t *doc_payload);
int vbm25_caster_collect(vbm25_caster *, const vbm25_documents **out);
int vbm25_caster_in_flight(const vbm25_caster *);
int vbm25_documents_extend(vbm25_documents *dst, const vbm25_documents *src);

/* The `<&>` operator from cast documents (csrc/evaluate.hip): bm25::evaluate (evaluate.rs:22-74) for a batch of queries, each
 * against its own list of candidate documents -- the reranking form of `tsvector <&> bm25query` (src/index/operators.rs:22-55) --
 * with the documents read from HBM.  Two steps.
 *   vbm25_documents_bind   the handle's keys looked up in ONE index's vocabulary, which that index's resolver already keeps in HBM
 *             (nothing is uploaded): per document the ascending term ids of the elements the vocabulary holds, with their tfs, and
 *             the fieldnorm code the cast gave the document (elements the vocabulary lacks count for the length and never score).
 *             The bound handle refers to the resolver's index, which must outlive it; the resolver and the vbm25_documents may be
 *             freed after the bind.  It is valid for that index only: after a compaction the caller binds again.  A handle of 0
 *             documents binds to a valid handle of 0 documents.  VBM25_ERR_INVALID, *out == NULL, nothing enqueued: NULL arguments,
 *             a handle and a resolver on different devices.
 *   info / download        n_docs, n_known (the elements kept) and the device; start (n_docs + 1 entries), term and tf (n_known
 *             each; either may be NULL when n_known is 0) copied to the host.
 *   vbm25_evaluate_documents   queries as the CSR term_ids / q_off every search entry point takes (vbm25_resolver_collect's output):
 *             per query the ids strictly ascending, ids >= the index's term count ignored.  Query q scores the documents
 *             cand_doc[q_cand[q] .. q_cand[q+1]) -- indices into the handle, any order, repeats allowed -- and scores is aligned
 *             with cand_doc.  q_cand == NULL: every query scores every document, scores is nq x n_docs, row-major.
 *             scores[i] is bit for bit what vbm25_evaluate returns for the pair (the document's keys and tfs as
 *             vbm25_documents_download gives them, the query's keys): the sum, in query key order, of
 *             idf * ((tf * (k1 + 1)) / (tf + s1[fieldnorm])) over the query's terms the document holds, with the idf and s1 tables of
 *             vbm25_evaluate_batch.  The SQL operator negates the value; the library does not.
 *             VBM25_ERR_INVALID with a message that names the first offender, before anything is enqueued: NULL term_ids, q_off or
 *             scores (nq > 0), q_off[0] != 0 or q_cand[0] != 0, offsets that are not monotone, cand_doc NULL while q_cand is not, a
 *             query whose ids do not ascend strictly, a candidate >= n_docs, an index without sealed documents.
 *             VBM25_ERR_UNSUPPORTED for 2^31 pairs or more.  nq == 0 and queries without candidates are legal and write nothing.
 * Both calls are synchronous, each on a stream of its own: no device-wide synchronisation is issued (freeing the call's buffers
 * at return waits for the device's other streams, as every hipFree does).  The handle is only read: two threads may score on one
 * handle at once.  One wave scores 64 candidates of one query; a lane finds each query term in its document's id run by bisection. */
typedef struct vbm25_doc_terms vbm25_doc_terms;
int vbm25_documents_bind(const vbm25_documents *, const vbm25_resolver *, vbm25_doc_terms **out);
int vbm25_doc_terms_info(const vbm25_doc_terms *, uint32_t *n_docs, uint64_t *n_known, int *device);
int vbm25_doc_terms_download(const vbm25_doc_terms *, uint64_t *start, uint32_t *term, uint32_t *tf);
uint64_t vbm25_doc_terms_device_bytes(const vbm25_doc_terms *);
void vbm25_doc_terms_free(vbm25_doc_terms *);
int vbm25_evaluate_documents(const vbm25_doc_terms *, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq,
                             const uint64_t *q_cand, const uint32_t *cand_doc, double *scores);

/* The rerank step (csrc/rerank.hip): a scorer handle over bound documents that keeps everything a scoring call needs between calls,
 * and the `<&>` scores cut to each query's k best on the device -- `ORDER BY doc <&> query LIMIT k` over a candidate list.
 *   vbm25_scorer_create    a handle on the vbm25_doc_terms, which must outlive it.  It owns one non-blocking stream, its events, one
 *             pinned staging block and its device buffers; these grow geometrically when a call needs more and are freed by
 *             vbm25_scorer_free only: a call of a shape already seen, or a smaller one, allocates and creates nothing.  A call's
 *             inputs travel in one staged block with one upload, its results come back through the pinned block; no device-wide
 *             synchronisation is issued.  A mutex inside serialises the calls on one scorer; several scorers on one
 *             vbm25_doc_terms may run at once.  A call that fails leaves the scorer usable.  VBM25_ERR_INVALID for NULL arguments.
 *   vbm25_scorer_device_bytes   what the handle holds of the device now (0 for NULL).
 *   vbm25_scorer_evaluate  vbm25_evaluate_documents through the handle: the same arguments, checks, messages and bits.
 *   vbm25_scorer_topk      the same inputs and checks, then k: 0 is VBM25_ERR_INVALID, more than 1024 VBM25_ERR_UNSUPPORTED (the limit
 *             of the search's general path); NULL ranks or n_ranks (nq > 0) are refused as NULL scores are.  Every refusal comes
 *             before anything is enqueued.  Every entry of query q's candidate list is eligible, zero scores and repeated documents
 *             included (q_cand == NULL: every document of the handle).  n_ranks[q] = min(k, candidates of q); ranks is nq x k,
 *             row-major, row q best first: score descending, then pos ascending.  pos is the entry's index within q's own list
 *             (from q_cand[q]; the document index without q_cand), doc the handle's document index, score bit for bit what
 *             vbm25_evaluate_documents gives the pair; entries at and beyond n_ranks[q] are all-zero bytes.  The rows equal a
 *             stable descending sort of vbm25_evaluate_documents' scores cut at k.  The scores themselves never reach HBM: each
 *             workgroup scores a part of one query's candidates and keeps the k best in LDS. */
typedef struct vbm25_rank { double score; uint32_t pos; uint32_t doc; } vbm25_rank;   /* 16 bytes */
typedef struct vbm25_scorer vbm25_scorer;
int vbm25_scorer_create(const vbm25_doc_terms *, vbm25_scorer **out);
void vbm25_scorer_free(vbm25_scorer *);
uint64_t vbm25_scorer_device_bytes(const vbm25_scorer *);
int vbm25_scorer_evaluate(vbm25_scorer *, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                          const uint32_t *cand_doc, double *scores);
int vbm25_scorer_topk(vbm25_scorer *, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                      const uint32_t *cand_doc, uint32_t k, vbm25_rank *ranks, uint32_t *n_ranks);

/* The reranker (csrc/reranker.hip): the rerank step as a ring, modelled on the resolver and the caster.  Lexeme queries (or term ids)
 * and candidate lists -- document indices, ctids, or none for the cross product -- go in; each query's k best rows come out, first in
 * first out, byte for byte what vbm25_resolver_submit_lexemes / _collect followed by vbm25_scorer_topk give.  Between submit and
 * collect the host touches nothing: the resolved ids stay in HBM, and ctids are mapped to document indices on the device.
 *   vbm25_reranker_create   `depth` slots (1 .. 16) on the vbm25_doc_terms, with the vocabulary and the seed of the resolver (nothing is
 *             uploaded again; both must outlive the reranker, sit on one device and belong to one index).  Every slot owns a
 *             non-blocking stream with two events, a pinned block for the staged inputs and one for the rows, and in HBM the staged
 *             block, the resolve scratch of a resolver of max_queries / max_lexemes, the resolved q_off / term_ids, the rows
 *             (max_queries x max_k x 16 + 4 max_queries bytes), the part lists at the rerank_part in force now and -- with payloads --
 *             max_candidates document indices.  Capacities a batch: max_queries queries, max_lexemes lexemes (or term ids),
 *             max_bytes lexeme bytes, max_candidates candidates over all queries (the cross product counts nq x n_docs), k up to
 *             max_k.  payloads, when not NULL, is a vbm25_documents with payloads of the same documents on the same device: the
 *             reranker sorts (ctid, document) once into a directory of its own and the handle may be freed afterwards; without it
 *             cand_tid is refused.  VBM25_ERR_INVALID, *out == NULL: NULL t or resolver, depth outside 1 .. 16, a zero capacity,
 *             different devices or indexes, a payloads handle without payloads, of another document count or device, an index
 *             without sealed documents (vbm25_evaluate_documents' words).  VBM25_ERR_UNSUPPORTED: max_k over 1024 (the scorer's words).
 *   vbm25_reranker_info     depth, the documents, whether ctids are taken, and `allocations`: every allocation and creation (device,
 *             pinned, stream, event) the handle has made.  It does not move after create: submit and collect allocate, create and
 *             free nothing.  vbm25_reranker_device_bytes: what the handle holds of the device (0 for NULL).
 *   vbm25_reranker_submit_lexemes   vbm25_resolver_submit_lexemes' arrays (its checks and messages), then the candidates: q_cand NULL
 *             for the cross product, or nq + 1 offsets with EITHER cand_doc (vbm25_scorer_topk's indices) OR cand_tid (three uint16_t
 *             a candidate, [bi_hi, bi_lo, ip_posid] as the payloads are).  The ids and the candidates pass the scorer's checks with its
 *             messages.  A ctid no document carries is not eligible and still holds its pos; a ctid of several documents names the
 *             lowest document index.  Everything is validated on the host, copied into the slot's pinned block (the caller's arrays
 *             are free at return), uploaded in one copy and enqueued; the call returns at once.  A batch in which no query has a
 *             candidate enqueues nothing and still takes a slot.  VBM25_ERR_INVALID, nothing enqueued, the ring as it was: NULL
 *             arguments, cand_doc and cand_tid both given, either without q_cand, cand_tid on a reranker without payloads, a full
 *             ring, counts over a capacity (the message names it), k == 0, k > max_k, a batch whose part lists need more scratch
 *             than a slot has because rerank_part was lowered after create.  VBM25_ERR_UNSUPPORTED for 2^31 pairs or more.
 *   vbm25_reranker_submit_ids   the same with the queries as vbm25_scorer_topk's term_ids / q_off (at most max_lexemes ids): no resolve.
 *   vbm25_reranker_collect  waits for the OLDEST batch and copies its nq x k rows and nq counts out, with that batch's nq and k:
 *             vbm25_scorer_topk's contract -- score descending, then pos ascending; n_ranks[q] = min(k, eligible entries of q); the
 *             tail all-zero bytes.  pos is the entry's index within q's own list whatever the list's form, so a caller maps a row
 *             back to its ctid by pos.  VBM25_ERR_INVALID on an empty ring and for NULL arguments (the batch stays in the ring).
 *   vbm25_reranker_in_flight   batches submitted and not collected (0 for NULL).
 *   vbm25_reranker_free     waits for what is in flight, then frees everything.
 * One host thread drives a reranker; two threads take two rerankers, which may share the vbm25_doc_terms and the resolver.  No stream
 * waits for another and no call issues a device-wide synchronisation (create and free allocate and free, as every hipMalloc may). */
typedef struct vbm25_reranker vbm25_reranker;
int vbm25_reranker_create(const vbm25_doc_terms *, const vbm25_resolver *, const vbm25_documents *payloads, uint32_t depth,
                          uint32_t max_queries, uint32_t max_lexemes, uint64_t max_bytes, uint64_t max_candidates, uint32_t max_k,
                          vbm25_reranker **out);
void vbm25_reranker_free(vbm25_reranker *);
uint64_t vbm25_reranker_device_bytes(const vbm25_reranker *);
int vbm25_reranker_info(const vbm25_reranker *, uint32_t *depth, uint32_t *n_docs, uint32_t *has_payloads, uint64_t *allocations);
int vbm25_reranker_submit_lexemes(vbm25_reranker *, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex, uint32_t nq,
                                  const uint64_t *q_cand, const uint32_t *cand_doc, const uint16_t *cand_tid, uint32_t k);
int vbm25_reranker_submit_ids(vbm25_reranker *, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                              const uint32_t *cand_doc, const uint16_t *cand_tid, uint32_t k);
int vbm25_reranker_collect(vbm25_reranker *, vbm25_rank *ranks, uint32_t *n_ranks, uint32_t *nq_out, uint32_t *k_out);
int vbm25_reranker_in_flight(const vbm25_reranker *);

/* The forward index of an index's own documents (csrc/forward.hip): the rerank stack on an index that arrived without its tsvectors --
 * read from pages, built from mappings, produced by a compaction.
 *   vbm25_index_bind       the transpose of the index's postings, made on the index's device from the arrays the index keeps in HBM
 *             (nothing is uploaded): a vbm25_doc_terms of the index's n_docs sealed documents in the index's document order -- per
 *             document the ascending term ids of its postings with their tfs, and the fieldnorm code its postings carry.  It is what
 *             vbm25_documents_bind gives for the documents the index was built from, array for array; a document without a posting
 *             has an empty run and the fieldnorm code 0, and never scores.  vbm25_doc_terms_*, vbm25_evaluate_documents, the scorer
 *             and the reranker take the handle as they take any other; document index d is sealed document d, the one whose ctid is
 *             the index's payload d.  The handle refers to the index, which must outlive it, and is valid for that index only: after
 *             a compaction the caller binds the new index.  The growing segment is not part of it at the bind; vbm25_doc_terms_append*
 *             (below) put its documents behind the sealed ones.  An index of 0 documents binds to
 *             a valid handle of 0 documents.  The result costs 8 bytes a posting and 9 a document; the scratch beyond it is a few
 *             words a document plus a double buffer of the runs longer than 2048 postings, never a sort of all postings.
 *             Synchronous, on a stream of its own, no device-wide synchronisation; the index is only read, so two threads may bind
 *             at once.  VBM25_ERR_INVALID, *out == NULL, nothing enqueued: NULL arguments.  VBM25_ERR_UNSUPPORTED: 2^31 postings or
 *             more in runs longer than 2048.
 *   vbm25_reranker_create_from_index   vbm25_reranker_create on a handle made by vbm25_index_bind, with the ctid directory built from
 *             the index's own payload plane: cand_tid names the rows of the indexed table.  VBM25_ERR_INVALID for a handle that
 *             vbm25_index_bind did not make; every other check and message is vbm25_reranker_create's.  (vbm25_reranker_create
 *             itself takes an index-bound handle as any other; with payloads == NULL it gives a ring without ctids.) */
int vbm25_index_bind(const vbm25_index *, vbm25_doc_terms **out);
int vbm25_reranker_create_from_index(const vbm25_doc_terms *, const vbm25_resolver *, uint32_t depth, uint32_t max_queries,
                                     uint32_t max_lexemes, uint64_t max_bytes, uint64_t max_candidates, uint32_t max_k,
                                     vbm25_reranker **out);

/* The rerank stack on a live table (csrc/live.hip, csrc/reranker.hip): a bound handle grows in place from a delta, and a reranker's ctid
 * directory takes the new rows by a merge on the device.  Neither repeats what was done before.
 *   vbm25_doc_terms_append_documents   the bind of `delta` (cast documents in HBM on the handle's device) written behind the handle's
 *             documents: document i of the delta becomes document n_docs + i.  On a handle from vbm25_index_bind, document
 *             n_sealed + g is then growing document g -- the one a search hit names as doc_id = 0xFFFFFFFF - g -- when the growing
 *             segment is fed the same deltas; the handle stays an index-bound one.  Nothing but the delta's own arrays is read and
 *             nothing is uploaded.  start, term, tf and the fieldnorm codes keep room to spare: a capacity that is outgrown at least
 *             DOUBLES (vbm25_documents_extend's factor), and a growth step copies device to device.
 *             Payloads: a delta's payloads are kept in a tail array of the handle that covers the appended documents only (the
 *             index's plane, or the vbm25_documents given to vbm25_reranker_create, serves the documents the handle was bound with).
 *             An index-bound handle refuses a delta without payloads; on any other handle the first append decides whether the
 *             appended documents carry payloads, and later deltas must agree (vbm25_documents_extend's rule).
 *             The call is synchronous.  Every check and every allocation comes first; then it waits for the DEVICE, and only then
 *             writes -- so a reranker batch or a scorer call enqueued before the append ends on the old arrays, and a call made
 *             after it takes the new documents as document indices (cand_doc, the cross product) with no further call.  A refused
 *             or failed append leaves the handle byte for byte as it was.  The caller does not append while another thread is inside
 *             a call on the same handle (a scorer's, a reranker's, a download): the handle holds no lock.
 *             VBM25_ERR_INVALID, nothing changed: NULL arguments, a delta that belongs to a caster slot which is in flight again
 *             (submitted since the delta's collect and not yet collected: its arrays are being rewritten -- this is all that is
 *             detected: once that batch is collected the same pointer is the new batch's documents, a valid delta, so a collected
 *             handle is appended before the submit that takes its slot again), a delta, a handle and a resolver on different devices, a resolver of another index than the handle's, the
 *             payload rules above.  VBM25_ERR_UNSUPPORTED: 2^32 - 1 documents or more (a document index is 32 bits and 0xFFFFFFFF
 *             names no document), or known elements that could reach 2^32 (a run's bounds are read as 32 bits).  A delta of 0
 *             documents that passes the checks returns VBM25_OK and changes nothing.
 *   vbm25_doc_terms_append   the same from a host CSR in the form vbm25_device_growing_append takes (what vbm25_growing_from_pages
 *             hands back for the rows that were unsealed when the process came up): keys, tfs, fieldnorm codes and payloads are staged
 *             to the device once, then the step above.  payload == NULL: a delta without payloads.  The CSR is validated as an upload's:
 *             keys that do not ascend strictly and a start that is not monotone are VBM25_ERR_INVALID, naming the document.  A
 *             document whose `deleted` flag is set is appended with an empty run (its fieldnorm code and payload as given), so the
 *             numbering stays the growing segment's.
 *   vbm25_doc_terms_base_docs   the documents the handle was bound with (0 for NULL): on an index-bound handle the sealed ones.
 *             vbm25_doc_terms_info, _download and _device_bytes report the grown handle (the bytes with the room to spare).
 *   vbm25_reranker_sync     brings the ctid directory up to the handle's n_docs.  On slot 0's stream: the payloads of the documents the
 *             directory lacks become (ctid, document) pairs in ctid order, equal ctids by ascending document -- a delta of up to
 *             live_sort_max rows (vbm25_tuning_set, 0 .. 4096, default 4096) sorted by one workgroup in LDS, a larger one by the radix
 *             sort create uses; old and new entries go to their ranks in the merged order in spare arrays (the new documents'
 *             indices exceed the old ones', so a ctid of several documents still names the lowest); the evenly spaced directory is
 *             sampled again, its stride may change.  The call then waits for every slot of the reranker and swaps the spare arrays
 *             in: a batch submitted before the sync resolves its ctids against the old directory whenever it is collected, one
 *             submitted after it against the new one.  The sorted arrays and the delta's scratch keep room to spare that at least
 *             doubles when outgrown: a sync that fits allocates nothing, `allocations` moves only in a sync that grows, submit and
 *             collect still allocate nothing.  max_candidates is unchanged: a cross product that outgrows it is refused at submit.
 *             VBM25_ERR_INVALID, the directory unchanged: NULL, a reranker without payloads, appended documents without payloads.
 *             Nothing new: VBM25_OK.  vbm25_reranker_info's n_docs stays the handle's count;
 *             vbm25_reranker_directory_docs is the count the directory covers (0 for NULL).
 *             vbm25_reranker_create and _create_from_index on a handle that has grown build the directory over everything at once
 *             -- the base payloads, then the handle's tail -- and compare `payloads` with vbm25_doc_terms_base_docs. */
int vbm25_doc_terms_append_documents(vbm25_doc_terms *, const vbm25_documents *delta, const vbm25_resolver *);
int vbm25_doc_terms_append(vbm25_doc_terms *, const vbm25_growing_desc *delta, const vbm25_resolver *);
uint32_t vbm25_doc_terms_base_docs(const vbm25_doc_terms *);
int vbm25_reranker_sync(vbm25_reranker *);
uint32_t vbm25_reranker_directory_docs(const vbm25_reranker *);

/* Deletes on a bound handle (csrc/live.hip): the rows a DELETE or a bulkdelete killed leave the rerank, as they leave the search
 * (vbm25_device_growing_delete_tids, vbm25_filter_set_tids, vbm25_device_vacuum_bulkdelete).  The handle gets a deletion bitmap: one
 * bit a document, packed as the filters and the deletion words are -- uint64_t words, document d at bit d & 63 of word d >> 6, set =
 * dead.  The bitmap is allocated by the first delete that names a document and never before: a handle nobody deleted from holds
 * none, reports the vbm25_doc_terms_device_bytes it always did, and runs every kernel as before.  Bits at and beyond n_docs are zero.
 *   vbm25_doc_terms_delete   `docs`: n document indices of the handle (on an index-bound handle sealed document d is index d, growing
 *             document g is vbm25_doc_terms_base_docs + g).  Repeats and documents already dead are allowed; *n_new (may be NULL) is
 *             the number of documents that were live before the call and are dead after it.  The indices are uploaded once; one
 *             lane handles one index with an atomicOr on its word, and the new bits are counted from the word the atomic returns, so
 *             a repeat within one call counts once.  VBM25_ERR_INVALID, checked on the host before anything is enqueued: NULL
 *             arguments, an index at or beyond n_docs (the message names the entry).
 *   vbm25_doc_terms_delete_tids   every document whose ctid is in the set dies.  The ctids of documents 0 .. base_docs are the index's
 *             doc_payload plane on an index-bound handle (`payloads` must be NULL), else those of `payloads` -- the handle
 *             vbm25_reranker_create takes, under its checks: with payloads, base_docs documents, on the handle's device; a
 *             documents-bound handle with base_docs > 0 needs it.  The ctids of the appended documents are the handle's tail; a
 *             handle whose appended documents carry no payloads is refused, as is a set on another device.  One kernel: wave w
 *             answers word w of the bitmap, each lane reading its document's ctid from the base plane or the tail (the split falls
 *             inside a word whenever base_docs % 64 != 0), the set's directory in LDS, one ballot a word; lane 0 ORs the word in
 *             and counts the new bits.  Grid-stride under the tid_grid cap.  Documents that share a ctid die together.
 *   Both deletes keep the append's contract.  They are synchronous.  Every check and every allocation comes first; then the call
 *             waits for the DEVICE, and only then writes -- so a scorer call or a reranker batch enqueued before the delete ends on
 *             the old bits, and one made after it sees the new bits with no further call.  A refused or failed delete leaves the
 *             words and the count as they were.  A delete of nothing (n == 0, an empty set, a set that matches nothing on a handle
 *             without a bitmap) returns VBM25_OK and leaves the handle without a bitmap.  The caller does not delete while another
 *             thread is inside a call on the handle.  There is no undelete, and ctids of the set that match no document are not
 *             counted.
 *   vbm25_doc_terms_dead_docs   the dead documents now (0 for NULL).
 *   vbm25_doc_terms_read_dead   ceil(n_docs / 64) words to the host, all zero on a handle without a bitmap.
 *   What a dead document changes: in vbm25_scorer_topk and in a reranker batch -- cand_doc lists, the cross product and ctid lists
 *             alike -- a candidate whose document is dead is not eligible, exactly as an entry that names no document is not: its
 *             pos still counts and it takes no rank, n_ranks[q] = min(k, the live eligible entries of q).  A ctid of several
 *             documents resolves to the lowest LIVE one (the lookup walks forward over the ctid's entries, which lie by ascending
 *             document), or to none when all are dead: once a reused ctid's new row is appended and synced, the ctid names that
 *             row.  Reranker `allocations` never moves on a delete.
 *   What it does not change: vbm25_evaluate_documents, vbm25_scorer_evaluate and vbm25_doc_terms_download -- `<&>` is a function of
 *             the pair -- and vbm25_reranker_sync, vbm25_reranker_create*: the ctid directory keeps the dead documents' entries
 *             (nothing compacts them out) until the VACUUM drops the handle.  vbm25_doc_terms_append still gives a document flagged
 *             `deleted` an empty run and leaves it live; a caller that restarts from a growing CSR calls vbm25_doc_terms_delete on
 *             those documents afterwards.  An append carries the bitmap along: its capacity follows the fieldnorm array's, the old
 *             words are copied, the appended documents are live, a refused append leaves it untouched. */
int vbm25_doc_terms_delete(vbm25_doc_terms *, const uint32_t *docs, uint64_t n, uint32_t *n_new);
int vbm25_doc_terms_delete_tids(vbm25_doc_terms *, const vbm25_tid_set *, const vbm25_documents *payloads, uint32_t *n_new);
uint32_t vbm25_doc_terms_dead_docs(const vbm25_doc_terms *);
int vbm25_doc_terms_read_dead(const vbm25_doc_terms *, uint64_t *words);

#ifdef __cplusplus
}
#endif
#endif
