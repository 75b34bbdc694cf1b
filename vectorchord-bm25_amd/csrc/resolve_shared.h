// resolve_shared.h -- what resolve.hip (the resolver ring) and reranker.hip (the reranker ring) have in common: the validation of a
// lexeme batch, the sizes of the resolve scratch, and the enqueue of intern -> lookup -> pack with the output pointers as
// parameters.  Both rings resolve through the same kernels, which live in resolve.hip; neither copies the other's text.
// HIP-only, not part of the ABI.
#ifndef VBM25_RESOLVE_SHARED_H
#define VBM25_RESOLVE_SHARED_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "vbm25_internal.h"
#include "hip_host.h"
#include "resolve_lane.h"
#include "lexeme_input.h"

namespace vbm25 {
namespace rsv {

constexpr uint32_t WAVE_QUERY = 64;  // the wave path's longest query

// what a lexeme batch is, checked before anything is allocated or enqueued
struct LexShape {
    uint32_t n_lex = 0, longest_query = 0;
    uint64_t n_bytes = 0, longest_lexeme = 0;
};
int check_offsets32(const uint32_t *q, uint32_t nq, const char *what, LexShape *s);
// vbm25_resolver_submit_lexemes' checks of the arrays, in its order and with its messages
int check_lexemes(bool has_seed, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex, uint32_t nq, LexShape *s);

// The scratch of one resolve in flight, for batches of up to max_queries queries and max_lexemes lexemes.  Bytes:
//   ids, tmp   4 (max_lexemes + 1)          counts, q_off   4 (max_queries + 1)
//   sort_a     8 max_lexemes                sort_b          8 max_lexemes + 4 (max_lexemes + 1)     cub   pack_cub_bytes
struct PackScratch {
    uint32_t *ids, *tmp, *counts, *q_off;
    unsigned long long *sort_a, *sort_b;
    void *cub;
    size_t cub_bytes;
    uint32_t max_lexemes;
};
// hipcub's temporary storage for the scans and the sort of a pack at these capacities
int pack_cub_bytes(uint32_t max_queries, uint32_t max_lexemes, hipStream_t st, size_t *bytes);

// intern_kernel on `st`; keys_out and ids may each be NULL.  The pool is 4-byte aligned and ends on a multiple of 4.
int launch_intern(hipStream_t st, const lexin::Seed &seed, const uint32_t *pool, const uint64_t *lex_off, uint32_t n_lex, uint64_t longest,
                  const Key *vocab, uint32_t n_terms, Key *keys_out, uint32_t *ids);
// Step (c) after the ids are in s.ids: the wave path when longest_query <= WAVE_QUERY, the radix path otherwise.  The last kernel
// writes out_q_off (nq + 1) and out_ids, in pinned host memory or in HBM.
int enqueue_pack(hipStream_t st, const PackScratch &s, const uint32_t *q_lex_dev, uint32_t nq, uint32_t n_lex, uint32_t longest_query,
                 uint32_t *out_ids, uint32_t *out_q_off);

// what a ring that resolves for itself reads of a resolver: the vocabulary in HBM (ResolverVocabulary) and the seed
struct ResolverSeed {
    bool has_seed;
    lexin::Seed seed;
};
int resolver_seed(const vbm25_resolver *r, ResolverSeed *out);

}  // namespace rsv
}  // namespace vbm25

#endif
