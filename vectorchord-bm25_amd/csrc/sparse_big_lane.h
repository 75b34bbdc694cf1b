// sparse_big_lane.h -- the per-lane functions of scan_sparse_big_kernel (sparse queries at 256 < k <= 1024: the rank-addressed window
// scan, scan_sparse_big.h).  __host__ __device__, and plain C++ as well: the kernel's tile plan, its chunk loads and its slot addresses
// are these, and tests/native/fuzz_sparse_big.cpp compiles the same text with g++ under AddressSanitizer and carries tiles out with
// them as the workgroup does, against a std::map accumulation.
//
//   run          the postings of one term inside one 2^16-document window: a contiguous, ascending run of 16-bit ids in post_id16,
//                [win_off[w], win_off[w + 1]) in the term's own posting numbers.  A SLICE [a, b) is the part of a run inside a tile.
//   tile         one window, or a power-of-two aligned part of one, clipped to the item's documents (tile_end).  A tile FITS
//                (tile_fits) when its slices hold at most CAP postings in at most THREADS chunks; otherwise its width halves (halve).
//                Width 1 always fits: one document, at most MAX_T postings in MAX_T chunks.
//   chunk        CHUNK = 8 consecutive postings of one term at a multiple of 8: one 16-byte load from post_id16 and one from post_tfn.
//                A slice [a, b) takes chunks_of(a, b) of them, the alignment waste at both ends included; the tile's chunks are
//                numbered term after term (cb: the exclusive prefix of the terms' chunk counts, cb[m] = all of them), thread c owns
//                chunk c: chunk_term, chunk_start, and chunk_mask says which of its 8 postings lie inside the slice.
//   slot         a document's accumulator is addressed by its RANK among the tile's documents: the bits set below its own in the
//                window's bitmap = the exclusive prefix of the popcounts of the words before + the bits below in its word (slot_of).
//   run_lower_bound   the first posting of a run at or above a 16-bit id: where a tile that is not a whole window cuts a run
#ifndef VBM25_SPARSE_BIG_LANE_H
#define VBM25_SPARSE_BIG_LANE_H

#include "dense_list_lane.h"

namespace vbm25 {
namespace sbig {

constexpr uint32_t CAP = 4096;                      // postings (and so documents, accumulators) of a tile
constexpr uint32_t CHUNK = 8;                       // postings a thread owns
constexpr uint32_t THREADS = dlist::WAVES * 64u;    // 512: chunks of a tile
constexpr uint32_t MAX_T = 16;                      // indexed terms of a query
constexpr uint32_t WIN = 65536;                     // documents of a window
constexpr uint32_t BM_WORDS = WIN / 32u;            // words of the window's bitmap
constexpr uint32_t ROUND = 2u * THREADS;            // slots of one sweep round: at most that many appends between two cuts
static_assert(THREADS * CHUNK == CAP, "a full tile is one chunk a thread");
static_assert(ROUND <= dlist::CAP - dlist::MAX_K, "a round's appends fit behind the k entries a cut leaves");
static_assert(BM_WORDS == 4u * THREADS, "the rank phase: four bitmap words a thread");

RRK_HD uint32_t chunk_floor(uint32_t p) { return p & ~(CHUNK - 1u); }
RRK_HD uint32_t chunks_of(uint32_t a, uint32_t b) { return b > a ? (chunk_floor(b - 1u) - chunk_floor(a)) / CHUNK + 1u : 0u; }

RRK_HD bool tile_fits(uint32_t postings, uint32_t chunks) { return postings <= CAP && chunks <= THREADS; }
RRK_HD uint32_t halve(uint32_t width) { return width > 1u ? width >> 1 : 1u; }
RRK_HD uint32_t widen(uint32_t width) { return width < WIN ? width << 1 : WIN; }
// the end of the tile that starts at document cur: the end of the aligned block of `width` documents (a power of two <= WIN) that
// holds cur, or the end of the part [.., part_hi) of the window that belongs to the item, whichever comes first
RRK_HD uint32_t tile_end(uint32_t cur, uint32_t width, uint32_t part_hi) {
    const uint64_t e = (uint64_t(cur) | uint64_t(width - 1u)) + 1ull;
    return e < part_hi ? uint32_t(e) : part_hi;
}
// the part of window w that belongs to an item whose documents end at hi
RRK_HD uint32_t part_end(uint32_t w, uint32_t hi) {
    const uint64_t e = (uint64_t(w) + 1ull) << 16;
    return e < hi ? uint32_t(e) : hi;
}
// a tile [cur, end) that is its whole window (the last window ends with the corpus): the slices are the runs, nothing is searched
RRK_HD bool whole_window(uint32_t cur, uint32_t end, uint32_t n_docs) { return (cur & (WIN - 1u)) == 0u && ((end & (WIN - 1u)) == 0u || end == n_docs); }

// id_at(i): the 16-bit id of the term's posting i.  The first posting of [a, b) whose id is >= x (b: none)
template <class IdAt>
RRK_HD uint32_t run_lower_bound(IdAt id_at, uint32_t a, uint32_t b, uint32_t x) {
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (uint32_t(id_at(mid)) < x) a = mid + 1u;
        else b = mid;
    }
    return a;
}

// chunk c of the tile (c < cb[m]) belongs to the term t with cb[t] <= c < cb[t + 1]
RRK_HD uint32_t chunk_term(const uint32_t *cb, uint32_t m, uint32_t c) {
    uint32_t t = 0;
    while (t + 1u < m && cb[t + 1u] <= c) ++t;
    return t;
}
// its first posting (a multiple of CHUNK), a the start of the term's slice and cb_t the term's first chunk
RRK_HD uint32_t chunk_start(uint32_t a, uint32_t cb_t, uint32_t c) { return chunk_floor(a) + CHUNK * (c - cb_t); }
// bit e: posting start + e lies inside the slice [a, b) (head and tail of a slice: the alignment waste masked out)
RRK_HD uint32_t chunk_mask(uint32_t start, uint32_t a, uint32_t b) {
    const uint32_t lo = a > start ? a - start : 0u;
    const uint32_t hi = b > start ? (b - start < CHUNK ? b - start : CHUNK) : 0u;
    return lo < hi ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}
// posting e of a chunk from its four id words / its four tf-fieldnorm words (device_types.h: post_id16, post_tfn)
RRK_HD uint32_t chunk_id(const uint32_t *idw, uint32_t e) { return (idw[e >> 1] >> (16u * (e & 1u))) & 0xffffu; }
RRK_HD uint32_t chunk_tf(const uint32_t *tfw, uint32_t e) { return (tfw[e >> 1] >> (8u * (e & 1u))) & 0xffu; }
RRK_HD uint32_t chunk_fn(const uint32_t *tfw, uint32_t e) { return (tfw[e >> 1] >> (16u + 8u * (e & 1u))) & 0xffu; }

RRK_HD uint32_t popc(uint32_t v) { return uint32_t(__builtin_popcount(v)); }
// the accumulator slot of the document that owns bit `bit` of a bitmap word: `prefix` = the bits set in all words before
RRK_HD uint32_t slot_of(uint32_t prefix, uint32_t word, uint32_t bit) { return prefix + popc(word & ((1u << bit) - 1u)); }

}  // namespace sbig
}  // namespace vbm25

#endif
