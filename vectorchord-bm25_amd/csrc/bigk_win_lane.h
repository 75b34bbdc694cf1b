// bigk_win_lane.h -- the per-lane functions of bigk_scan_win_kernel (bigk.hip: the candidate scan of sparse queries at k > 1024, fed
// from the window planes).  __host__ __device__, and plain C++ as well: tests/native/fuzz_bigk_win.cpp compiles the same text with g++
// under AddressSanitizer and carries tiles out with them as the workgroup does, against a std::map accumulation and a straightforward
// field extraction.  Runs, slices, chunks and slots are sparse_big_lane.h's (sbig::); what is new here:
//
//   tile         FAST PATH: up to MAX_G consecutive whole 2^16-document windows [w, w + g).  A term's postings of consecutive windows
//                are contiguous in posting order, so its slice of the tile is the single run [win_off[w], win_off[w + g]): chunk
//                numbering and the two 16-byte loads a thread are those of a one-window tile.  fit_windows: the longest g whose slices
//                fit (sbig::tile_fits).  SLOW PATH (one window does not fit): a power-of-two aligned part of that window, as in
//                scan_sparse_big_kernel.
//   tile id      a document's place in the tile: window inside the tile << 16 | its 16-bit id (tile_id): its bit in the tile's bitmap
//                of MAX_G x 2^16 bits, and what the sweep adds to the tile's first document.  posting_window: the window of posting p
//                of a term inside the tile = how many of the g - 1 inner win_off entries are <= p (empty windows counted through).
//   wide tf      a zero word in post_tfn: one posting of the pair has a term frequency wider than a byte (wide_pair).  Its exact value
//                is one field of the reference's block (compression.rs:65-136): tf_fields finds the term-frequency payload behind the
//                document ids, field_at extracts field i, bit-packed (crates/simd/src/bitpacking.rs:58-98: four interleaved LSB-first
//                streams) or byte-packed.  The formats are decode.h's bp_field / byte_field; this reads one field, not a block.
#ifndef VBM25_BIGK_WIN_LANE_H
#define VBM25_BIGK_WIN_LANE_H

#include "sparse_big_lane.h"

#ifndef VBM25_BIGK_WIN_G
#define VBM25_BIGK_WIN_G 2
#endif

namespace vbm25 {
namespace bwin {

constexpr uint32_t MAX_G = VBM25_BIGK_WIN_G;                    // whole windows of a tile at most
static_assert(MAX_G == 1u || MAX_G == 2u || MAX_G == 4u, "the tile spans 1, 2 or 4 windows");
constexpr uint32_t BM_WORDS = MAX_G * sbig::BM_WORDS;           // words of the tile's bitmap
constexpr uint32_t RANK_WORDS = BM_WORDS / sbig::THREADS;       // consecutive bitmap words a thread counts: 4 MAX_G
constexpr uint32_t INNER = 3;                                   // inner window bounds kept per term (MAX_G - 1 of them used)

// the whole windows a fast tile may span: the tuning value, the compile-time maximum and what the item has left (>= 1)
RRK_HD uint32_t tile_windows(uint32_t wanted, uint32_t left) {
    uint32_t g = wanted < MAX_G ? wanted : MAX_G;
    if (g > left) g = left;
    return g ? g : 1u;
}

// The longest run of whole windows that fits, tried from g down.  totals(n, posts, chunks): postings and chunks of all terms' slices
// over the first n windows (in the kernel: two wave scans).  Returns 0 when one window does not fit: the slow path.
template <class Totals>
RRK_HD uint32_t fit_windows(Totals totals, uint32_t g) {
    for (; g; --g) {
        uint32_t posts = 0, chunks = 0;
        totals(g, posts, chunks);
        if (sbig::tile_fits(posts, chunks)) break;
    }
    return g;
}

// the window, inside a tile of g whole windows, of posting p of a term: inner[i] = the term's win_off entry of window i + 1 of the tile
RRK_HD uint32_t posting_window(uint32_t p, const uint32_t *inner, uint32_t g) {
    uint32_t w = 0;
    for (uint32_t i = 0; i < INNER; ++i) w += i + 1u < g && p >= inner[i] ? 1u : 0u;  // (inner holds INNER entries; a fixed trip count)
    return w;
}
RRK_HD uint32_t tile_id(uint32_t win, uint32_t id16) { return win << 16 | id16; }

// posting e of a chunk lies in a pair with a term frequency wider than a byte: its tf and fieldnorm bytes are not in the word
RRK_HD bool wide_pair(const uint32_t *tfw, uint32_t e) { return tfw[e >> 1] == 0u; }

// bytes of a block payload of n fields.  meta: bit 7 = byte packed, low bits = width (bits, or bytes)
RRK_HD uint32_t payload_bytes(uint32_t meta, uint32_t n) { return (meta >> 7) ? (meta & 127u) * n : 16u * (meta & 127u); }
// the term-frequency payload of a block body: behind the document ids, at the next multiple of 8
RRK_HD const uint8_t *tf_fields(const uint8_t *body, uint32_t meta_doc, uint32_t n) { return body + ((payload_bytes(meta_doc, n) + 7u) & ~7u); }
// field i of a payload (no delta).  Bit-packed payloads are read as 32-bit words: p is 4-byte aligned (block bodies lie at multiples of 8)
RRK_HD uint32_t field_at(const uint8_t *p, uint32_t meta, uint32_t i) {
    const uint32_t width = meta & 127u;
    if (meta >> 7) {
        uint32_t v = 0;
        for (uint32_t j = 0; j < width && j < 4u; ++j) v |= uint32_t(p[i * width + j]) << (8u * j);
        return v;
    }
    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(p);
    if (width == 0u) return 0u;
    if (width >= 32u) return w32[i];
    const uint32_t l = i & 3u, bit = (i >> 2) * width, w = bit >> 5, sh = bit & 31u;
    const uint64_t lo = w32[4u * w + l];
    const uint64_t hi = sh + width > 32u ? w32[4u * (w + 1u) + l] : 0u;
    return uint32_t((hi << 32 | lo) >> sh) & ((1u << width) - 1u);
}

}  // namespace bwin
}  // namespace vbm25

#endif
