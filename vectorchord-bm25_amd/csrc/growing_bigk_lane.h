// growing_bigk_lane.h -- the per-entry functions of the growing segment's k > 1024 route (growing_bigk.h).  __host__ __device__, and
// plain C++ as well: the kernels and the host's cut are loops over these, and tests/native/fuzz_growing_bigk.cpp compiles the same
// text with g++ under AddressSanitizer and holds it against std::merge and a brute-force chunking.
//
//   the two lists   a query's sealed records S (ns of them, best first, a record `stride` doubles apart with its score first) and its
//                growing survivors: ng entries (key = the bits of the f64 score, g) in tiles of bgk::TILE, each tile sorted best
//                first -- key descending, g ascending (bigk_lane.h's order).  A growing entry goes before a sealed one only with a
//                HIGHER score: that is vbm25_merge_hits, and grow_rank_merge of growing.h.
//   growing_rank / growing_pos   a survivor's rank among the survivors is its index in its tile plus bgk::count_beating over the
//                query's other tiles; its record's position adds the sealed records that score at least as high
//   sealed_pos   a sealed record's position: its index plus the survivors that score strictly higher, one bisection a tile
//   query_cap    a query's candidate capacity: no more than its terms' growing postings, no more than the growing documents
//   chunk_end    the host's chunk cut: queries in order while their segments fit the candidate scratch and their survivors the rows
//   items_per_query / item_tiles   the scan's work items: runs of tiles per query, about `target` items a launch, computed from the
//                workgroup's number (no item list)
#ifndef VBM25_GROWING_BIGK_LANE_H
#define VBM25_GROWING_BIGK_LANE_H

#include <cstddef>
#include <cstdint>

#include "bigk_lane.h"

namespace vbm25 {
namespace gbk {

constexpr uint32_t TERM_PASS = 256;     // entries of the scan's LDS term table: a query of more terms refills it in passes
constexpr uint32_t ITEM_TARGET = 2048;  // work items a launch of the scan aims at: a few per CU

BGK_HD double key_score(uint64_t key) {
    double s;
    __builtin_memcpy(&s, &key, 8);
    return s;
}

// sealed records that score at least s
BGK_HD uint32_t sealed_at_least(const double *S, uint32_t stride, uint32_t ns, double s) {
    uint32_t lo = 0, hi = ns;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (S[size_t(mid) * stride] >= s) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// entries of a tile sorted best first that score strictly higher than s
BGK_HD uint32_t tile_above(const uint64_t *keys, uint32_t n, double s) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key_score(keys[mid]) > s) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// survivor i of ng (tiles of bgk::TILE from keys / docs): its rank among the survivors
BGK_HD uint32_t growing_rank(const uint64_t *keys, const uint32_t *docs, uint32_t ng, uint32_t i) {
    const uint32_t mine = i / bgk::TILE, n_tiles = (ng + bgk::TILE - 1u) / bgk::TILE;
    uint32_t rank = i % bgk::TILE;
    for (uint32_t u = 0; u < n_tiles; ++u) {
        const uint32_t n = ng - u * bgk::TILE < bgk::TILE ? ng - u * bgk::TILE : bgk::TILE;
        if (u != mine) rank += bgk::count_beating(keys + size_t(u) * bgk::TILE, docs + size_t(u) * bgk::TILE, n, keys[i], docs[i]);
    }
    return rank;
}

// ... and its record's position in the merged list
BGK_HD uint32_t growing_pos(const uint64_t *keys, const uint32_t *docs, uint32_t ng, uint32_t i, const double *S, uint32_t stride,
                            uint32_t ns) {
    return growing_rank(keys, docs, ng, i) + sealed_at_least(S, stride, ns, key_score(keys[i]));
}

// sealed record i: its position in the merged list
BGK_HD uint32_t sealed_pos(const uint64_t *keys, uint32_t ng, const double *S, uint32_t stride, uint32_t i) {
    const double s = S[size_t(i) * stride];
    const uint32_t n_tiles = (ng + bgk::TILE - 1u) / bgk::TILE;
    uint32_t pos = i;
    for (uint32_t u = 0; u < n_tiles; ++u) {
        const uint32_t n = ng - u * bgk::TILE < bgk::TILE ? ng - u * bgk::TILE : bgk::TILE;
        pos += tile_above(keys + size_t(u) * bgk::TILE, n, s);
    }
    return pos;
}

BGK_HD uint32_t query_cap(uint32_t n_grow, uint64_t postings) { return postings < n_grow ? uint32_t(postings) : n_grow; }

// The chunk that starts at query q0: the first query behind it.  Queries join in order while the chunk holds fewer than chunk_q of
// them and their capacities fit chunk_cand; base[q] is where query q's segment starts in the scratch.  A capacity above chunk_cand
// does not fit any chunk: q0 is returned (the scratch is sized so that none is -- the caller reports it).
BGK_HD uint32_t chunk_end(const uint32_t *cap, uint32_t nq, uint32_t q0, uint32_t chunk_q, uint64_t chunk_cand, uint32_t *base) {
    uint64_t used = 0;
    uint32_t q = q0;
    while (q < nq && q - q0 < chunk_q && used + cap[q] <= chunk_cand) {
        base[q] = uint32_t(used);
        used += cap[q];
        ++q;
    }
    return q;
}

// work items per query of a chunk of cq queries over n_tiles tiles: at least one, at most one per tile
BGK_HD uint32_t items_per_query(uint32_t n_tiles, uint32_t cq, uint32_t target) {
    const uint32_t share = target / (cq ? cq : 1u), most = n_tiles ? n_tiles : 1u;
    return share < 1u ? 1u : share > most ? most : share;
}

// item w of ipq: its tiles [j0, j1) -- the items of a query cover [0, n_tiles) exactly once
BGK_HD void item_tiles(uint32_t w, uint32_t ipq, uint32_t n_tiles, uint32_t &j0, uint32_t &j1) {
    j0 = uint32_t(uint64_t(w) * n_tiles / ipq);
    j1 = uint32_t(uint64_t(w + 1u) * n_tiles / ipq);
}

}  // namespace gbk
}  // namespace vbm25

#endif
