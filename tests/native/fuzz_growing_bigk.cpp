// fuzz_growing_bigk.cpp -- csrc/growing_bigk_lane.h on the CPU under AddressSanitizer + UBSan: the two position formulas of
// growing_bigk_merge_kernel against std::merge (sealed first on equal scores) over random sorted lists with ties, and the capacity,
// chunk and item cuts of growing_bigk_run against brute force.  Buffers are allocated exactly.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/growing_bigk_lane.h"

using namespace vbm25;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Rec { double score; bool sealed; uint32_t id; };  // a merged entry: its score, and where it came from

static uint64_t bits_of(double s) { uint64_t b; std::memcpy(&b, &s, 8); return b; }

// ns sealed records (three doubles apart) and ng growing survivors in tiles sorted best first, scores from `levels` values (ties)
static void merge_case(std::mt19937_64 &rng, uint32_t ns, uint32_t ng, uint32_t levels) {
    auto score = [&] { return 0.25 * double(1 + rng() % levels); };
    std::vector<double> S(3 * size_t(ns)), ss(ns);
    for (double &s : ss) s = score();
    std::sort(ss.begin(), ss.end(), std::greater<double>());
    for (uint32_t i = 0; i < ns; ++i) S[3 * size_t(i)] = ss[i];
    std::vector<Rec> grow(ng);
    for (uint32_t j = 0; j < ng; ++j) grow[j] = Rec{score(), false, j};  // (distinct g)
    std::shuffle(grow.begin(), grow.end(), rng);
    std::vector<uint64_t> keys(ng);
    std::vector<uint32_t> docs(ng);
    for (uint32_t t = 0; t < ng; t += bgk::TILE) {  // the tile sort: arrival order cut in tiles, each best first
        const uint32_t e = std::min(ng, t + bgk::TILE);
        std::sort(grow.begin() + t, grow.begin() + e, [](const Rec &a, const Rec &b) { return bgk::beats(bits_of(a.score), a.id, bits_of(b.score), b.id); });
        for (uint32_t j = t; j < e; ++j) keys[j] = bits_of(grow[j].score), docs[j] = grow[j].id;
    }
    // the reference: the growing list in its order, merged behind the sealed one on equal scores
    std::vector<Rec> gl = grow, sl(ns), want(size_t(ns) + ng);
    std::sort(gl.begin(), gl.end(), [](const Rec &a, const Rec &b) { return a.score > b.score || (a.score == b.score && a.id < b.id); });
    for (uint32_t i = 0; i < ns; ++i) sl[i] = Rec{ss[i], true, i};
    std::merge(sl.begin(), sl.end(), gl.begin(), gl.end(), want.begin(), [](const Rec &a, const Rec &b) { return a.score > b.score; });
    std::vector<int> seen(want.size(), 0);
    for (uint32_t i = 0; i < ns; ++i) {
        const uint32_t pos = gbk::sealed_pos(keys.data(), ng, S.data(), 3, i);
        CHECK(pos < want.size() && want[pos].sealed && want[pos].id == i, "sealed %u of %u at %u (ng %u)", i, ns, pos, ng);
        if (pos < seen.size()) ++seen[pos];
    }
    for (uint32_t j = 0; j < ng; ++j) {
        const uint32_t pos = gbk::growing_pos(keys.data(), docs.data(), ng, j, S.data(), 3, ns);
        CHECK(pos < want.size() && !want[pos].sealed && want[pos].id == docs[j], "growing %u of %u at %u (ns %u)", j, ng, pos, ns);
        if (pos < seen.size()) ++seen[pos];
    }
    for (size_t p = 0; p < seen.size(); ++p) CHECK(seen[p] == 1, "position %zu written %d times", p, seen[p]);
}

static void cut_case(std::mt19937_64 &rng, uint32_t nq, uint32_t n_grow, uint32_t chunk_q, uint64_t chunk_cand) {
    std::vector<uint32_t> cap(nq), base(nq, 0xdeadbeefu);
    for (uint32_t &c : cap) {
        const uint64_t postings = rng() % 3 ? rng() % (2ull * n_grow + 1) : 0;
        c = gbk::query_cap(n_grow, postings);
        CHECK(c <= n_grow && c <= postings && (c == n_grow || c == postings), "cap %u of %llu postings, %u documents", c, (unsigned long long)postings, n_grow);
    }
    uint32_t q = 0;
    while (q < nq) {
        const uint32_t q1 = gbk::chunk_end(cap.data(), nq, q, chunk_q, chunk_cand, base.data());
        CHECK(q1 > q && q1 <= nq && q1 - q <= chunk_q, "chunk [%u, %u) of %u", q, q1, nq);
        if (q1 <= q) return;
        uint64_t used = 0;  // brute force: the segments lie back to back inside the scratch, and the next query would not have fit
        for (uint32_t i = q; i < q1; ++i) {
            CHECK(base[i] == used, "query %u starts at %u, want %llu", i, base[i], (unsigned long long)used);
            used += cap[i];
        }
        CHECK(used <= chunk_cand, "chunk [%u, %u) holds %llu > %llu", q, q1, (unsigned long long)used, (unsigned long long)chunk_cand);
        CHECK(q1 == nq || q1 - q == chunk_q || used + cap[q1] > chunk_cand, "chunk [%u, %u) ends early", q, q1);
        q = q1;
    }
    // the items of a query cover its tiles exactly once, whatever the cut
    const uint32_t n_tiles = uint32_t(rng() % 40), cq = 1 + uint32_t(rng() % 3000);
    const uint32_t ipq = gbk::items_per_query(n_tiles, cq, gbk::ITEM_TARGET);
    CHECK(ipq >= 1 && ipq <= std::max(n_tiles, 1u) && (ipq == 1 || uint64_t(ipq) * cq <= gbk::ITEM_TARGET), "ipq %u for %u tiles, %u queries", ipq, n_tiles, cq);
    uint32_t next = 0;
    for (uint32_t w = 0; w < ipq; ++w) {
        uint32_t j0, j1;
        gbk::item_tiles(w, ipq, n_tiles, j0, j1);
        CHECK(j0 == next && j1 >= j0 && j1 <= n_tiles, "item %u of %u: [%u, %u) behind %u", w, ipq, j0, j1, next);
        next = j1;
    }
    CHECK(next == n_tiles, "the items end at %u of %u tiles", next, n_tiles);
}

int main() {
    std::mt19937_64 rng(20261126);
    uint32_t cases = 0;
    for (uint32_t ns : {0u, 1u, 7u, 1025u, 5000u})
        for (uint32_t ng : {0u, 1u, 2u, 100u, bgk::TILE - 1, bgk::TILE, bgk::TILE + 1, 2 * bgk::TILE + 77})
            for (uint32_t levels : {1u, 3u, 1000u}) merge_case(rng, ns, ng, levels), ++cases;
    for (uint32_t i = 0; i < 300; ++i) {
        const uint32_t n_grow = uint32_t(rng() % 5000);
        cut_case(rng, 1 + uint32_t(rng() % 200), n_grow, 1 + uint32_t(rng() % 64), std::max<uint64_t>(1, n_grow) * (1 + rng() % 8) + rng() % 100);
        ++cases;
    }
    std::printf("%u cases, %d failures\n%s\n", cases, fails, fails ? "FAILED" : "fuzz done");
    return fails ? 1 : 0;
}
