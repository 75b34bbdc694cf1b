// fuzz_bigk_dense.cpp -- csrc/bigk_dense_lane.h on the CPU under AddressSanitizer + UBSan: the threshold search of the dense k > 1024
// route (histogram of the entries inside the interval -> walk -> settle or narrow, as bigk_dense_scan_kernel and
// bigk_dense_walk_kernel run it) and the emit's cut, against std::nth_element on the strict order "key descending, doc ascending".
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_bigk_dense.cpp -o fuzz_bigk_dense && ./fuzz_bigk_dense
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/bigk_dense_lane.h"

using namespace vbm25;

struct Cand {
    uint64_t key;
    uint32_t doc;
};
static bool before(const Cand &a, const Cand &b) { return bgk::beats(a.key, a.doc, b.key, b.doc); }
static uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}

static int fails = 0;
static uint32_t most_levels = 0, clips = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a level's histogram as a scan makes it and the walk kernel reads it
static uint64_t level_hist(const std::vector<Cand> &c, const bgd::State &st, std::vector<uint32_t> &hist, std::vector<uint32_t> &gsum) {
    hist.assign(bgd::BINS, 0);
    gsum.assign(bgd::WALK_THREADS, 0);
    const bgd::u128 lo = bgd::lo_of(st), top = bgd::top_of(st);
    uint64_t total = 0;
    for (const Cand &e : c) {
        const bgd::u128 x = bgd::composite(e.key, e.doc);
        CHECK(st.level != 0 || x <= top, "an entry above K_ub");
        if (!bgd::inside(x, lo, top)) continue;
        const uint32_t b = bgd::bin_of(x, top, st.shift);
        ++hist[b], ++gsum[b / bgd::WALK_GROUP], ++total;
    }
    return total;
}

// the whole search and the emit; returns the levels it took (cap_at_l0: the count "above + before + boundary bin" of level 0)
static uint32_t run(const std::vector<Cand> &c, uint32_t k, uint32_t cap, uint64_t k_ub, uint64_t *cap_at_l0 = nullptr) {
    bgd::State st = bgd::level0(k_ub);
    std::vector<uint32_t> hist, gsum;
    uint32_t levels = 0;
    bool clip = false;
    while (!st.settled && levels < bgd::MAX_LEVELS) {
        const uint64_t total = level_hist(c, st, hist, gsum);
        uint64_t bef = 0, bef1 = 0;
        const uint32_t d = bgd::walk_grouped(hist.data(), gsum.data(), k - st.above, bef);
        CHECK(d == bgd::walk(hist.data(), bgd::BINS, k - st.above, bef1) && bef == bef1, "the grouped walk differs");
        CHECK(st.level == 0 || d < bgd::BINS, "a later interval holds fewer than it must");
        if (levels == 0 && cap_at_l0) *cap_at_l0 = d < bgd::BINS ? bef + hist[d] : total;
        clip |= bgd::decide(st, k, cap, total, d, bef, d < bgd::BINS ? hist[d] : 0u);
        CHECK(st.above < k, "above reached k");
        ++levels;
    }
    CHECK(st.settled, "not settled after %u levels", levels);
    most_levels = std::max(most_levels, levels);
    clips += clip;
    std::vector<Cand> em, all = c;
    for (const Cand &e : c)
        if (bgd::composite(e.key, e.doc) >= bgd::lo_of(st)) em.push_back(e);
    const size_t want = std::min<size_t>(k, c.size());
    CHECK(em.size() <= cap && em.size() >= want, "%zu emitted, k %u, capacity %u, %zu entries", em.size(), k, cap, c.size());
    if (em.size() >= want) {
        std::nth_element(all.begin(), all.begin() + want, all.end(), before);
        std::nth_element(em.begin(), em.begin() + want, em.end(), before);
        std::sort(all.begin(), all.begin() + want, before);
        std::sort(em.begin(), em.begin() + want, before);
        for (size_t i = 0; i < want; ++i)
            if (all[i].key != em[i].key || all[i].doc != em[i].doc) {
                CHECK(false, "rank %zu differs", i);
                break;
            }
    }
    return levels;
}

int main() {
    std::mt19937_64 rng(7);
    uint32_t cases = 0;
    // kind 0: scores a few octaves below the bound; 1: far below it (the clip bin); 2: one tie mass; 3: a tie mass far below the
    // bound (clip bin, then every digit down to the last level); n below, at and above k
    for (uint32_t kind = 0; kind < 4; ++kind)
        for (uint32_t k : {1025u, 4097u})
            for (uint32_t n : {k - 1, k, k + 1, 3 * k, 20000u})
                for (uint32_t cap : {k, (k + 4095u) / 4096u * 4096u, 1u << 20}) {  // (k itself: the search must end on one value)
                    const double ub = kind == 1 || kind == 3 ? 3.0e6 : 24.0;
                    std::vector<Cand> c(n);
                    for (uint32_t i = 0; i < n; ++i) {
                        const double s = kind >= 2 ? 2.5 : kind == 1 ? 1.0 + double(rng() % 100000) * 1e-4 : 24.0 / (1.0 + double(rng() % 5000) * 0.01);
                        c[i] = Cand{bits(i % 97 == 0 && kind >= 2 ? s + 1.0 : s), uint32_t(i) * 3u + 1u};
                    }
                    std::shuffle(c.begin(), c.end(), rng);
                    const uint32_t levels = run(c, k, cap, bits(ub));
                    if (kind == 3 && n == 20000u && cap == k) CHECK(levels == bgd::MAX_LEVELS, "%u levels, not the last", levels);
                    ++cases;
                }
    // capacity edges: the level-0 count "above + boundary bin" equal to the capacity settles at level 0, one more entry does not
    for (uint32_t k : {1025u, 3000u}) {
        std::vector<Cand> c;
        for (uint32_t i = 0; i < 500; ++i) c.push_back(Cand{bits(20.0 + double(i) * 0.001), i});
        for (uint32_t i = 0; i < 6000; ++i) c.push_back(Cand{bits(3.0) + 1 + i % 7, 1000 + i});  // one level-0 bin (bits(3.0) itself is the top of the next)
        for (uint32_t i = 0; i < 4000; ++i) c.push_back(Cand{bits(0.5 + double(i) * 1e-5), 9000 + i});
        uint64_t at = 0;
        run(c, k, 1u << 20, bits(24.0), &at);
        CHECK(at == 6500, "the boundary count is %llu", (unsigned long long)at);
        CHECK(run(c, k, uint32_t(at), bits(24.0)) == 1, "above + bin = capacity did not settle at level 0");
        CHECK(run(c, k, uint32_t(at) - 1, bits(24.0)) > 1, "above + bin = capacity + 1 settled at level 0");
        cases += 3;
    }
    run({}, 1025, 4096, bgd::KUB_ALL);  // no entry, the bound of an untrusted s0
    ++cases;
    CHECK(most_levels == bgd::MAX_LEVELS && clips > 0, "levels %u, clip boundaries %u", most_levels, clips);
    std::printf("%u cases, most levels %u, clip boundaries %u\n", cases, most_levels, clips);
    std::printf(fails ? "FAILED\n" : "fuzz done\n");
    return fails != 0;
}
