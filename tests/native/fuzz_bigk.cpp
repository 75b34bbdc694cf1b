// fuzz_bigk.cpp -- csrc/bigk_lane.h on the CPU under AddressSanitizer + UBSan: the select of bigk_select_kernel (digit walk over
// histograms, boundary count, compaction) against std::nth_element, and the tile sort and rank of bigk_sort_kernel /
// bigk_rank_emit_kernel against std::sort, on the strict order "key descending, doc ascending".  Buffers are allocated exactly.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_bigk.cpp -o fuzz_bigk && ./fuzz_bigk
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/bigk_lane.h"
#include "../../vectorchord-bm25_amd/csrc/rerank_lane.h"

using namespace vbm25;

struct Cand {
    uint64_t key;
    uint32_t doc;
};
static bool before(const Cand &a, const Cand &b) { return bgk::beats(a.key, a.doc, b.key, b.doc); }

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the select as the workgroup runs it; returns the survivors in arrival order and the levels it took
static std::vector<Cand> select(const std::vector<Cand> &c, uint32_t k, uint32_t &levels) {
    levels = 0;
    if (c.size() <= k) return c;
    uint64_t b_key = 0;
    uint32_t b_doc = 0xffffffffu, need = k;
    for (uint32_t level = 0; level < bgk::LEVELS; ++level) {
        std::vector<uint32_t> hist(bgk::BINS, 0);
        for (const Cand &e : c)
            if (bgk::same_prefix(e.key, e.doc, b_key, b_doc, level)) ++hist[bgk::digit(e.key, e.doc, level)];
        bool exact = false;
        const uint32_t d = bgk::walk_digits(hist.data(), need, exact);
        bgk::set_digit(b_key, b_doc, level, d);
        levels = level + 1;
        if (exact) break;
    }
    std::vector<Cand> out;
    for (const Cand &e : c)
        if (bgk::keeps(e.key, e.doc, b_key, b_doc, levels)) out.push_back(e);
    return out;
}

// tiles of TILE sorted on the bitonic schedule, then every entry to its rank
static std::vector<Cand> sort_by_rank(const std::vector<Cand> &s) {
    const uint32_t ns = uint32_t(s.size()), n_tiles = (ns + bgk::TILE - 1) / bgk::TILE;
    std::vector<uint64_t> keys(ns);
    std::vector<uint32_t> docs(ns);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t first = t * bgk::TILE, m = std::min(bgk::TILE, ns - first), sn = rrk::sort_entries(m);
        std::vector<uint64_t> tk(sn, bgk::WORST_KEY);
        std::vector<uint32_t> td(sn, bgk::WORST_DOC);
        for (uint32_t i = 0; i < m; ++i) tk[i] = s[first + i].key, td[i] = s[first + i].doc;
        for (uint32_t size = 2; size <= sn; size <<= 1)
            for (uint32_t stride = size >> 1; stride; stride >>= 1)
                for (uint32_t x = 0; x < sn / 2; ++x) {
                    uint32_t i, j;
                    rrk::bitonic_pair(x, stride, i, j);
                    rrk::exchange(tk[i], td[i], tk[j], td[j], rrk::bitonic_best_first(i, size));
                }
        for (uint32_t i = 0; i < m; ++i) keys[first + i] = tk[i], docs[first + i] = td[i];
    }
    std::vector<Cand> out(ns, Cand{0, 0});
    std::vector<uint8_t> taken(ns, 0);
    for (uint32_t i = 0; i < ns; ++i) {
        uint32_t rank = i % bgk::TILE;
        for (uint32_t u = 0; u < n_tiles; ++u)
            if (u != i / bgk::TILE)
                rank += bgk::count_beating(keys.data() + u * bgk::TILE, docs.data() + u * bgk::TILE, std::min(bgk::TILE, ns - u * bgk::TILE), keys[i], docs[i]);
        CHECK(rank < ns && !taken[rank], "rank %u of entry %u (of %u) is taken or out of range", rank, i, ns);
        if (rank < ns) out[rank] = Cand{keys[i], docs[i]}, taken[rank] = 1;
    }
    return out;
}

int main() {
    std::mt19937_64 rng(12345);
    int cases = 0;
    // key shapes: all equal, two values, a few values, doubles' bit patterns, full random; docs: dense from 0, sparse, around 2^32 - 1
    const uint32_t counts[] = {1, 2, 63, 64, 65, 255, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 20000};
    for (uint32_t n : counts)
        for (int shape = 0; shape < 5; ++shape)
            for (int dshape = 0; dshape < 3; ++dshape) {
                std::vector<uint32_t> docs(n);
                for (uint32_t i = 0; i < n; ++i)
                    docs[i] = dshape == 0 ? i : dshape == 1 ? i * 9973u + 17u : 0xffffffffu - i * 3u;
                std::shuffle(docs.begin(), docs.end(), rng);
                std::vector<Cand> c(n);
                for (uint32_t i = 0; i < n; ++i) {
                    uint64_t key;
                    if (shape == 0) key = 0x4008000000000000ull;
                    else if (shape == 1) key = 0x4008000000000000ull + (rng() & 1);
                    else if (shape == 2) key = 0x3ff0000000000000ull + ((rng() % 7) << (8 * (rng() % 7)));
                    else if (shape == 3) key = 0x3ff0000000000000ull + (rng() >> 14);
                    else key = rng() | 1ull;
                    c[i] = Cand{key, docs[i]};
                }
                for (uint32_t k : {1u, n / 2 ? n / 2 : 1u, n > 1 ? n - 1 : 1u, n, n + 1, 1025u, 4096u, 4097u}) {
                    uint32_t levels = 0;
                    std::vector<Cand> surv = select(c, k, levels);
                    const uint32_t want_n = std::min<uint32_t>(k, n);
                    CHECK(surv.size() == want_n, "n %u k %u shape %d/%d: %zu survivors", n, k, shape, dshape, surv.size());
                    std::vector<Cand> ref = c;
                    if (k < n) std::nth_element(ref.begin(), ref.begin() + (k - 1), ref.end(), before);
                    ref.resize(want_n);
                    std::sort(ref.begin(), ref.end(), before);
                    if (k < n && shape == 0) CHECK(levels > 8, "equal keys decided in %u levels", levels);
                    std::vector<Cand> got = sort_by_rank(surv);
                    bool same = got.size() == ref.size();
                    for (size_t i = 0; same && i < ref.size(); ++i) same = got[i].key == ref[i].key && got[i].doc == ref[i].doc;
                    CHECK(same, "n %u k %u shape %d/%d: records differ from nth_element + sort", n, k, shape, dshape);
                    ++cases;
                }
            }
    // the host's item cut: within the index's windows, and the batch's items within the cap unless an item is already a whole query
    for (uint32_t n_win : {1u, 2u, 5u, 1221u})
        for (uint32_t n_q : {1u, 7u, 4096u})
            for (uint32_t wanted : {0u, 1u, 3u, 1u << 20})
                for (uint64_t cap : {uint64_t(1), uint64_t(4096), uint64_t(1) << 20}) {
                    const uint32_t wpi = bgk::item_windows(n_win, n_q, wanted, 2048, cap);
                    const bool fits = uint64_t(n_q) * ((n_win + wpi - 1) / wpi) <= cap;
                    CHECK(wpi >= 1 && wpi <= n_win && (fits || wpi == n_win), "n_win %u n_q %u wanted %u: wpi %u", n_win, n_q, wanted, wpi);
                    if (wanted && fits && wanted <= n_win && uint64_t(n_q) * ((n_win + wanted - 1) / wanted) <= cap) CHECK(wpi == wanted, "wanted %u: wpi %u", wanted, wpi);
                }
    std::printf("%d cases\n", cases);
    std::printf(fails ? "FAILED %d\n" : "fuzz done\n", fails);
    return fails ? 1 : 0;
}
