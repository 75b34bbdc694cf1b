// fuzz_forward.cpp -- csrc/forward_lane.h under AddressSanitizer + UBSan on the CPU: the functions the sort kernels of forward.hip are
// made of, driven as a wave and as a workgroup drive them.  A stand-alone program (tests/test_forward_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_forward.cpp -o fuzz_forward && ./fuzz_forward
// Runs of every length 0 .. 130 and of the class edges (2047, 2048, 2049, 5000), each in several arrival orders: distinct term ids
// (the largest and the smallest legal ones among them) with their tfs, shuffled as the cursors' atomics may leave them.
//   the model wave       64 lanes hold one element each (the lanes behind the run the padding); every step of the network each lane
//                        reads its partner's element of the PREVIOUS step (the shuffle) and cx_take decides -- runs up to 64
//   the model workgroup  256 threads over an array of exactly padded_len elements (an index beyond it is a heap overflow here): thread
//                        t takes the pairs t, t + 256 .. of a step, pair_low / pair_ascending / pair_swaps decide -- runs up to 2048
// Both against std::sort of the (term, tf) pairs.  Then run_class at every length around both bounds for several settings of the
// bounds, padded_len, slot_of and next_step's walk.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/forward_lane.h"

using namespace vbm25::fwd;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            if (++failures > 20) return 1;                   \
        }                                                    \
    } while (0)

using Run = std::vector<std::pair<uint32_t, uint32_t>>;  // (term, tf)

// a run of `len` distinct terms in an arbitrary order
static Run make_run(uint32_t len, std::mt19937 &rng, int order) {
    std::vector<uint32_t> terms;
    terms.reserve(len);
    uint32_t t = rng() % 3 == 0 ? 0u : rng() % 1000u;
    for (uint32_t i = 0; i < len; ++i) {
        terms.push_back(t);
        t += 1u + rng() % (order == 3 ? 2u : 100000u);
    }
    if (len >= 2 && order == 2) terms[len - 1] = 0xfffffffeu;  // the largest id a term can have: one below the padding
    Run run;
    run.reserve(len);
    for (uint32_t x : terms) run.emplace_back(x, 1u + rng() % 70000u);
    if (order == 1) std::reverse(run.begin(), run.end());
    else if (order >= 2) std::shuffle(run.begin(), run.end(), rng);
    return run;
}

static int wave_sort(const Run &in, Run &out) {
    const uint32_t len = uint32_t(in.size()), p = padded_len(len);
    CHECK(len <= 64 && p <= 64, "a wave run of %u", len);
    uint32_t key[64], val[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
        key[lane] = lane < len ? in[lane].first : PAD_TERM;
        val[lane] = lane < len ? in[lane].second : 0u;
    }
    for (uint32_t k = 2, j = 1; k <= p; next_step(k, j)) {
        uint32_t pk[64], pv[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {  // the shuffle: every lane reads before any lane writes
            const uint32_t from = cx_partner(lane, j);
            CHECK(from < 64, "lane %u step (%u, %u) reads lane %u", lane, k, j, from);
            pk[lane] = key[from];
            pv[lane] = val[from];
        }
        for (uint32_t lane = 0; lane < 64; ++lane) cx_take(lane, k, j, key[lane], val[lane], pk[lane], pv[lane]);
    }
    out.clear();
    for (uint32_t lane = 0; lane < len; ++lane) out.emplace_back(key[lane], val[lane]);
    for (uint32_t lane = len; lane < 64; ++lane) CHECK(key[lane] == PAD_TERM, "run of %u: lane %u lost its padding", len, lane);
    return 0;
}

static int group_sort(const Run &in, Run &out) {
    constexpr uint32_t WG = 256;
    const uint32_t len = uint32_t(in.size()), p = padded_len(len);
    CHECK(len <= FWD_GROUP_MAX && p <= FWD_GROUP_MAX, "a workgroup run of %u", len);
    std::vector<uint32_t> key(p), val(p);  // exactly the network's size
    for (uint32_t i = 0; i < p; ++i) {
        key[i] = i < len ? in[i].first : PAD_TERM;
        val[i] = i < len ? in[i].second : 0u;
    }
    std::vector<uint8_t> touched(p);
    for (uint32_t k = 2, j = 1; k <= p; next_step(k, j)) {
        std::fill(touched.begin(), touched.end(), 0);
        for (uint32_t thread = 0; thread < WG; ++thread)
            for (uint32_t t = thread; t < (p >> 1); t += WG) {
                const uint32_t lo = pair_low(t, j), hi = lo | j;
                CHECK(hi < p && !(lo & j), "pair %u of step (%u, %u): elements %u, %u of %u", t, k, j, lo, hi, p);
                CHECK(!touched[lo] && !touched[hi], "step (%u, %u): two pairs share an element", k, j);  // (no barrier inside a step)
                touched[lo] = touched[hi] = 1;
                if (pair_swaps(key.at(lo), key.at(hi), pair_ascending(lo, k))) {
                    std::swap(key.at(lo), key.at(hi));
                    std::swap(val.at(lo), val.at(hi));
                }
            }
    }
    out.clear();
    for (uint32_t i = 0; i < len; ++i) out.emplace_back(key[i], val[i]);
    for (uint32_t i = len; i < p; ++i) CHECK(key[i] == PAD_TERM, "run of %u: element %u lost its padding", len, i);
    return 0;
}

static int check_run(uint32_t len, std::mt19937 &rng, unsigned &cases) {
    for (int order = 0; order < 5; ++order) {
        const Run in = make_run(len, rng, order);
        Run want = in, got;
        std::sort(want.begin(), want.end());
        if (len <= FWD_WAVE_MAX) {
            if (wave_sort(in, got)) return 1;
            CHECK(got == want, "the wave's sort of a run of %u (order %d) differs from std::sort", len, order);
        }
        if (len <= FWD_GROUP_MAX) {
            if (group_sort(in, got)) return 1;
            CHECK(got == want, "the workgroup's sort of a run of %u (order %d) differs from std::sort", len, order);
        }
        ++cases;
    }
    return 0;
}

static int check_classes() {
    const uint32_t bounds[][2] = {{FWD_WAVE_MAX, FWD_GROUP_MAX}, {8, 65}, {0, FWD_GROUP_MAX}, {0, 0}, {64, 64}, {1, 2047}, {64, 0}};
    for (const auto &b : bounds)
        for (uint64_t len = 0; len <= 5001; ++len) {
            const uint32_t c = run_class(len, b[0], b[1]);
            const uint32_t want = len <= b[0] ? RUN_WAVE : len <= b[1] ? RUN_GROUP : RUN_LONG;
            CHECK(c == want, "run_class(%llu, %u, %u) = %u", (unsigned long long)len, b[0], b[1], c);
            if (c == RUN_WAVE) CHECK(len <= FWD_WAVE_MAX, "a wave run of %llu", (unsigned long long)len);
            if (c == RUN_GROUP) CHECK(len <= FWD_GROUP_MAX, "a workgroup run of %llu", (unsigned long long)len);
        }
    CHECK(run_class(1ull << 33, FWD_WAVE_MAX, FWD_GROUP_MAX) == RUN_LONG, "a run beyond 2^32");
    CHECK(run_class(0, FWD_WAVE_MAX, FWD_GROUP_MAX) == RUN_WAVE && run_class(64, 64, 2048) == RUN_WAVE && run_class(65, 64, 2048) == RUN_GROUP &&
              run_class(2048, 64, 2048) == RUN_GROUP && run_class(2049, 64, 2048) == RUN_LONG,
          "the class edges");
    for (uint32_t len = 0; len <= FWD_GROUP_MAX; ++len) {
        const uint32_t p = padded_len(len);
        CHECK(p >= 2 && p >= len && (p & (p - 1)) == 0 && (p == 2 || p / 2 < len) && p <= FWD_GROUP_MAX, "padded_len(%u) = %u", len, p);
    }
    CHECK(slot_of(0, 0) == 0 && slot_of((1ull << 32) + 5, 7) == (1ull << 32) + 12 && slot_of(~0ull - 0xffffffffull, 0xffffffffu) == ~0ull, "slot_of");
    // the walk: log2(P) (log2(P) + 1) / 2 steps, j a power of two below k
    for (uint32_t p = 2; p <= FWD_GROUP_MAX; p <<= 1) {
        uint32_t steps = 0, lg = 0;
        while ((1u << lg) < p) ++lg;
        for (uint32_t k = 2, j = 1; k <= p; next_step(k, j)) {
            CHECK(j >= 1 && j < k && (j & (j - 1)) == 0 && (k & (k - 1)) == 0, "step (%u, %u)", k, j);
            ++steps;
        }
        CHECK(steps == lg * (lg + 1) / 2, "%u steps for %u elements", steps, p);
    }
    return 0;
}

int main() {
    std::mt19937 rng(20261020);
    unsigned cases = 0;
    for (uint32_t len = 0; len <= 130; ++len)
        if (check_run(len, rng, cases)) return 1;
    for (uint32_t len : {255u, 256u, 257u, 1023u, 1025u, 2047u, 2048u})
        if (check_run(len, rng, cases)) return 1;
    // beyond the workgroup class nothing of this header sorts: the class says so
    for (uint32_t len : {2049u, 5000u}) CHECK(run_class(len, FWD_WAVE_MAX, FWD_GROUP_MAX) == RUN_LONG, "a run of %u", len);
    if (check_classes()) return 1;
    std::printf("%u cases\n", cases);
    if (failures) {
        std::printf("%d FAILures\n", failures);
        return 1;
    }
    std::printf("fuzz done\n");
    return 0;
}
