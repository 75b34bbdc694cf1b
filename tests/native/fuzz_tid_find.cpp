// fuzz_tid_find.cpp -- tid_find of csrc/tid_lane.h under AddressSanitizer + UBSan on the CPU: the lane function cand_lookup_kernel of
// reranker.hip is a loop over.  A stand-alone program (tests/test_reranker_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_tid_find.cpp -o fuzz_tid_find && ./fuzz_tid_find
// Sorted keys WITH duplicates (the payloads of a handle's documents: two documents may share a ctid), sets of 0 .. 5000 keys, and the
// directory dir_shape / dir_source give for every directory size 0 .. 4 entries, 2048 and 4096 -- both heap blocks of exactly
// their sizes, so an index beyond either is a heap overflow here.  tid_find must equal std::lower_bound + equality: the FIRST
// position of the key or NOT_THERE, for keys below, between, equal to and above the set's.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/tid_lane.h"

using namespace vbm25::tid;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            if (++failures > 20) return 1;                \
        }                                                 \
    } while (0)

// the directory of at most `cap` entries over n keys: dir_shape's for a power of two, the same rule for the other sizes
static DirShape shape_for(uint64_t n, uint32_t cap) {
    if (cap == 0) return DirShape{0u, 1u};  // (only the empty set has no directory)
    if ((cap & (cap - 1)) == 0) {
        uint32_t log2 = 0;
        while ((1u << log2) < cap) ++log2;
        return dir_shape(n, log2);
    }
    if (n <= cap) return DirShape{uint32_t(n), 1u};
    const uint64_t stride = (n + cap - 1) / cap;
    return DirShape{uint32_t((n + stride - 1) / stride), uint32_t(stride)};
}

struct Sorted {
    std::vector<uint64_t> keys, dir;
    DirShape shape{};
    Sorted(std::vector<uint64_t> k, uint32_t cap) : keys(std::move(k)) {
        std::sort(keys.begin(), keys.end());  // (duplicates stay)
        keys.shrink_to_fit();
        shape = shape_for(keys.size(), cap);
        dir.reserve(shape.n_dir);
        for (uint32_t j = 0; j < shape.n_dir; ++j) dir.push_back(keys.at(dir_source(j, shape.stride)));
        dir.shrink_to_fit();
    }
    uint64_t find(uint64_t key) const {
        return tid_find(key, dir.empty() ? nullptr : dir.data(), shape.n_dir, keys.empty() ? nullptr : keys.data(), keys.size(), shape.stride);
    }
    uint64_t model(uint64_t key) const {
        const auto it = std::lower_bound(keys.begin(), keys.end(), key);
        return it != keys.end() && *it == key ? uint64_t(it - keys.begin()) : NOT_THERE;
    }
};

static int check(const Sorted &s, uint32_t cap, uint64_t &probes) {
    auto probe = [&](uint64_t key) {
        ++probes;
        return s.find(key) == s.model(key);
    };
    CHECK(probe(0) && probe(KEY_MAX), "n=%zu cap=%u: key 0 or 2^48 - 1", s.keys.size(), cap);
    for (size_t i = 0; i < s.keys.size(); ++i) {
        const uint64_t m = s.keys[i];
        CHECK(probe(m), "n=%zu cap=%u: key %012llx at %zu: got %llu, want %llu", s.keys.size(), cap, (unsigned long long)m, i,
              (unsigned long long)s.find(m), (unsigned long long)s.model(m));
        if (m > 0) CHECK(probe(m - 1), "n=%zu cap=%u: below %012llx", s.keys.size(), cap, (unsigned long long)m);
        if (m < KEY_MAX) CHECK(probe(m + 1), "n=%zu cap=%u: above %012llx", s.keys.size(), cap, (unsigned long long)m);
        if (i + 1 < s.keys.size() && s.keys[i + 1] - m > 1) CHECK(probe(m + (s.keys[i + 1] - m) / 2), "n=%zu cap=%u: between", s.keys.size(), cap);
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20261020);
    const uint32_t caps[] = {0, 1, 2, 3, 4, 2048, 4096};
    const size_t sizes[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129, 1000, 2047, 2048, 2049, 4095, 4096, 4097, 5000};
    uint64_t probes = 0, cases = 0;
    for (uint32_t cap : caps)
        for (size_t n : sizes) {
            if (cap == 0 && n) continue;
            for (int style = 0; style < 4; ++style) {
                std::vector<uint64_t> keys;
                // 0: distinct spread keys; 1: few values, long runs of duplicates (runs that span directory entries); 2: dense
                // neighbours with every third key doubled; 3: the extremes 0 and 2^48 - 1 among random keys, doubled
                for (size_t i = 0; i < n; ++i) {
                    switch (style) {
                        case 0: keys.push_back(rng() & KEY_MAX); break;
                        case 1: keys.push_back(((rng() % (n / 7 + 1)) * 1000003ull + 5) & KEY_MAX); break;
                        case 2: keys.push_back(1000 + 2 * (i - (i % 3 == 2))); break;
                        default: keys.push_back(i % 5 == 0 ? 0 : i % 5 == 1 ? KEY_MAX : rng() & KEY_MAX); break;
                    }
                }
                const Sorted s(std::move(keys), cap);
                CHECK(s.shape.n_dir <= (cap ? cap : 0u) && s.shape.stride >= 1, "n=%zu cap=%u: %u entries", n, cap, s.shape.n_dir);
                if (check(s, cap, probes)) return 1;
                ++cases;
            }
        }
    std::printf("%llu cases, %llu probes\n", (unsigned long long)cases, (unsigned long long)probes);
    if (failures) {
        std::printf("%d FAILURES\n", failures);
        return 1;
    }
    std::printf("fuzz done\n");
    return 0;
}
