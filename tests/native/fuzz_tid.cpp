// fuzz_tid.cpp -- csrc/tid_lane.h under AddressSanitizer + UBSan on the CPU: the functions tid_match_kernel of tid.hip is made of,
// driven as its waves drive them.  A stand-alone program (tests/test_tid_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_tid.cpp -o fuzz_tid && ./fuzz_tid
// 200 seeded sets: the sorted distinct keys and the directory dir_shape / dir_source give are allocated to exactly their sizes (an
// index beyond either is a heap overflow here), for every directory size from 2^0 up, and tid_contains must agree with
// std::binary_search on every member, every member +- 1 in each of the three fields, keys 0 and 2^48 - 1 and keys that differ from a
// member in one field only.  Then a model wave: 64 lanes vote, match_word makes the word (tail bits, invert), the OR mode counts
// new_bits -- against a plain loop over the documents.
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

static uint64_t key_of(uint16_t a, uint16_t b, uint16_t c) {
    const uint16_t p[3] = {a, b, c};
    return tid_key(p);
}

// a set as tid.hip keeps it: the keys and the directory, each a heap block of exactly its size
struct Set {
    std::vector<uint64_t> keys, dir;
    DirShape shape{};
    Set(std::vector<uint64_t> k, uint32_t dir_log2) : keys(std::move(k)) {
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        keys.shrink_to_fit();
        shape = dir_shape(keys.size(), dir_log2);
        dir.reserve(shape.n_dir);
        for (uint32_t j = 0; j < shape.n_dir; ++j) dir.push_back(keys.at(dir_source(j, shape.stride)));
        dir.shrink_to_fit();
    }
    bool contains(uint64_t key) const {
        return tid_contains(key, dir.empty() ? nullptr : dir.data(), shape.n_dir, keys.empty() ? nullptr : keys.data(), keys.size(), shape.stride);
    }
    bool model(uint64_t key) const { return std::binary_search(keys.begin(), keys.end(), key); }
};

static int check_shape(const Set &s, uint32_t dir_log2) {
    const uint64_t n = s.keys.size(), cap = 1ull << dir_log2;
    CHECK(s.shape.n_dir <= cap && s.shape.stride >= 1, "n=%llu dir_log2=%u: %u entries", (unsigned long long)n, dir_log2, s.shape.n_dir);
    if (n <= cap) CHECK(s.shape.n_dir == n && s.shape.stride == 1, "n=%llu dir_log2=%u: a small set is its own directory", (unsigned long long)n, dir_log2);
    else {
        // the runs cover the keys: the last entry's run reaches the end, none starts beyond it
        CHECK(dir_source(s.shape.n_dir - 1, s.shape.stride) < n, "n=%llu dir_log2=%u: the last run starts beyond the keys", (unsigned long long)n, dir_log2);
        CHECK(dir_source(s.shape.n_dir, s.shape.stride) >= n, "n=%llu dir_log2=%u: keys behind the last run", (unsigned long long)n, dir_log2);
    }
    return 0;
}

static int check_set(const Set &s, uint32_t dir_log2, uint64_t &probes) {
    if (check_shape(s, dir_log2)) return 1;
    auto probe = [&](uint64_t key) {
        ++probes;
        return s.contains(key) == s.model(key);
    };
    CHECK(probe(0) && probe(KEY_MAX), "n=%zu dir_log2=%u: key 0 or 2^48 - 1", s.keys.size(), dir_log2);
    for (uint64_t m : s.keys) {
        CHECK(s.contains(m), "n=%zu dir_log2=%u: member %012llx not found", s.keys.size(), dir_log2, (unsigned long long)m);
        ++probes;
        const uint16_t f[3] = {uint16_t(m >> 32), uint16_t(m >> 16), uint16_t(m)};
        for (int field = 0; field < 3; ++field) {
            for (int delta : {-1, 1, 2, 256, 0x7fff}) {  // the field alone moves (it wraps inside its 16 bits): a packing mistake shows
                uint16_t g[3] = {f[0], f[1], f[2]};
                g[field] = uint16_t(g[field] + delta);
                const uint64_t key = tid_key(g);
                CHECK(probe(key), "n=%zu dir_log2=%u: member %012llx, field %d %+d", s.keys.size(), dir_log2, (unsigned long long)m, field, delta);
            }
            // +- 1 of the key as an integer at the field's position (with carry into the fields above)
            const uint64_t unit = 1ull << (16 * (2 - field));
            if (m >= unit) CHECK(probe(m - unit), "n=%zu dir_log2=%u: member %012llx - unit %d", s.keys.size(), dir_log2, (unsigned long long)m, field);
            if (m + unit <= KEY_MAX) CHECK(probe(m + unit), "n=%zu dir_log2=%u: member %012llx + unit %d", s.keys.size(), dir_log2, (unsigned long long)m, field);
        }
    }
    return 0;
}

// a model wave over `n` documents with payload keys doc[], the plain loop beside it
static int check_words(const Set &s, const std::vector<uint64_t> &doc, std::mt19937_64 &rng) {
    const uint64_t n = doc.size(), n_words = (n + 63) / 64;
    for (int invert = 0; invert < 2; ++invert) {
        std::vector<uint64_t> words(n_words), old(n_words), ored;
        for (uint64_t &w : old) w = rng() & rng();
        if (n & 63) if (n_words) old[n_words - 1] &= (1ull << (n & 63)) - 1;
        ored = old;
        uint32_t counted = 0, fresh = 0;
        for (uint64_t w = 0; w < n_words; ++w) {
            uint64_t ballot = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint64_t d = (w << 6) + lane;
                const bool hit = d < n && s.contains(doc.at(d));  // (lanes at or beyond n vote 0)
                ballot |= uint64_t(hit) << lane;
            }
            words.at(w) = match_word(ballot, w << 6, n, invert ? ~0ull : 0ull);
            counted += popcount64(words[w]);
            if (!invert) {
                fresh += new_bits(ored.at(w), words[w]);
                ored[w] |= words[w];
            }
        }
        uint32_t want_count = 0, want_fresh = 0;
        for (uint64_t d = 0; d < 64 * n_words; ++d) {
            const bool want = d < n && (s.model(doc[d]) != (invert != 0));
            const bool got = (words[d >> 6] >> (d & 63)) & 1;
            CHECK(got == want, "n=%llu invert=%d: bit %llu", (unsigned long long)n, invert, (unsigned long long)d);
            want_count += want;
            if (!invert) {
                const bool was = (old[d >> 6] >> (d & 63)) & 1;
                want_fresh += want && !was;
                CHECK((((ored[d >> 6] >> (d & 63)) & 1) != 0) == (want || was), "n=%llu: OR bit %llu", (unsigned long long)n, (unsigned long long)d);
            }
        }
        CHECK(counted == want_count, "n=%llu invert=%d: %u counted, %u set", (unsigned long long)n, invert, counted, want_count);
        if (!invert) CHECK(fresh == want_fresh, "n=%llu: %u new, %u expected", (unsigned long long)n, fresh, want_fresh);
    }
    return 0;
}

int main() {
    // tid_key: the packing
    if (key_of(1, 2, 3) != ((1ull << 32) | (2ull << 16) | 3ull) || key_of(0xffff, 0xffff, 0xffff) != KEY_MAX || key_of(0, 0, 0) != 0 ||
        !(key_of(0, 0xffff, 0xffff) < key_of(1, 0, 0)) || !(key_of(5, 0, 0xffff) < key_of(5, 1, 0))) {
        std::printf("FAIL tid_key\n");
        return 1;
    }
    uint64_t probes = 0;
    int cases = 0;
    for (int seed = 0; seed < 200; ++seed, ++cases) {
        std::mt19937_64 rng(seed);
        const uint32_t dir_log2 = seed % (MAX_DIR_LOG2 + 1);  // every tid_dir from 0 up
        const uint64_t D = 1ull << dir_log2;
        // the sizes around the directory's, the smallest, and sizes whose stride does not divide them
        const uint64_t sizes[] = {0, 1, 2, D > 1 ? D - 1 : 3, D, D + 1, 2 * D + 1, 3 * D + (rng() % (D + 1)), 1 + rng() % 3000, 7 * D - 1};
        const uint64_t n = sizes[(seed / (MAX_DIR_LOG2 + 1)) % 10];
        // keys that collide in two of three fields: few distinct values a field
        const uint32_t spread = (seed & 1) ? 4 : 65536;
        std::vector<uint64_t> keys;
        while (keys.size() < n) {
            keys.push_back(key_of(uint16_t(rng() % spread), uint16_t(rng() % spread), uint16_t(rng() % 65536)));
            if (keys.size() == n) {
                std::sort(keys.begin(), keys.end());
                keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            }
        }
        if (n >= 2 && (seed % 3) == 0) keys[0] = 0, keys[1] = KEY_MAX;  // the extreme keys as members
        Set s(keys, dir_log2);
        if (check_set(s, dir_log2, probes)) return 1;
        // documents: members, near misses and strangers, a count that is no multiple of 64 most of the time
        const uint64_t n_docs = (seed % 5 == 0) ? 64 * (1 + seed % 3) : 1 + rng() % 300;
        std::vector<uint64_t> doc(n_docs);
        for (uint64_t &d : doc) {
            const uint64_t r = rng() % 3;
            d = (r == 0 || s.keys.empty()) ? (rng() & KEY_MAX) : s.keys[rng() % s.keys.size()] ^ (r == 2 ? 1ull << (rng() % 48) : 0);
        }
        if (check_words(s, doc, rng)) return 1;
    }
    // every size from 0 to 40 under every small directory: each stride that does not divide, each boundary
    for (uint32_t dir_log2 = 0; dir_log2 <= 4; ++dir_log2)
        for (uint64_t n = 0; n <= 40; ++n) {
            std::vector<uint64_t> keys;
            for (uint64_t i = 0; i < n; ++i) keys.push_back(3 * i + 1);
            Set s(keys, dir_log2);
            if (check_shape(s, dir_log2)) return 1;
            for (uint64_t key = 0; key <= 3 * n + 3; ++key, ++probes) CHECK(s.contains(key) == s.model(key), "n=%llu dir_log2=%u key %llu", (unsigned long long)n, dir_log2, (unsigned long long)key);
        }
    // the largest set a handle takes: the shape's arithmetic does not wrap
    for (uint32_t dir_log2 = 0; dir_log2 <= MAX_DIR_LOG2; ++dir_log2) {
        const uint64_t n = 0xffffffffull;
        const DirShape sh = dir_shape(n, dir_log2);
        CHECK(sh.n_dir >= 1 && sh.n_dir <= (1ull << dir_log2) && dir_source(sh.n_dir - 1, sh.stride) < n && dir_source(sh.n_dir, sh.stride) >= n,
              "2^32 - 1 keys, dir_log2=%u", dir_log2);
    }
    if (failures) return 1;
    std::printf("%d cases, %llu probes\nfuzz done\n", cases, (unsigned long long)probes);
    return 0;
}
