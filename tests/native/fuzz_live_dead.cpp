// fuzz_live_dead.cpp -- the per-lane functions of the deletes on a bound handle (csrc/tid_lane.h: tid_first_live, split_payload, with
// tid_find, tid_contains, match_word and new_bits around them) under AddressSanitizer + UBSan on the CPU, driven as cand_lookup_kernel
// of reranker.hip and live_dead_tids_kernel of live.hip drive them.  A stand-alone program (tests/test_live_delete_host.py builds and
// runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_live_dead.cpp -o fuzz_live_dead && ./fuzz_live_dead
// Every array is a heap block of exactly its size, so an index beyond one is a heap overflow here.
//   1. the walk: sorted keys in runs of 1 .. 5 equal keys, documents ascending inside a run, and for one run after the other EVERY dead
//      pattern of its documents (the other runs' patterns random); directories of 1 .. 4, 2048 and 4096 entries.  Every key, and keys
//      nobody carries, are looked up as the kernel does -- tid_find, then tid_first_live -- against a linear scan for the lowest live
//      document of the key.
//   2. the word: a model wave of 64 lanes answers word w of a handle of base_docs + n_tail documents, each lane taking its ctid from
//      the base plane or the tail (split_payload), one "ballot" a word through match_word, ORed into words that already hold bits and
//      counted by new_bits -- against a loop over the bits.  base_docs of 0, 1, 59, 64, 70 and 300 with tails of 0, 1, 58, 59 and 200.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/tid_lane.h"

using namespace vbm25::tid;

static int failures = 0;
static long cases = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            if (++failures > 20) return 1;                   \
        }                                                    \
    } while (0)

template <class T>
static std::vector<T> exact(const std::vector<T> &v) {  // a block of exactly size() elements
    std::vector<T> out(v);
    out.shrink_to_fit();
    return out;
}

static DirShape shape_for(uint64_t n, uint32_t cap) {
    if (cap == 0) return DirShape{0u, 1u};
    if ((cap & (cap - 1)) == 0) {
        uint32_t log2 = 0;
        while ((1u << log2) < cap) ++log2;
        return dir_shape(n, log2);
    }
    if (n <= cap) return DirShape{uint32_t(n), 1u};
    const uint64_t stride = (n + cap - 1) / cap;
    return DirShape{uint32_t((n + stride - 1) / stride), uint32_t(stride)};
}

static std::vector<uint64_t> directory(const std::vector<uint64_t> &keys, const DirShape &s) {
    std::vector<uint64_t> d;
    for (uint32_t j = 0; j < s.n_dir; ++j) d.push_back(keys[dir_source(j, s.stride)]);
    return exact(d);
}

static int walk_case(std::mt19937_64 &rng, uint32_t n_runs, uint32_t dir_cap) {
    // the runs: distinct ascending keys, 1 .. 5 entries each; the documents a permutation of 0 .. n, sorted inside each run
    std::vector<uint32_t> run_len(n_runs);
    uint32_t n = 0;
    for (auto &l : run_len) n += (l = 1 + uint32_t(rng() % 5));
    std::vector<uint64_t> run_key;
    {
        std::set<uint64_t> ks;
        ks.insert(0);  // (the keys 0 and 2^48 - 1 are keys like any other)
        ks.insert(KEY_MAX);
        while (ks.size() < std::max<size_t>(n_runs, 2)) ks.insert((rng() & KEY_MAX) | 1ull);
        run_key.assign(ks.begin(), ks.end());
        while (run_key.size() > n_runs) run_key.erase(run_key.begin() + 1);
    }
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; ++i) perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<uint64_t> keys;
    std::vector<uint32_t> docs, run_at;
    for (uint32_t r = 0, at = 0; r < n_runs; at += run_len[r], ++r) {
        run_at.push_back(at);
        std::sort(perm.begin() + at, perm.begin() + at + run_len[r]);
        for (uint32_t i = 0; i < run_len[r]; ++i) keys.push_back(run_key[r]), docs.push_back(perm[at + i]);
    }
    const std::vector<uint64_t> k = exact(keys);
    const std::vector<uint32_t> d = exact(docs);
    const DirShape shape = shape_for(n, dir_cap);
    const std::vector<uint64_t> dir = directory(k, shape);
    // the keys asked for: every run's, and neighbours nobody carries
    std::vector<uint64_t> ask(run_key);
    for (uint64_t key : run_key) {
        if (key && !std::binary_search(run_key.begin(), run_key.end(), key - 1)) ask.push_back(key - 1);
        if (key < KEY_MAX && !std::binary_search(run_key.begin(), run_key.end(), key + 1)) ask.push_back(key + 1);
    }
    // (a large set: a sample of the runs, each with its own key, its neighbours and a few other runs' keys)
    const bool large = n_runs > 64;
    const std::vector<uint64_t> all_asks = ask;
    for (uint32_t r = 0; r < n_runs; r += large ? n_runs / 24 : 1)
        for (uint32_t pattern = 0; pattern < (1u << run_len[r]); ++pattern) {
            if (large) {
                ask = {run_key[r], run_key[r] + 1 < KEY_MAX ? run_key[r] + 1 : 5, run_key[r] ? run_key[r] - 1 : 7};
                for (int i = 0; i < 5; ++i) ask.push_back(all_asks[rng() % all_asks.size()]);
            }
            std::vector<uint64_t> dead((size_t(n) + 63) / 64, 0);
            dead.shrink_to_fit();
            for (uint32_t i = 0; i < n; ++i)
                if (rng() & 1) dead[d[i] >> 6] |= 1ull << (d[i] & 63);
            for (uint32_t i = 0; i < run_len[r]; ++i) {
                const uint32_t doc = d[run_at[r] + i];
                dead[doc >> 6] &= ~(1ull << (doc & 63));
                if (pattern >> i & 1) dead[doc >> 6] |= 1ull << (doc & 63);
            }
            for (uint64_t key : ask) {
                uint32_t want = NO_LIVE_DOC;
                bool present = false;
                for (uint32_t i = 0; i < n; ++i)
                    if (k[i] == key) {
                        present = true;
                        if (!dead_bit(dead.data(), d[i]) && d[i] < want) want = d[i];
                    }
                const uint64_t at = tid_find(key, dir.data(), shape.n_dir, k.data(), n, shape.stride);
                CHECK((at != NOT_THERE) == present, "tid_find of key %llx: %llu", (unsigned long long)key, (unsigned long long)at);
                const uint32_t got = at == NOT_THERE ? NO_LIVE_DOC : tid_first_live(at, key, k.data(), d.data(), n, dead.data());
                CHECK(got == want, "runs %u dir %u run %u pattern %x key %llx: document %u, the scan has %u", n_runs, dir_cap, r, pattern,
                      (unsigned long long)key, got, want);
                ++cases;
            }
        }
    return 0;
}

static int word_case(std::mt19937_64 &rng, uint32_t base_docs, uint32_t n_tail, uint32_t dir_log2, int set_kind) {
    const uint32_t n = base_docs + n_tail;
    if (!n) return 0;
    // the ctids: mostly distinct, some shared between the base and the tail, the extreme keys among them
    std::vector<uint16_t> base(3 * size_t(base_docs)), tail(3 * size_t(n_tail));
    auto fill = [&](std::vector<uint16_t> &p, size_t i) {
        const uint64_t key = rng() % 7 == 0 ? rng() % 5 : rng() & KEY_MAX;
        p[3 * i] = uint16_t(key >> 32), p[3 * i + 1] = uint16_t(key >> 16), p[3 * i + 2] = uint16_t(key);
    };
    for (size_t i = 0; i < base_docs; ++i) fill(base, i);
    for (size_t i = 0; i < n_tail; ++i) fill(tail, i);
    if (base_docs) base[0] = base[1] = base[2] = 0;
    if (n_tail) tail[3 * (n_tail - 1)] = tail[3 * (n_tail - 1) + 1] = tail[3 * (n_tail - 1) + 2] = 0xFFFF;
    base.shrink_to_fit();
    tail.shrink_to_fit();
    auto key_of = [&](uint32_t d) { return d < base_docs ? tid_key(&base[3 * size_t(d)]) : tid_key(&tail[3 * size_t(d - base_docs)]); };
    // the set: empty, one ctid, all ctids, absent ctids only, a random half
    std::set<uint64_t> set;
    if (set_kind == 1) set.insert(key_of(uint32_t(rng() % n)));
    if (set_kind == 2)
        for (uint32_t d = 0; d < n; ++d) set.insert(key_of(d));
    if (set_kind == 3)
        for (int i = 0; i < 50; ++i) set.insert(((rng() & KEY_MAX) | 0x800000000000ull) ^ 0x5a5a);
    if (set_kind == 4)
        for (uint32_t d = 0; d < n; ++d)
            if (rng() & 1) set.insert(key_of(d));
    if (set_kind == 3)
        for (uint32_t d = 0; d < n; ++d) set.erase(key_of(d));
    const std::vector<uint64_t> keys = exact(std::vector<uint64_t>(set.begin(), set.end()));
    const DirShape shape = dir_shape(keys.size(), dir_log2);
    const std::vector<uint64_t> dir = directory(keys, shape);
    const uint32_t n_words = (n + 63) / 64;
    std::vector<uint64_t> words(n_words, 0), want(n_words, 0);
    words.shrink_to_fit();
    for (uint32_t d = 0; d < n; ++d)
        if (rng() % 4 == 0) words[d >> 6] |= 1ull << (d & 63);  // (bits of earlier deletes)
    want = words;
    uint32_t want_new = 0;
    for (uint32_t d = 0; d < n; ++d)
        if (set.count(key_of(d)) && !(want[d >> 6] >> (d & 63) & 1)) want[d >> 6] |= 1ull << (d & 63), ++want_new;
    // the kernel's loop: wave w answers word w
    uint32_t counted = 0;
    for (uint64_t w = 0; w < n_words; ++w) {
        uint64_t ballot = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t d = (w << 6) + lane;
            bool hit = false;
            if (d < n) {
                const uint16_t *p = split_payload(base.data(), tail.data(), base_docs, d);
                const uint16_t p3[3] = {p[0], p[1], p[2]};
                hit = tid_contains(tid_key(p3), dir.data(), shape.n_dir, keys.data(), keys.size(), shape.stride);
            }
            ballot |= uint64_t(hit) << lane;
        }
        const uint64_t word = match_word(ballot, w << 6, n, 0);
        const uint64_t old = words[w];
        counted += new_bits(old, word);
        if (word & ~old) words[w] = old | word;
    }
    CHECK(words == want, "base %u tail %u dir %u set %d: the words differ", base_docs, n_tail, dir_log2, set_kind);
    CHECK(counted == want_new, "base %u tail %u dir %u set %d: %u new bits, the loop has %u", base_docs, n_tail, dir_log2, set_kind, counted, want_new);
    if (n & 63) CHECK((words[n_words - 1] >> (n & 63)) == 0, "base %u tail %u: bits beyond n_docs", base_docs, n_tail);
    ++cases;
    return 0;
}

int main() {
    std::mt19937_64 rng(20240607);
    for (uint32_t dir_cap : {1u, 2u, 3u, 4u, 2048u, 4096u})  // (tid_dir 0 is a directory of one entry)
        for (uint32_t n_runs : {1u, 2u, 3u, 7u, 40u})
            if (walk_case(rng, n_runs, dir_cap)) return 1;
    if (walk_case(rng, 3000, 2048)) return 1;  // (a stride above 1 at the default directory: stage two of tid_find in front of the walk)
    if (walk_case(rng, 600, 4)) return 1;
    for (uint32_t base_docs : {0u, 1u, 59u, 64u, 70u, 300u})
        for (uint32_t n_tail : {0u, 1u, 58u, 59u, 200u})
            for (uint32_t dir_log2 : {0u, 2u, 11u})
                for (int set_kind = 0; set_kind < 5; ++set_kind)
                    if (word_case(rng, base_docs, n_tail, dir_log2, set_kind)) return 1;
    std::printf("%ld cases, %d failures\n", cases, failures);
    if (failures) return 1;
    std::printf("fuzz done\n");
    return 0;
}
