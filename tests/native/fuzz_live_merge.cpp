// fuzz_live_merge.cpp -- the rank functions of vbm25_reranker_sync's merge (csrc/tid_lane.h: live_rank_old, live_rank_delta) and the
// LDS sort's word and network (live_sort_word, live_sort_step) under AddressSanitizer + UBSan on the CPU, driven as live_merge_kernel
// and live_sort_kernel of live.hip drive them.  A stand-alone program (tests/test_live_rerank_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_live_merge.cpp -o fuzz_live_merge && ./fuzz_live_merge
// Old sets of 0 .. 5000 (key, doc) entries sorted by key with duplicates, doc ascending among equals; deltas of 0 .. 300 keys below,
// between, equal to and above the old keys, their docs above every old one; the old set's directory at every size 0 .. 4 entries, 2048
// and 4096.  Every array is a heap block of exactly its size, so an index beyond one is a heap overflow here.  One "lane" per entry
// writes its entry at its rank; the result must be std::merge of the two sequences on (key, doc) -- with every position written
// exactly once -- and the directory sampled again for dir_shape(new n) must hold dir_source's keys.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/tid_lane.h"

using namespace vbm25::tid;
using Entry = std::pair<uint64_t, uint32_t>;  // (key, doc)

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

// live_sort_kernel's steps on the host: the words of the delta's rows padded to a power of two, the network, the rows read back
static std::vector<Entry> lds_sort(const std::vector<uint64_t> &row_keys, uint32_t first_doc) {
    const uint32_t m = uint32_t(row_keys.size());
    uint32_t padded = 1;
    while (padded < m) padded <<= 1;
    std::vector<uint64_t> w(padded, LIVE_SORT_PAD);
    w.shrink_to_fit();
    for (uint32_t j = 0; j < m; ++j) w[j] = live_sort_word(row_keys[j], j);
    for (uint32_t k = 2; k <= padded; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1)
            for (uint32_t t = 0; t < (padded >> 1); ++t) live_sort_step(w.data(), t, k, j);
    std::vector<Entry> out;
    for (uint32_t j = 0; j < m; ++j) out.emplace_back(live_sort_key(w[j]), first_doc + live_sort_row(w[j]));
    return out;
}

static int one_case(const std::vector<uint64_t> &old_keys_in, const std::vector<uint64_t> &delta_rows, uint32_t cap, uint32_t new_cap, uint64_t &lanes) {
    // the old directory: keys sorted, docs a permutation that ascends among equal keys (a stable sort of (key, doc))
    const uint32_t n_old = uint32_t(old_keys_in.size()), m = uint32_t(delta_rows.size());
    std::vector<Entry> old_e;
    for (uint32_t d = 0; d < n_old; ++d) old_e.emplace_back(old_keys_in[d], d);
    std::stable_sort(old_e.begin(), old_e.end(), [](const Entry &a, const Entry &b) { return a.first < b.first; });
    std::vector<uint64_t> keys(n_old), dir;
    std::vector<uint32_t> docs(n_old);
    for (uint32_t i = 0; i < n_old; ++i) keys[i] = old_e[i].first, docs[i] = old_e[i].second;
    const DirShape shape = shape_for(n_old, cap);
    for (uint32_t j = 0; j < shape.n_dir; ++j) dir.push_back(keys.at(dir_source(j, shape.stride)));
    keys.shrink_to_fit(), docs.shrink_to_fit(), dir.shrink_to_fit();
    // the delta, sorted as the kernel sorts it, against a stable sort
    const std::vector<Entry> delta = lds_sort(delta_rows, n_old);
    std::vector<Entry> want_delta;
    for (uint32_t j = 0; j < m; ++j) want_delta.emplace_back(delta_rows[j], n_old + j);
    std::stable_sort(want_delta.begin(), want_delta.end(), [](const Entry &a, const Entry &b) { return a.first < b.first; });
    CHECK(delta == want_delta, "n_old=%u m=%u: the LDS sort is not the stable sort", n_old, m);
    std::vector<uint64_t> dkeys(m);
    for (uint32_t j = 0; j < m; ++j) dkeys[j] = delta[j].first;
    dkeys.shrink_to_fit();
    // the merge by rank: one lane an entry
    std::vector<Entry> out(size_t(n_old) + m);
    std::vector<uint8_t> written(size_t(n_old) + m, 0);
    out.shrink_to_fit(), written.shrink_to_fit();
    for (uint32_t j = 0; j < m; ++j) {
        const uint64_t at = j + live_rank_delta(dkeys[j], dir.empty() ? nullptr : dir.data(), shape.n_dir, keys.empty() ? nullptr : keys.data(), n_old, shape.stride);
        CHECK(at < out.size() && !written[at], "n_old=%u m=%u cap=%u: delta entry %u goes to %llu", n_old, m, cap, j, (unsigned long long)at);
        out[at] = delta[j], written[at] = 1, ++lanes;
    }
    for (uint32_t i = 0; i < n_old; ++i) {
        const uint64_t at = i + live_rank_old(keys[i], dkeys.empty() ? nullptr : dkeys.data(), m);
        CHECK(at < out.size() && !written[at], "n_old=%u m=%u cap=%u: old entry %u goes to %llu", n_old, m, cap, i, (unsigned long long)at);
        out[at] = Entry(keys[i], docs[i]), written[at] = 1, ++lanes;
    }
    std::vector<Entry> want(size_t(n_old) + m);
    std::merge(old_e.begin(), old_e.end(), delta.begin(), delta.end(), want.begin());  // (on (key, doc): every old doc is below every new one)
    CHECK(out == want, "n_old=%u m=%u cap=%u stride=%u: the merge by rank is not std::merge", n_old, m, cap, shape.stride);
    CHECK(std::is_sorted(want.begin(), want.end()), "n_old=%u m=%u: the model itself is not in (key, doc) order", n_old, m);
    // the directory sampled again
    const DirShape ns = shape_for(out.size(), new_cap);
    CHECK(ns.n_dir <= new_cap && (out.empty() || (uint64_t(ns.n_dir - 1) * ns.stride < out.size() && uint64_t(ns.n_dir) * ns.stride >= out.size())),
          "n=%zu cap=%u: shape %u x %u", out.size(), new_cap, ns.n_dir, ns.stride);
    for (uint32_t j = 0; j < ns.n_dir; ++j) CHECK(out.at(dir_source(j, ns.stride)).first == want[size_t(j) * ns.stride].first, "the new directory's entry %u", j);
    return 0;
}

int main() {
    std::mt19937_64 rng(20261021);
    const uint32_t caps[] = {0, 1, 2, 3, 4, 2048, 4096};
    const size_t sizes[] = {0, 1, 2, 3, 4, 5, 8, 63, 64, 65, 1000, 2047, 2048, 2049, 4096, 4097, 5000};
    const size_t deltas[] = {0, 1, 2, 3, 63, 64, 65, 300};
    uint64_t lanes = 0, cases = 0;
    for (uint32_t cap : caps)
        for (size_t n : sizes) {
            if (cap == 0 && n) continue;
            for (size_t m : deltas)
                for (int style = 0; style < 4; ++style) {
                    std::vector<uint64_t> keys, rows;
                    // the old keys -- 0: distinct spread keys; 1: few values, long runs of duplicates; 2: dense neighbours, every third
                    // doubled; 3: the extremes 0 and 2^48 - 1 among random keys
                    for (size_t i = 0; i < n; ++i) {
                        switch (style) {
                            case 0: keys.push_back(rng() & KEY_MAX); break;
                            case 1: keys.push_back(((rng() % (n / 7 + 1)) * 1000003ull + 5) & KEY_MAX); break;
                            case 2: keys.push_back(1000 + 2 * (i - (i % 3 == 2))); break;
                            default: keys.push_back(i % 5 == 0 ? 0 : i % 5 == 1 ? KEY_MAX : rng() & KEY_MAX); break;
                        }
                    }
                    // the delta's rows, unsorted: equal to an old key, one below, one above, between two, the extremes, and repeats of itself
                    for (size_t j = 0; j < m; ++j) {
                        const uint64_t base = n ? keys[rng() % n] : rng() & KEY_MAX;
                        switch ((j + style) % 7) {
                            case 0: rows.push_back(base); break;
                            case 1: rows.push_back(base ? base - 1 : 0); break;
                            case 2: rows.push_back(base < KEY_MAX ? base + 1 : KEY_MAX); break;
                            case 3: rows.push_back(rng() & KEY_MAX); break;
                            case 4: rows.push_back(j % 2 ? 0 : KEY_MAX); break;
                            case 5: rows.push_back(rows.empty() ? base : rows[rng() % rows.size()]); break;
                            default: rows.push_back(style == 2 ? 999 + rng() % (2 * n + 3) : base); break;
                        }
                    }
                    if (one_case(keys, rows, cap, caps[(cases + 1) % 7] ? caps[(cases + 1) % 7] : 1, lanes)) return 1;
                    ++cases;
                }
        }
    // the LDS sort at its capacity, every row one key and every row another
    for (int same = 0; same < 2; ++same) {
        std::vector<uint64_t> rows(1u << LIVE_SORT_LOG2);
        for (size_t j = 0; j < rows.size(); ++j) rows[j] = same ? KEY_MAX : rng() % 97;
        if (one_case({5, 5, KEY_MAX, 0}, rows, 2, 4096, lanes)) return 1;
        ++cases;
    }
    std::printf("%llu cases, %llu lanes\n", (unsigned long long)cases, (unsigned long long)lanes);
    if (failures) {
        std::printf("%d FAILURES\n", failures);
        return 1;
    }
    std::printf("fuzz done\n");
    return 0;
}
