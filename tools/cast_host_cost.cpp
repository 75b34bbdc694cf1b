// cast_host_cost.cpp -- the host side of tools/cast_cost.py: the Document step with the library's host functions (vbm25_intern one lexeme
// a call, std::sort by key and a saturating merge per document), on T threads, timed in C++ so that no ctypes call overhead is charged
// to it; and the build baseline: that cast + a host vocabulary (sort and unique of all keys, ranks by bisection) +
// vbm25_segment_build_device_unsorted.  Built by the tool against csrc/libvbm25.so.
//
//   cast_host_cost FILE THREADS WARMUP REPS BUILD_REPS
// FILE: u64 n_docs, n_lex, n_bytes | 32 seed bytes | doc_lex u32 (n_docs + 1) | lex_off u64 (n_lex + 1) | lex_count u32 (n_lex) |
//       payload u16 (3 n_docs) | the lexemes' bytes.
// Prints one JSON line: the cast's median / min / max ms, the checksum of (start, key, tf, length) that the tool compares with the
// device's output, and (BUILD_REPS > 0) the build's times, its number of terms and postings.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../include/vbm25.h"

#define CHECK(expr)                                                             \
    do {                                                                        \
        if ((expr) != 0) {                                                      \
            std::fprintf(stderr, "%s failed: %s\n", #expr, vbm25_last_error()); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "short file\n");
        std::exit(2);
    }
    return v;
}

using Key = std::array<uint8_t, 16>;
struct Corpus {
    uint64_t n_docs, n_lex, n_bytes;
    std::vector<uint8_t> seed, bytes;
    std::vector<uint32_t> doc_lex, lex_count;
    std::vector<uint64_t> lex_off;
    std::vector<uint16_t> payload;
};
struct Cast {
    std::vector<uint64_t> start;
    std::vector<Key> key;
    std::vector<uint32_t> tf, length;
};

static void host_cast(const Corpus &c, int threads, Cast &out) {
    out.start.assign(c.n_docs + 1, 0);
    out.length.assign(c.n_docs, 0);
    std::vector<std::vector<Key>> tkey(threads);
    std::vector<std::vector<uint32_t>> ttf(threads);
    std::vector<uint64_t> first(threads + 1);
    for (int t = 0; t <= threads; ++t) first[t] = c.n_docs * uint64_t(t) / threads;
    auto work = [&](int t) {
        std::vector<std::pair<Key, uint32_t>> el;
        for (uint64_t d = first[t]; d < first[t + 1]; ++d) {
            el.clear();
            for (uint32_t i = c.doc_lex[d]; i < c.doc_lex[d + 1]; ++i) {
                Key k;
                CHECK(vbm25_intern(c.seed.data(), c.bytes.data() + c.lex_off[i], size_t(c.lex_off[i + 1] - c.lex_off[i]), k.data()));
                el.push_back({k, c.lex_count[i]});
            }
            std::sort(el.begin(), el.end(), [](const auto &a, const auto &b) { return std::memcmp(a.first.data(), b.first.data(), 16) < 0; });
            uint64_t len = 0, kept = 0;
            for (size_t i = 0; i < el.size();) {
                size_t j = i;
                uint64_t sum = 0;
                while (j < el.size() && el[j].first == el[i].first) sum += el[j++].second;
                const uint32_t v = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(sum);
                tkey[t].push_back(el[i].first);
                ttf[t].push_back(v);
                len += v;
                ++kept;
                i = j;
            }
            out.start[d + 1] = kept;
            out.length[d] = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(len);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool) th.join();
    for (uint64_t d = 0; d < c.n_docs; ++d) out.start[d + 1] += out.start[d];
    out.key.resize(out.start[c.n_docs]);
    out.tf.resize(out.start[c.n_docs]);
    auto gather = [&](int t) {
        const uint64_t at = out.start[first[t]];
        if (!tkey[t].empty()) {
            std::memcpy(out.key.data() + at, tkey[t].data(), 16 * tkey[t].size());
            std::memcpy(out.tf.data() + at, ttf[t].data(), 4 * ttf[t].size());
        }
    };
    pool.clear();
    for (int t = 1; t < threads; ++t) pool.emplace_back(gather, t);
    gather(0);
    for (auto &th : pool) th.join();
}

// sum of every array's values weighted by position, in wrapping 64-bit arithmetic (tools/cast_cost.py computes the same with numpy)
static uint64_t checksum(const Cast &c) {
    uint64_t h = 0;
    for (size_t i = 0; i < c.start.size(); ++i) h += c.start[i] * (i + 1);
    for (size_t e = 0; e < c.tf.size(); ++e) {
        uint64_t x, y;
        std::memcpy(&x, c.key[e].data(), 8);
        std::memcpy(&y, c.key[e].data() + 8, 8);
        h += (x ^ (y * 3)) * (2 * e + 1) + uint64_t(c.tf[e]) * (e + 5);
    }
    for (size_t d = 0; d < c.length.size(); ++d) h += uint64_t(c.length[d]) * (d + 7);
    return h;
}

static void host_build(const Corpus &c, const Cast &k, int threads, uint32_t *n_terms_out) {
    std::vector<Key> vocab(k.key);
    std::sort(vocab.begin(), vocab.end(), [](const Key &a, const Key &b) { return std::memcmp(a.data(), b.data(), 16) < 0; });
    vocab.erase(std::unique(vocab.begin(), vocab.end()), vocab.end());
    const uint64_t n = k.tf.size();
    std::vector<uint32_t> term(n), doc(n);
    auto work = [&](int t) {
        for (uint64_t d = c.n_docs * uint64_t(t) / threads; d < c.n_docs * uint64_t(t + 1) / threads; ++d)
            for (uint64_t e = k.start[d]; e < k.start[d + 1]; ++e) {
                doc[e] = uint32_t(d);
                term[e] = uint32_t(std::lower_bound(vocab.begin(), vocab.end(), k.key[e],
                                                    [](const Key &a, const Key &b) { return std::memcmp(a.data(), b.data(), 16) < 0; }) - vocab.begin());
            }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool) th.join();
    vbm25_segment *seg = nullptr;
    CHECK(vbm25_segment_build_device_unsorted(0, 1.2, 0.75, uint32_t(c.n_docs), k.length.data(), c.payload.data(), uint32_t(vocab.size()),
                                              vocab.empty() ? nullptr : vocab[0].data(), n, term.data(), doc.data(), k.tf.data(), &seg));
    vbm25_segment_free(seg);
    *n_terms_out = uint32_t(vocab.size());
}

static void stats(std::vector<double> v, const char *name) {
    std::sort(v.begin(), v.end());
    const double med = v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
    std::printf("\"%s\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}", name, med, v.front(), v.back());
}

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const int threads = std::atoi(argv[2]), warmup = std::atoi(argv[3]), reps = std::atoi(argv[4]), build_reps = std::atoi(argv[5]);
    Corpus c;
    const auto head = rd<uint64_t>(f, 3);
    c.n_docs = head[0], c.n_lex = head[1], c.n_bytes = head[2];
    c.seed = rd<uint8_t>(f, 32);
    c.doc_lex = rd<uint32_t>(f, c.n_docs + 1);
    c.lex_off = rd<uint64_t>(f, c.n_lex + 1);
    c.lex_count = rd<uint32_t>(f, c.n_lex);
    c.payload = rd<uint16_t>(f, 3 * c.n_docs);
    c.bytes = rd<uint8_t>(f, c.n_bytes);
    std::fclose(f);
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    Cast k;
    std::vector<double> t_cast, t_build;
    for (int r = 0; r < warmup + reps; ++r) {
        const auto t0 = clk::now();
        host_cast(c, threads, k);
        if (r >= warmup) t_cast.push_back(ms(t0, clk::now()));
    }
    uint32_t n_terms = 0;
    for (int r = 0; r < (build_reps ? 1 + build_reps : 0); ++r) {  // (one untimed run first)
        const auto t0 = clk::now();
        host_cast(c, threads, k);
        host_build(c, k, threads, &n_terms);
        if (r >= 1) t_build.push_back(ms(t0, clk::now()));
    }
    std::printf("{\"threads\": %d, \"reps\": %d, \"n_elements\": %llu, \"checksum\": \"%016llx\", ", threads, reps, (unsigned long long)k.tf.size(),
                (unsigned long long)checksum(k));
    stats(t_cast, "cast_ms");
    if (build_reps) {
        std::printf(", \"build_reps\": %d, \"n_terms\": %u, ", build_reps, n_terms);
        stats(t_build, "cast_and_build_ms");
    }
    std::printf("}\n");
    return 0;
}
