// resolve_host_cost.cpp -- the host side of tools/resolve_cost.py: the Query step with the library's host functions (vbm25_intern one
// lexeme a call, ONE vbm25_lookup_terms call over the batch's keys, std::sort + unique + drop per query), timed in C++ so that no
// ctypes call overhead is charged to it.  Built by the tool against csrc/libvbm25.so.
//
//   resolve_host_cost FILE
// FILE: u32 n_terms | 16 n_terms key bytes (ascending) | 32 seed bytes | u32 n_cases | per case: u32 nq, u32 n_lex, u64 n_bytes,
//       q_lex u32 (nq + 1), lex_off u64 (n_lex + 1), the lexemes' bytes, the lexemes' keys (16 n_lex).
// The index is built here from the keys (one posting a term: only the vocabulary matters).  Prints one JSON line per case with the
// medians of REPS timed runs and an FNV-1a checksum of (q_off, term_ids) that the tool compares with the device's output.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/vbm25.h"

static const int WARMUP = 3, REPS = 30;

#define CHECK(expr)                                                                    \
    do {                                                                               \
        if ((expr) != 0) {                                                             \
            std::fprintf(stderr, "%s failed: %s\n", #expr, vbm25_last_error());        \
            return 1;                                                                  \
        }                                                                              \
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

static uint64_t fnv(uint64_t h, const uint32_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        h ^= p[i];
        h *= 1099511628211ull;
    }
    return h;
}

struct Stat {
    double median, lo, hi;
};
static Stat stat(std::vector<double> t) {
    std::sort(t.begin(), t.end());
    return {t[t.size() / 2], t.front(), t.back()};
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t n_terms = rd<uint32_t>(f, 1)[0];
    const std::vector<uint8_t> term_key = rd<uint8_t>(f, 16ull * n_terms), seed = rd<uint8_t>(f, 32);
    const uint32_t n_docs = 1000;
    std::vector<uint32_t> doc_len(n_docs, 0), post_doc(n_terms), post_tf(n_terms, 1);
    std::vector<uint64_t> term_start(size_t(n_terms) + 1);
    std::vector<uint16_t> payload(3 * n_docs, 0);
    for (uint32_t t = 0; t < n_terms; ++t) {
        post_doc[t] = t % n_docs;
        ++doc_len[t % n_docs];
        term_start[t + 1] = t + 1;
    }
    vbm25_device_segment *ds = nullptr;
    vbm25_index *ix = nullptr;
    CHECK(vbm25_device_segment_build(0, 1.2, 0.75, n_docs, doc_len.data(), payload.data(), n_terms, term_key.data(), term_start.data(), post_doc.data(),
                                     post_tf.data(), &ds));
    CHECK(vbm25_index_create_from_device(ds, &ix));
    const uint32_t n_cases = rd<uint32_t>(f, 1)[0];
    for (uint32_t c = 0; c < n_cases; ++c) {
        const uint32_t nq = rd<uint32_t>(f, 1)[0], n_lex = rd<uint32_t>(f, 1)[0];
        const uint64_t n_bytes = rd<uint64_t>(f, 1)[0];
        const std::vector<uint32_t> q_lex = rd<uint32_t>(f, size_t(nq) + 1);
        const std::vector<uint64_t> lex_off = rd<uint64_t>(f, size_t(n_lex) + 1);
        const std::vector<uint8_t> bytes = rd<uint8_t>(f, n_bytes), keys = rd<uint8_t>(f, 16ull * n_lex);
        std::vector<uint8_t> my_keys(16ull * n_lex);
        std::vector<uint32_t> ids(n_lex), term_ids(n_lex), q_off(size_t(nq) + 1);
        auto pack = [&](const uint8_t *k) {  // one lookup call over the batch, then sort, dedup and drop per query
            if (vbm25_lookup_terms(ix, k, n_lex, ids.data())) std::exit(3);
            uint32_t o = 0;
            q_off[0] = 0;
            for (uint32_t q = 0; q < nq; ++q) {
                uint32_t *b = ids.data() + q_lex[q], *e = ids.data() + q_lex[q + 1];
                std::sort(b, e);
                e = std::unique(b, e);
                for (; b != e && *b != UINT32_MAX; ++b) term_ids[o++] = *b;
                q_off[q + 1] = o;
            }
        };
        auto now = [] { return std::chrono::steady_clock::now(); };
        std::vector<double> t_keys, t_lex, t_intern;
        for (int r = 0; r < WARMUP + REPS; ++r) {
            auto t0 = now();
            pack(keys.data());
            auto t1 = now();
            for (uint32_t i = 0; i < n_lex; ++i)
                if (vbm25_intern(seed.data(), bytes.data() + lex_off[i], size_t(lex_off[i + 1] - lex_off[i]), my_keys.data() + 16ull * i)) std::exit(3);
            auto t2 = now();
            pack(my_keys.data());
            auto t3 = now();
            if (r < WARMUP) continue;
            t_keys.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            t_intern.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
            t_lex.push_back(std::chrono::duration<double, std::milli>(t3 - t1).count());
        }
        if (my_keys != keys) {
            std::fprintf(stderr, "case %u: vbm25_intern's keys differ from the file's\n", c);
            return 4;
        }
        const uint64_t sum = fnv(fnv(1469598103934665603ull, q_off.data(), q_off.size()), term_ids.data(), q_off[nq]);
        const Stat k = stat(t_keys), l = stat(t_lex), i = stat(t_intern);
        std::printf("{\"case\": %u, \"n_ids\": %u, \"checksum\": \"%016llx\", \"keys_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, "
                    "\"lexemes_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, \"intern_only_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}}\n",
                    c, q_off[nq], (unsigned long long)sum, k.median, k.lo, k.hi, l.median, l.lo, l.hi, i.median, i.lo, i.hi);
    }
    vbm25_index_destroy(ix);
    vbm25_device_segment_free(ds);
    std::fclose(f);
    return 0;
}
