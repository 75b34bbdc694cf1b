// fuzz_evaluate.cpp -- csrc/evaluate_lane.h on the CPU under AddressSanitizer + UBSan: bisect_run (the bisection a lane of
// eval_score_kernel runs for every query term) against std::lower_bound, and pair_score (score_step per term, the text the kernel
// loops over) against a plain merge walk written here.  Stand-alone, built and run by tests/test_evaluate_documents_host.py.  Every
// array is allocated exactly: a read past a run, past the query or past the idf table is a heap-buffer-overflow.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/evaluate_lane.h"

using namespace vbm25::evl;

static int failures = 0;
static long checked = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL: ");        \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            if (++failures > 20) std::exit(1); \
        }                                 \
    } while (0)

static std::mt19937_64 rng(20261019);

// n strictly ascending ids with gaps (so that probes fall between them), the first one >= 3
static std::vector<uint32_t> ascending(uint32_t n, uint32_t max_gap) {
    std::vector<uint32_t> v(n);
    uint32_t at = 3;
    for (uint32_t i = 0; i < n; ++i) {
        at += 1 + uint32_t(rng() % max_gap);
        v[i] = at;
    }
    return v;
}

static void check_probe(const std::vector<uint32_t> &run, uint32_t lo, uint32_t hi, uint32_t id) {
    bool found = true;
    const uint32_t p = bisect_run(run.data(), lo, hi, id, found);
    const uint32_t want = uint32_t(std::lower_bound(run.begin() + lo, run.begin() + hi, id) - run.begin());
    EXPECT(p == want, "bisect_run(%zu ids, [%u, %u), %u) = %u, lower_bound %u", run.size(), lo, hi, id, p, want);
    EXPECT(found == (want < hi && run[want] == id), "found flag for id %u in [%u, %u) of %zu ids", id, lo, hi, run.size());
    ++checked;
}

static void test_bisection() {
    std::vector<uint32_t> lengths{5000};
    for (uint32_t p = 1; p <= 4096; p <<= 1) {
        lengths.push_back(p - 1);
        lengths.push_back(p);
        lengths.push_back(p + 1);
    }
    for (uint32_t n : lengths) {
        const std::vector<uint32_t> run = ascending(n, 3);  // (exactly n entries: run.data() + n is past the allocation)
        // below, every member, every gap, above -- on the whole run
        check_probe(run, 0, n, 0);
        check_probe(run, 0, n, 0xFFFFFFFFu);
        for (uint32_t i = 0; i < n; ++i) {
            check_probe(run, 0, n, run[i]);
            check_probe(run, 0, n, run[i] - 1);
            check_probe(run, 0, n, run[i] + 1);
        }
        // sub-ranges, the empty ones among them: what a cursor that has moved leaves
        for (int rep = 0; rep < 200; ++rep) {
            const uint32_t lo = n ? uint32_t(rng() % (n + 1)) : 0, hi = lo + (n > lo ? uint32_t(rng() % (n - lo + 1)) : 0);
            const uint32_t id = n && (rng() & 1) ? run[rng() % n] : uint32_t(rng() % (run.empty() ? 10 : run.back() + 5));
            check_probe(run, lo, hi, id);
        }
    }
    // an empty run reads nothing whatever its bounds are: a NULL array
    bool found = true;
    EXPECT(bisect_run(nullptr, 0, 0, 7, found) == 0 && !found, "empty run at 0");
    EXPECT(bisect_run(nullptr, 9, 9, 7, found) == 9 && !found, "empty run at 9");
    checked += 2;
}

// evaluate_kernel's walk (index.hip), restated: a merge of the document's ids with the query's
static double merge_walk(const std::vector<uint32_t> &term, const std::vector<uint32_t> &tf, uint32_t lo, uint32_t hi, const std::vector<uint32_t> &q,
                         const std::vector<double> &idf, double k1p1, double s1) {
    const uint32_t n_terms = uint32_t(idf.size());
    uint32_t cur = lo;
    double result = 0.0;
    for (uint32_t qt : q) {
        if (qt >= n_terms) continue;
        while (cur < hi && term[cur] < qt) ++cur;
        if (!(cur < hi && term[cur] == qt)) continue;
        const double f = double(tf[cur]);
        const double tfv = (f * k1p1) / (f + s1);
        result += idf[qt] * tfv;
    }
    return result;
}

static void test_pair_score() {
    const uint32_t n_terms = 700;
    std::vector<double> idf(n_terms);
    for (double &v : idf) v = 0.01 + double(rng() % 100000) / 7919.0;
    for (uint32_t n_q = 0; n_q <= 300; ++n_q) {
        for (int rep = 0; rep < 6; ++rep) {
            // the query: n_q ascending ids out of 0 .. 999 -- those >= 700 are unknown to the index and skipped
            std::vector<uint32_t> pool(1000);
            for (uint32_t i = 0; i < 1000; ++i) pool[i] = i;
            std::shuffle(pool.begin(), pool.end(), rng);
            std::vector<uint32_t> q(pool.begin(), pool.begin() + n_q);
            std::sort(q.begin(), q.end());
            if (n_q && rep == 5) q.back() = 0xFFFFFFFFu;
            // the documents of two neighbours in one array: the pair's run is the middle one
            const uint32_t len[3] = {uint32_t(rng() % 4), rep == 0 ? 0u : uint32_t(rng() % (rep < 3 ? 8 : 600)), uint32_t(rng() % 4)};
            std::vector<uint32_t> term, tf;
            for (uint32_t len_d : len) {
                std::shuffle(pool.begin(), pool.end(), rng);
                std::vector<uint32_t> ids;
                for (uint32_t v : pool)
                    if (v < n_terms && ids.size() < len_d) ids.push_back(v);
                std::sort(ids.begin(), ids.end());
                for (uint32_t v : ids) {
                    term.push_back(v);
                    tf.push_back(rng() % 8 == 0 ? 0xFFFFFFFFu : 1 + uint32_t(rng() % 50));
                }
            }
            const uint32_t lo = len[0], hi = len[0] + len[1];
            const double k1p1 = rep & 1 ? 2.2 : 3.0, s1 = 0.3 + double(rng() % 1000) / 100.0;
            const double got = pair_score(term.data(), tf.data(), lo, hi, q.data(), n_q, n_terms, idf.data(), k1p1, s1);
            const double want = merge_walk(term, tf, lo, hi, q, idf, k1p1, s1);
            EXPECT(std::memcmp(&got, &want, 8) == 0, "pair_score %a, merge walk %a (query of %u, document of %u)", got, want, n_q, len[1]);
            ++checked;
        }
    }
}

int main() {
    test_bisection();
    test_pair_score();
    std::printf("%ld checks\n", checked);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("fuzz done\n");
    return 0;
}
