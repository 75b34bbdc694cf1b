// fuzz_rerank.cpp -- csrc/rerank_lane.h under AddressSanitizer + UBSan on the CPU: the functions the top-k selection of rerank.hip is
// made of, driven as its workgroup drives them.  A stand-alone program (tests/test_rerank_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_rerank.cpp -o fuzz_rerank && ./fuzz_rerank
// A model workgroup of four waves offers 64 entries a wave a round, the waves in shuffled order between the barriers, to a buffer
// allocated to exactly its size (a slot beyond it is a heap overflow here); a full buffer is sorted with the bitonic schedule and cut
// to k; candidates are split into parts whose lists a second buffer merges.  The result must equal std::stable_sort (score
// descending) cut at k, entry for entry.  Also: the key order is the doubles' order, and `better` is a strict weak (in fact total)
// order on samples with equal scores and the extreme positions.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/rerank_lane.h"

using namespace vbm25::rrk;

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

static uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

// the selection buffer of one workgroup, as rerank.hip keeps it in LDS
struct Buffer {
    std::vector<uint64_t> key;
    std::vector<uint32_t> pos;
    uint32_t buf, k, cnt = 0;
    Entry thr = WORST;
    uint32_t cuts = 0;
    Buffer(uint32_t buf_, uint32_t k_) : key(buf_), pos(buf_), buf(buf_), k(k_) {}

    void sort(uint32_t n) {  // sel_sort: every exchange of a step is independent of the others, so their order is shuffled too
        for (uint32_t size = 2; size <= n; size <<= 1)
            for (uint32_t stride = size >> 1; stride; stride >>= 1)
                for (uint32_t t0 = 0; t0 < n / 2; ++t0) {
                    const uint32_t t = (size & 4u) ? n / 2 - 1 - t0 : t0;
                    uint32_t i, j;
                    bitonic_pair(t, stride, i, j);
                    exchange(key.at(i), pos.at(i), key.at(j), pos.at(j), bitonic_best_first(i, size));
                }
    }

    // sel_offer: 256 lanes, lane l of wave w is entry w * 64 + l
    void offer(const std::vector<Entry> &e, const std::vector<bool> &have, std::mt19937_64 &rng) {
        bool pending[ROUND];
        for (uint32_t i = 0; i < ROUND; ++i) pending[i] = have[i] && better(e[i], thr);
        for (;;) {
            uint32_t order[4] = {0, 1, 2, 3};
            std::shuffle(order, order + 4, rng);
            for (uint32_t w : order) {
                uint64_t ballot = 0;
                for (uint32_t l = 0; l < 64; ++l)
                    if (pending[w * 64 + l]) ballot |= 1ull << l;
                if (!ballot) continue;
                const uint32_t base = cnt;  // (the atomic add)
                cnt += uint32_t(__builtin_popcountll(ballot));
                for (uint32_t l = 0; l < 64; ++l) {
                    if (!pending[w * 64 + l]) continue;
                    const uint32_t slot = offer_slot(base, rank_in(ballot, l));
                    if (slot < buf) {
                        key[slot] = e[w * 64 + l].key;  // (operator[] on an exactly sized vector: AddressSanitizer sees an overflow)
                        pos[slot] = e[w * 64 + l].pos;
                        pending[w * 64 + l] = false;
                    }
                }
            }
            if (cnt < buf) {
                for (bool p : pending)
                    if (p) std::printf("FAIL an entry is pending under a buffer that is not full\n"), ++failures;
                return;
            }
            sort(buf);
            ++cuts;
            cnt = k;
            thr = Entry{key[k - 1], pos[k - 1]};
            for (uint32_t i = 0; i < ROUND; ++i) pending[i] = pending[i] && better(e[i], thr);
        }
    }

    // sel_finish
    std::vector<Entry> finish() {
        const uint32_t span = sort_entries(cnt);
        for (uint32_t i = cnt; i < span; ++i) key.at(i) = WORST_KEY, pos.at(i) = WORST_POS;
        sort(span);
        std::vector<Entry> out;
        for (uint32_t i = 0; i < std::min(cnt, k); ++i) out.push_back(Entry{key[i], pos[i]});
        return out;
    }
};

static std::vector<Entry> select_stream(const std::vector<Entry> &in, uint32_t buf, uint32_t k, std::mt19937_64 &rng, uint32_t *cuts) {
    Buffer b(buf, k);
    for (size_t c0 = 0; c0 < in.size(); c0 += ROUND) {
        std::vector<Entry> e(ROUND, WORST);
        std::vector<bool> have(ROUND, false);
        for (uint32_t i = 0; i < ROUND && c0 + i < in.size(); ++i) e[i] = in[c0 + i], have[i] = true;
        b.offer(e, have, rng);
    }
    *cuts += b.cuts;
    return b.finish();
}

static int order_checks() {
    const double values[] = {0.0, 5e-324, 1e-300, 0.5, 1.0, 1.0000000000000002, 3.25, 1e300, INFINITY, -5e-324, -0.5, -1.0, -1e300, -INFINITY};
    const size_t nv = sizeof values / sizeof *values;
    for (size_t a = 0; a < nv; ++a) {
        CHECK(key_score(score_key(bits_of(values[a]))) == bits_of(values[a]), "key round trip of %a", values[a]);
        for (size_t b = 0; b < nv; ++b)
            CHECK((values[a] < values[b]) == (score_key(bits_of(values[a])) < score_key(bits_of(values[b]))), "key order of %a and %a", values[a], values[b]);
    }
    const uint32_t positions[] = {0u, 1u, 63u, 64u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    std::vector<Entry> s;
    for (double v : {0.0, 0.0, 1.0, 1.0, 2.5, 1e-300})
        for (uint32_t p : positions) s.push_back(Entry{score_key(bits_of(v)), p});
    s.push_back(WORST);
    for (const Entry &a : s) {
        CHECK(!better(a, a), "better is not irreflexive");
        for (const Entry &b : s) {
            const bool same = a.key == b.key && a.pos == b.pos;
            CHECK(!(better(a, b) && better(b, a)), "better is not asymmetric");
            CHECK(same || better(a, b) || better(b, a), "two different entries compare equal");
            for (const Entry &c : s) {
                CHECK(!(better(a, b) && better(b, c)) || better(a, c), "better is not transitive");
                // incomparability (here: identity) is transitive
                CHECK(!(!better(a, b) && !better(b, a) && !better(b, c) && !better(c, b)) || (!better(a, c) && !better(c, a)), "equivalence is not transitive");
            }
        }
        CHECK((a.key == WORST_KEY && a.pos == WORST_POS) || better(a, WORST), "WORST does not lose");
    }
    // the sizes
    for (uint32_t k = 1; k <= MAX_K; ++k)
        for (uint32_t m : {0u, 2u, 3u, 8u, 100u}) {
            const uint32_t b = buffer_entries(k, m);
            CHECK((b & (b - 1)) == 0 && b >= 2 * k && b >= ROUND && b <= MAX_BUFFER, "buffer_entries(%u, %u) = %u", k, m, b);
        }
    for (uint32_t n = 0; n < 5000; ++n) {
        const uint32_t sp = sort_entries(n);
        CHECK((sp & (sp - 1)) == 0 && sp >= 2 && sp >= n && (sp == 2 || sp / 2 < n), "sort_entries(%u) = %u", n, sp);
    }
    for (uint32_t l = 0; l < 64; ++l) {
        CHECK(rank_in(~0ull, l) == l && rank_in(0x5555555555555555ull, l) == (l + 1) / 2, "rank_in at lane %u", l);
    }
    return 0;
}

static int one_case(uint32_t seed, uint32_t *cuts, uint32_t *merged) {
    std::mt19937_64 rng(seed);
    static const uint32_t ks[] = {1, 2, 3, 10, 31, 32, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 1000, 1023, 1024};
    const uint32_t k = seed < 2 * (sizeof ks / sizeof *ks) ? ks[seed / 2] : 1 + uint32_t(rng() % MAX_K);
    // buffers of 2k (the power of two over it: the network's size), with and without the floor of one round
    const uint32_t buf = seed % 2 ? buffer_entries(k, 2) : pow2_ceil(2 * k);
    const uint32_t sizes[] = {0, 1, 63, 64, 65, k - 1, k, k + 1, 2 * k, 2 * k + 1, 3000, 5000, 4 * k + 100, 2500 + uint32_t(rng() % 3500), uint32_t(rng() % 6000)};
    const uint32_t n = sizes[rng() % (sizeof sizes / sizeof *sizes)];
    // heavy ties: a handful of scores, zero the most frequent; some cases ascending (every entry beats the threshold), some with
    // negative scores
    const uint32_t distinct = 1 + uint32_t(rng() % 6);
    const int shape = int(rng() % 5);
    std::vector<double> score(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (shape == 0) score[i] = double(i / 7);                                    // ascending runs of ties
        else if (shape == 1) score[i] = (rng() % 3) ? 0.0 : double(rng() % distinct) * 0.25;
        else if (shape == 2) score[i] = double(rng() % distinct) - 2.0;              // negative ones among them (never -0.0)
        else if (shape == 3) score[i] = double(rng() % 1000) / 8.0;
        else score[i] = double(i) * 0.5 + double(rng() % 3);                         // rising: most entries beat the threshold
    }
    std::vector<Entry> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = Entry{score_key(bits_of(score[i])), i};
    // the reference
    std::vector<uint32_t> want(n);
    for (uint32_t i = 0; i < n; ++i) want[i] = i;
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return score[a] > score[b]; });
    want.resize(std::min(n, k));
    // one part, or parts of 64 .. 1024 candidates merged as rerank_merge_kernel merges them
    const uint32_t part_choices[] = {64, 128, 192, 1000 / 64 * 64, 1024, 1u << 20};
    const uint32_t part = part_choices[rng() % 6];
    std::vector<Entry> got;
    if (n <= part) {
        got = select_stream(in, buf, k, rng, cuts);
    } else {
        ++*merged;
        std::vector<std::vector<Entry>> lists;
        for (uint32_t lo = 0; lo < n; lo += part)
            lists.push_back(select_stream(std::vector<Entry>(in.begin() + lo, in.begin() + std::min(n, lo + part)), buf, k, rng, cuts));
        std::shuffle(lists.begin(), lists.end(), rng);  // (the order the lists are read in must not matter)
        Buffer b(buf, k);
        for (const auto &l : lists)
            for (size_t j0 = 0; j0 < l.size(); j0 += ROUND) {
                std::vector<Entry> e(ROUND, WORST);
                std::vector<bool> have(ROUND, false);
                for (uint32_t i = 0; i < ROUND && j0 + i < l.size(); ++i) e[i] = l[j0 + i], have[i] = true;
                b.offer(e, have, rng);
            }
        *cuts += b.cuts;
        got = b.finish();
    }
    CHECK(got.size() == want.size(), "case %u (k %u, buf %u, n %u, part %u): %zu entries, want %zu", seed, k, buf, n, part, got.size(), want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); ++i)
        CHECK(got[i].pos == want[i] && key_score(got[i].key) == bits_of(score[want[i]]),
              "case %u (k %u, buf %u, n %u, part %u): entry %zu is pos %u, want %u", seed, k, buf, n, part, i, got[i].pos, want[i]);
    return 0;
}

int main() {
    if (order_checks()) return 1;
    uint32_t cuts = 0, merged = 0;
    for (uint32_t seed = 0; seed < 200; ++seed)
        if (one_case(seed, &cuts, &merged)) return 1;
    std::printf("200 cases, %u cuts, %u merged from parts\n", cuts, merged);
    if (cuts < 200 || merged < 20) std::printf("FAIL the cases do not exercise the cut or the merge\n"), ++failures;
    if (failures) return 1;
    std::printf("fuzz done\n");
    return 0;
}
