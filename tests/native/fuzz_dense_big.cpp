// fuzz_dense_big.cpp -- csrc/dense_list_lane.h under AddressSanitizer + UBSan on the CPU: the functions the survivor list of
// scan_dense_kernel<1024> is made of, driven as its workgroup drives them.  A stand-alone program (tests/test_dense_big_host.py builds
// and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_dense_big.cpp -o fuzz_dense_big && ./fuzz_dense_big
// Eight model waves append up to 64 entries each between two barriers, in shuffled order, to a buffer allocated to exactly CAP entries
// (a slot beyond it is a heap overflow here); behind a barrier with the cursor past k the list is cut: the bitonic schedule, where a run
// of LOCAL stages is carried out wave after wave -- each wave through the whole run before the next starts, which is only right if a
// wave's pairs stay inside its own eighth -- then the first k are kept and the k-th key becomes the threshold.  The result must equal
// std::partial_sort on "score descending, doc ascending"; an item that overflows must have written nothing past the buffer.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/dense_list_lane.h"

using namespace vbm25;
using rrk::Entry;

struct List {
    std::vector<uint64_t> key = std::vector<uint64_t>(dlist::CAP);
    std::vector<uint32_t> doc = std::vector<uint32_t>(dlist::CAP);
    uint32_t cur = 0, k, cuts = 0;
    uint64_t theta = 0;
    bool fail = false;

    void append(const std::vector<Entry> &e) {  // one wave: e.size() <= 64 lanes hold a re-scored document
        uint64_t ballot = 0;
        for (size_t l = 0; l < e.size(); ++l)
            if (dlist::keeps(e[l].key, theta)) ballot |= 1ull << l;
        if (!ballot) return;
        const uint32_t base = cur;  // (the atomic add)
        cur += uint32_t(__builtin_popcountll(ballot));
        for (size_t l = 0; l < e.size(); ++l) {
            if (!((ballot >> l) & 1ull)) continue;
            const uint32_t slot = rrk::offer_slot(base, rrk::rank_in(ballot, uint32_t(l)));
            if (dlist::fits(slot)) key[slot] = e[l].key, doc[slot] = e[l].pos;  // (operator[] on an exactly sized vector)
            else fail = true;
        }
    }
    void stage(uint32_t w, uint32_t n, uint32_t size, uint32_t stride) {
        for (uint32_t p = 0; p < dlist::wave_pairs(n); ++p) {
            uint32_t i, j;
            bool best_first;
            dlist::wave_pair(w, p, n, size, stride, i, j, best_first);
            rrk::exchange(key.at(i), doc.at(i), key.at(j), doc.at(j), best_first);
        }
    }
    void cut() {
        const uint32_t live = std::min(cur, dlist::CAP), n = dlist::sort_entries(live);
        for (uint32_t i = live; i < n; ++i) key.at(i) = dlist::PAD_KEY, doc.at(i) = dlist::PAD_DOC;
        std::vector<std::pair<uint32_t, uint32_t>> stages;
        for (uint32_t size = 2; size <= n; size <<= 1)
            for (uint32_t stride = size >> 1; stride; stride >>= 1) stages.push_back({size, stride});
        for (size_t s = 0; s < stages.size();) {
            size_t e = s + 1;
            if (dlist::stage_local(stages[s].second, n))
                while (e < stages.size() && dlist::stage_local(stages[e].second, n)) ++e;
            for (uint32_t w0 = 0; w0 < dlist::WAVES; ++w0)  // (a wide stage: a run of one, any wave order; between runs: the barrier)
                for (size_t x = s; x < e; ++x) stage((w0 * 5 + cuts) % dlist::WAVES, n, stages[x].first, stages[x].second);
            s = e;
        }
        ++cuts;
        cur = dlist::cut_count(live, k);
        if (live >= k) theta = std::max(theta, key.at(k - 1));
    }
};

static int one_case(uint32_t seed, uint32_t *cuts, uint32_t *given_up) {
    std::mt19937_64 rng(seed);
    static const uint32_t ks[] = {257, 512, 1000, 1024};
    const uint32_t k = seed < 8 ? ks[seed / 2] : 257 + uint32_t(rng() % 768);
    const uint32_t sizes[] = {0, k - 1, k, k + 1, 2 * k + 1, 5 * k};
    const uint32_t n = sizes[rng() % 6];
    const int shape = int(rng() % 3);  // few distinct scores (runs of ties) | random | rising (every entry beats the threshold)
    std::vector<Entry> in(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double s = shape == 0 ? 1.0 + double(rng() % 5) : shape == 1 ? 0.001 + double(rng() % 100000) / 7.0 : 1.0 + i * 0.5;
        std::memcpy(&in[i].key, &s, 8);
        in[i].pos = i;
    }
    if (shape != 2) std::shuffle(in.begin(), in.end(), rng);  // (the list must not care about the order of arrival; rising stays rising)
    List L;
    L.k = k;
    for (uint32_t at = 0; at < n && !L.fail;) {  // a window: every wave appends a few times, then the barrier
        const uint32_t rounds = seed % 3 == 2 ? 8 : 1 + uint32_t(rng() % 3);  // (every third case: windows that can outrun the buffer)
        for (uint32_t r = 0; r < rounds * dlist::WAVES && at < n; ++r) {
            const uint32_t c = std::min<uint32_t>(n - at, 1 + uint32_t(rng() % 64));
            L.append(std::vector<Entry>(in.begin() + at, in.begin() + at + c));
            at += c;
        }
        if (L.cur > k && !L.fail) L.cut();
    }
    if (L.fail) {  // given up: scan_many_kernel's item.  Only more entries than the buffer holds can do that.
        ++*given_up;
        if (n <= dlist::CAP) std::printf("FAIL case %u (k %u, n %u, shape %d) overflowed\n", seed, k, n, shape);
        return n <= dlist::CAP;
    }
    L.cut();
    *cuts += L.cuts;
    std::vector<Entry> want = in;
    const size_t keep = std::min<size_t>(n, k);
    std::partial_sort(want.begin(), want.begin() + keep, want.end(), [](const Entry &a, const Entry &b) { return rrk::better(a, b); });
    int bad = L.cur != keep;
    for (size_t i = 0; i < keep && !bad; ++i) bad = L.key[i] != want[i].key || L.doc[i] != want[i].pos;
    if (bad) std::printf("FAIL case %u (k %u, n %u, shape %d): the list differs from partial_sort\n", seed, k, n, shape);
    return bad;
}

int main() {
    uint32_t cuts = 0, given_up = 0;
    for (uint32_t seed = 0; seed < 160; ++seed)
        if (one_case(seed, &cuts, &given_up)) return 1;
    std::printf("160 cases, %u cuts, %u given up\n", cuts, given_up);
    if (cuts < 300 || given_up < 3) return std::printf("FAIL the cases do not exercise the cut or the overflow\n"), 1;
    std::printf("fuzz done\n");
    return 0;
}
