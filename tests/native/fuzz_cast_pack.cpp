// fuzz_cast_pack.cpp -- the packing functions of csrc/cast_lane.h on the CPU under AddressSanitizer + UBSan: the host's plan (pack_step /
// pack_flush) against a straightforward restatement, and the segmented rank-and-merge (lane_document, seg_head_and_sum, seg_rank_of,
// lane_span) driven lane by lane, the way cast_pack_kernel drives it, against merge_document per document.  Stand-alone, built and
// run by tests/test_caster_host.py.  Every array is allocated exactly: a read or write past a run is a heap-buffer-overflow.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/cast_lane.h"

using namespace vbm25::cst;

static int failures = 0;
static long checked = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            std::printf("FAIL: ");             \
            std::printf(__VA_ARGS__);          \
            std::printf("\n");                 \
            if (++failures > 20) std::exit(1); \
        }                                      \
    } while (0)

// ---- the plan ----
static std::vector<PackEntry> plan_of(const std::vector<uint32_t> &doc_lex, uint32_t wave_max, uint32_t group_max) {
    std::vector<PackEntry> plan;
    PackRun run;
    PackEntry e;
    const uint32_t n_docs = uint32_t(doc_lex.size() - 1);
    for (uint32_t d = 0; d < n_docs; ++d) {
        const uint32_t n = doc_lex[d + 1] - doc_lex[d];
        if (pack_step(run, d, n, doc_class(n, wave_max, group_max) == CLASS_WAVE, e)) plan.push_back(e);
    }
    if (pack_flush(run, e)) plan.push_back(e);
    return plan;
}

static void check_plan(const std::vector<uint32_t> &doc_lex, uint32_t wave_max, uint32_t group_max, const char *what) {
    const std::vector<PackEntry> plan = plan_of(doc_lex, wave_max, group_max);
    const uint32_t n_docs = uint32_t(doc_lex.size() - 1);
    ++checked;
    // the restatement: the next wave-class document starts an entry; the entry takes the following documents while they are of the
    // wave class and the entry stays within 64 lexemes and 64 documents
    size_t at = 0;
    uint32_t d = 0;
    while (d < n_docs) {
        auto wave = [&](uint32_t x) { return doc_class(doc_lex[x + 1] - doc_lex[x], wave_max, group_max) == CLASS_WAVE; };
        if (!wave(d)) {
            ++d;
            continue;
        }
        uint32_t end = d + 1;
        while (end < n_docs && wave(end) && end - d < 64 && doc_lex[end + 1] - doc_lex[d] <= 64) ++end;
        EXPECT(at < plan.size(), "%s: the plan ends at entry %zu, document %u is not covered", what, at, d);
        if (at >= plan.size()) return;
        EXPECT(plan[at].first == d && plan[at].count == end - d, "%s: entry %zu is (%u, %u), expected (%u, %u)", what, at, plan[at].first, plan[at].count, d,
               end - d);
        ++at;
        d = end;
    }
    EXPECT(at == plan.size(), "%s: %zu entries, expected %zu", what, plan.size(), at);
    // and the properties themselves
    std::vector<uint8_t> covered(n_docs, 0);
    uint32_t last = 0;
    for (size_t i = 0; i < plan.size(); ++i) {
        const PackEntry &e = plan[i];
        EXPECT(e.count >= 1 && e.count <= 64 && e.first + e.count <= n_docs, "%s: entry %zu has %u documents", what, i, e.count);
        if (e.first + e.count > n_docs) return;
        EXPECT(doc_lex[e.first + e.count] - doc_lex[e.first] <= 64, "%s: entry %zu has more than 64 lexemes", what, i);
        EXPECT(i == 0 || e.first >= last, "%s: entry %zu is out of order", what, i);
        last = e.first + e.count;
        for (uint32_t x = e.first; x < e.first + e.count; ++x) {
            EXPECT(doc_class(doc_lex[x + 1] - doc_lex[x], wave_max, group_max) == CLASS_WAVE, "%s: entry %zu spans document %u of another class", what, i, x);
            EXPECT(!covered[x], "%s: document %u is in two entries", what, x);
            covered[x] = 1;
        }
    }
    for (uint32_t x = 0; x < n_docs; ++x)
        if (doc_class(doc_lex[x + 1] - doc_lex[x], wave_max, group_max) == CLASS_WAVE) EXPECT(covered[x], "%s: wave-class document %u is in no entry", what, x);
}

static std::vector<uint32_t> offsets_of(const std::vector<uint32_t> &sizes) {
    std::vector<uint32_t> off(1, 0);
    for (uint32_t n : sizes) off.push_back(off.back() + n);
    return off;
}

// ---- one packed wave ----
struct Run {
    std::vector<uint32_t> sizes;  // per document
    std::vector<Key> key;         // the run's lexemes, document after document
    std::vector<uint32_t> count;
};

// what cast_pack_kernel does with one plan entry, lane after lane; every cross-lane read is a read of these arrays
static void check_run(const Run &r, const char *what) {
    const uint32_t cnt = uint32_t(r.sizes.size()), n = uint32_t(r.key.size());
    ++checked;
    if (cnt < 1 || cnt > 64 || n > 64) {
        EXPECT(false, "%s: not a run (%u documents, %u lexemes)", what, cnt, n);
        return;
    }
    const std::vector<uint32_t> off = offsets_of(r.sizes);
    // lane j's register: where document j begins (lanes at and beyond cnt hold n), exactly 64 of them
    std::vector<uint32_t> bound_reg(64);
    for (uint32_t l = 0; l < 64; ++l) bound_reg[l] = l < cnt ? off[l] : n;
    struct Bound {
        const std::vector<uint32_t> *reg;
        uint32_t operator()(uint32_t j) const { return reg->at(j); }
    } bound{&bound_reg};
    struct At {
        const Run *r;
        void operator()(uint32_t j, Key &k, uint32_t &c) const {
            k = r->key.at(j);
            c = r->count.at(j);
        }
    } at{&r};
    std::vector<uint32_t> sb(64), se(64), sum(64);
    uint32_t longest = 0;  // (the kernel's wave-wide maximum of the documents' sizes)
    for (uint32_t d = 0; d < cnt; ++d) longest = std::max(longest, (d + 1 < cnt ? bound_reg[d + 1] : n) - bound_reg[d]);
    uint64_t heads = 0;
    for (uint32_t l = 0; l < 64; ++l) {
        const uint32_t doc = lane_document(bound, cnt, l);
        EXPECT(doc < cnt, "%s: lane %u got document %u of %u", what, l, doc, cnt);
        if (doc >= cnt) return;
        sb[l] = bound(doc);
        se[l] = doc + 1 < cnt ? bound((doc + 1) & 63u) : n;
        if (l >= n) continue;
        EXPECT(off[doc] <= l && l < off[doc + 1], "%s: lane %u got document %u (lanes %u .. %u)", what, l, doc, off[doc], off[doc + 1]);
        if (seg_head_and_sum(at, longest, l, r.key[l], sb[l], se[l], sum[l])) heads |= 1ull << l;
    }
    struct IsHead {
        uint64_t mask;
        bool operator()(uint32_t j) const { return (mask >> j) & 1ull; }
    } is_head{heads};
    std::vector<Key> out_key(n);
    std::vector<uint32_t> out_tf(n);
    std::vector<uint8_t> written(n, 0);
    for (uint32_t l = 0; l < n; ++l) {
        if (!is_head(l)) continue;
        const uint32_t at_out = sb[l] + seg_rank_of(at, is_head, longest, l, r.key[l], sb[l], se[l]);
        EXPECT(at_out < n && !written[at_out], "%s: lane %u writes position %u again or outside", what, l, at_out);
        if (at_out >= n) return;
        out_key[at_out] = r.key[l];
        out_tf[at_out] = sum[l];
        written[at_out] = 1;
    }
    // against merge_document, document by document
    for (uint32_t d = 0; d < cnt; ++d) {
        const uint32_t b = off[d], m = r.sizes[d];
        const uint32_t got = uint32_t(__builtin_popcountll(heads & lane_span(bound_reg[d], d + 1 < cnt ? bound_reg[d + 1] : n)));
        std::vector<Key> want_key(m);
        std::vector<uint32_t> want_tf(m);
        std::vector<uint8_t> scratch(m);
        uint32_t length = 0;
        const uint32_t want = merge_document(r.key.data() + b, r.count.data() + b, m, want_key.data(), want_tf.data(), scratch.data(), &length);
        EXPECT(got == want, "%s: document %u has %u elements, expected %u", what, d, got, want);
        for (uint32_t i = 0; i < want && i < got; ++i) {
            EXPECT(written[b + i], "%s: document %u element %u was not written", what, d, i);
            EXPECT(key_equal(out_key[b + i], want_key[i]), "%s: document %u key %u differs", what, d, i);
            EXPECT(out_tf[b + i] == want_tf[i], "%s: document %u tf %u is %u, expected %u", what, d, i, out_tf[b + i], want_tf[i]);
        }
        for (uint32_t i = got; i < m; ++i) EXPECT(!written[b + i], "%s: document %u wrote behind its %u elements", what, d, got);
    }
}

static Key small_key(uint32_t v) {
    uint8_t b[16] = {0};
    b[0] = uint8_t('a' + v % 26);
    b[1] = uint8_t('a' + (v / 26) % 26);
    Key k;
    std::memcpy(&k, b, 16);
    return k;
}

// documents of the given sizes; keys drawn from `pool` distinct ones by rng, so they repeat inside and across documents
static Run run_of(const std::vector<uint32_t> &sizes, uint32_t pool, std::mt19937 &rng) {
    Run r;
    r.sizes = sizes;
    for (uint32_t n : sizes)
        for (uint32_t i = 0; i < n; ++i) {
            r.key.push_back(small_key(rng() % pool));
            r.count.push_back(1 + rng() % 5);
        }
    return r;
}

int main() {
    std::mt19937 rng(20240611);
    // the plan: the edges, then random size mixes under the default and lowered class bounds
    check_plan(offsets_of({}), 64, 2048, "no documents");
    check_plan(offsets_of({0}), 64, 2048, "one empty document");
    check_plan(offsets_of(std::vector<uint32_t>(64, 0)), 64, 2048, "64 empty documents");
    check_plan(offsets_of(std::vector<uint32_t>(65, 0)), 64, 2048, "65 empty documents");
    check_plan(offsets_of(std::vector<uint32_t>(64, 1)), 64, 2048, "64 lexemes");
    check_plan(offsets_of(std::vector<uint32_t>(65, 1)), 64, 2048, "65 lexemes");
    check_plan(offsets_of({1, 64, 1}), 64, 2048, "64 between ones");
    check_plan(offsets_of({5, 5, 65, 5, 5}), 64, 2048, "a group-class document splits a run");
    check_plan(offsets_of({3, 8, 9, 2, 8}), 8, 2048, "wave_max 8");
    check_plan(offsets_of({3, 8, 9, 2, 8}), 0, 2048, "wave class off");
    for (int it = 0; it < 3000; ++it) {
        std::vector<uint32_t> sizes(rng() % 300);
        const uint32_t kind = rng() % 4;
        for (uint32_t &n : sizes) n = kind == 0 ? rng() % 4 : kind == 1 ? rng() % 70 : kind == 2 ? (rng() % 10 ? rng() % 3 : 60 + rng() % 10) : (rng() % 50 ? 0 : rng() % 66);
        const uint32_t wave_max = it % 3 == 0 ? 64 : it % 3 == 1 ? 8 : 1 + rng() % 64;
        check_plan(offsets_of(sizes), wave_max, it % 5 ? 2048 : 0, "random sizes");
    }

    // the segmented merge: the runs of the GPU tests
    {
        std::vector<uint32_t> ones63(63, 1), ones64(64, 1);
        check_run(run_of(ones63, 5, rng), "63 documents of one lexeme");
        check_run(run_of(ones64, 5, rng), "64 documents of one lexeme");
        check_run(run_of({63}, 40, rng), "one document of 63");
        check_run(run_of({64}, 40, rng), "one document of 64");
        check_run(run_of({32, 32}, 20, rng), "two halves");
        check_run(run_of({31, 32}, 20, rng), "63 in two");
        check_run(run_of(std::vector<uint32_t>(64, 0), 1, rng), "64 empty documents");
        check_run(run_of({0}, 1, rng), "one empty document");
        check_run(run_of({0, 5, 0, 0, 7, 0}, 4, rng), "empty documents first, last and between");
        check_run(run_of({0, 64}, 30, rng), "an empty document in front of 64");
        check_run(run_of({64, 0}, 30, rng), "an empty document behind 64");
        check_run(run_of({1, 62, 1}, 3, rng), "a long document between ones");
        check_run(run_of({8, 8, 8, 8, 8, 8, 8, 8}, 6, rng), "eight of eight");
    }
    {  // the same lexeme in adjacent documents, with and without repeats inside each
        Run r;
        r.sizes = {1, 1, 3, 3};
        const Key k = small_key(7), o = small_key(8);
        r.key = {k, k, k, o, k, k, k, o};
        r.count = {1, 1, 2, 3, 4, 5, 6, 7};
        check_run(r, "one key in four adjacent documents");
    }
    {  // saturation inside a packed document while the neighbour's k stays 1; two documents that both saturate
        Run r;
        r.sizes = {2, 1, 2, 2};
        const Key k = small_key(3);
        r.key = {k, k, k, k, k, k, small_key(4)};
        r.count = {0xFFFFFFFFu, 1, 1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFF0u, 0x20u};
        check_run(r, "saturating sums beside a count of 1");
    }
    {  // keys that differ only in byte 15, across and inside documents
        Run r;
        r.sizes = {4, 4, 2};
        for (uint32_t i = 0; i < 10; ++i) {
            uint8_t b[16];
            std::memset(b, 0x55, 16);
            b[15] = uint8_t(i % 4 == 0 ? 0x01 : i % 4 == 1 ? 0x80 : i % 4 == 2 ? 0xFF : 0x01);
            Key k;
            std::memcpy(&k, b, 16);
            r.key.push_back(k);
            r.count.push_back(i + 1);
        }
        check_run(r, "keys that differ in byte 15 only");
    }
    // random packed waves: whatever the plan makes of random short documents, keys repeated inside and across documents
    long waves = 0;
    for (int it = 0; it < 400; ++it) {
        std::vector<uint32_t> sizes(1 + rng() % 200);
        const uint32_t kind = rng() % 3, pool = 1 + rng() % (it % 2 ? 6 : 200);
        for (uint32_t &n : sizes) n = kind == 0 ? rng() % 6 : kind == 1 ? rng() % 65 : (rng() % 4 ? 0 : rng() % 20);
        const std::vector<uint32_t> off = offsets_of(sizes);
        for (const PackEntry &e : plan_of(off, 64, 2048)) {
            std::vector<uint32_t> part(sizes.begin() + e.first, sizes.begin() + e.first + e.count);
            check_run(run_of(part, pool, rng), "random wave");
            ++waves;
        }
    }
    EXPECT(waves >= 2000, "only %ld random waves", waves);
    std::printf("fuzz done: %ld checks, %ld random waves, %d failures\n", checked, waves, failures);
    return failures ? 1 : 0;
}
