// fuzz_cast.cpp -- csrc/cast_lane.h on the CPU under AddressSanitizer + UBSan: merge_document (the rank-and-merge of one document, the
// text the wave kernel of cast.hip runs lane by lane) against a restatement with std::sort + memcmp and a loop, the key compare against
// memcmp, the saturating sums, fieldnorm_of against a linear search and doc_class at its edges.  Stand-alone, built and run by
// tests/test_cast_host.py.  Every array is allocated exactly (std::vector of the document's size): a read or write past a document is
// a heap-buffer-overflow.
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
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL: ");        \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            if (++failures > 20) std::exit(1); \
        }                                 \
    } while (0)

static Key key_of(const uint8_t (&b)[16]) {
    Key k;
    std::memcpy(&k, b, 16);
    return k;
}
static int cmp(const Key &a, const Key &b) { return std::memcmp(&a, &b, 16); }

struct Doc {
    std::vector<Key> key;
    std::vector<uint32_t> count;
};

// the restatement: sort (key, count) by memcmp, merge equal keys in 64 bits, clamp
static void reference(const Doc &d, std::vector<Key> &key, std::vector<uint32_t> &tf, uint32_t &length) {
    std::vector<size_t> order(d.key.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cmp(d.key[a], d.key[b]) < 0; });
    key.clear();
    tf.clear();
    uint64_t len = 0;
    for (size_t i = 0; i < order.size();) {
        size_t j = i;
        uint64_t sum = 0;
        while (j < order.size() && cmp(d.key[order[j]], d.key[order[i]]) == 0) sum += d.count[order[j++]];
        const uint32_t v = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(sum);
        key.push_back(d.key[order[i]]);
        tf.push_back(v);
        len += v;
        i = j;
    }
    length = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(len);
}

static void check_doc(const Doc &d, const char *what) {
    const uint32_t n = uint32_t(d.key.size());
    std::vector<Key> out_key(n), want_key;
    std::vector<uint32_t> out_tf(n), want_tf;
    std::vector<uint8_t> head(n);
    uint32_t length = 12345, want_len = 0;
    const uint32_t kept = merge_document(d.key.data(), d.count.data(), n, out_key.data(), out_tf.data(), head.data(), &length);
    reference(d, want_key, want_tf, want_len);
    ++checked;
    EXPECT(kept == want_key.size(), "%s: %u elements, expected %zu", what, kept, want_key.size());
    EXPECT(length == want_len, "%s: length %u, expected %u", what, length, want_len);
    for (uint32_t i = 0; i < kept && i < want_key.size(); ++i) {
        EXPECT(cmp(out_key[i], want_key[i]) == 0, "%s: key %u differs", what, i);
        EXPECT(out_tf[i] == want_tf[i], "%s: tf %u is %u, expected %u", what, i, out_tf[i], want_tf[i]);
        if (i) EXPECT(key_less(out_key[i - 1], out_key[i]), "%s: keys not strictly ascending at %u", what, i);
    }
}

static Doc doc_of(std::initializer_list<std::pair<Key, uint32_t>> l) {
    Doc d;
    for (const auto &e : l) {
        d.key.push_back(e.first);
        d.count.push_back(e.second);
    }
    return d;
}

static void test_compare() {
    std::mt19937_64 rng(1);
    for (int i = 0; i < 200000; ++i) {
        uint8_t a[16], b[16];
        for (int j = 0; j < 16; ++j) {
            a[j] = uint8_t(rng());
            b[j] = (rng() & 3) ? a[j] : uint8_t(rng());  // long common prefixes
        }
        const Key ka = key_of(a), kb = key_of(b);
        const int c = cmp(ka, kb);
        ++checked;
        EXPECT(key_less(ka, kb) == (c < 0) && key_less(kb, ka) == (c > 0) && key_equal(ka, kb) == (c == 0), "compare %d", i);
    }
    // the traps: one differing byte at 0, 7, 8 and 15; 0x7f against 0x80 (a signed compare orders them the other way)
    for (int pos : {0, 7, 8, 15}) {
        uint8_t a[16] = {0}, b[16] = {0};
        for (int j = 0; j < 16; ++j) a[j] = b[j] = uint8_t(0x55 + j);
        a[pos] = 0x7f;
        b[pos] = 0x80;
        ++checked;
        EXPECT(key_less(key_of(a), key_of(b)) && !key_less(key_of(b), key_of(a)), "0x7f / 0x80 at byte %d", pos);
    }
    {  // byte 7 decides before byte 8, byte 0 before byte 7 (a little-endian compare of a half orders them the other way)
        uint8_t a[16] = {0}, b[16] = {0};
        a[7] = 1;
        b[8] = 2;
        EXPECT(key_less(key_of(b), key_of(a)), "byte 7 against byte 8");
        uint8_t c[16] = {0}, e[16] = {0};
        c[0] = 1;
        e[7] = 2;
        EXPECT(key_less(key_of(e), key_of(c)), "byte 0 against byte 7");
        checked += 2;
    }
}

static void test_sums() {
    EXPECT(sat_add(0xFFFFFFFFu, 1) == 0xFFFFFFFFu, "sat_add max + 1");
    EXPECT(sat_add(0x80000000u, 0x80000000u) == 0xFFFFFFFFu, "sat_add 2^31 twice");
    EXPECT(sat_add(0x7FFFFFFFu, 0x7FFFFFFFu) == 0xFFFFFFFEu, "sat_add below the clamp");
    EXPECT(sat_add(sat_add(0x7FFFFFFFu, 0x7FFFFFFFu), 0x7FFFFFFFu) == 0xFFFFFFFFu, "sat_add three times");
    EXPECT(sat_add(0, 0) == 0 && sat_add(5, 7) == 12, "sat_add small");
    EXPECT(clamp_u32(0xFFFFFFFFull) == 0xFFFFFFFFu && clamp_u32(0x100000000ull) == 0xFFFFFFFFu && clamp_u32(17) == 17, "clamp_u32");
    checked += 6;
}

static void test_documents() {
    uint8_t z[16] = {0}, one[16] = {1}, b15[16] = {0}, b8[16] = {0}, b7[16] = {0}, lo[16], hi[16];
    b15[15] = 1;
    b8[8] = 1;
    b7[7] = 1;
    std::memset(lo, 0x7f, 16);
    std::memset(hi, 0x80, 16);
    const Key Z = key_of(z), ONE = key_of(one), B15 = key_of(b15), B8 = key_of(b8), B7 = key_of(b7), LO = key_of(lo), HI = key_of(hi);
    check_doc(Doc{}, "empty");
    check_doc(doc_of({{Z, 3}}), "one");
    check_doc(doc_of({{ONE, 1}, {Z, 2}}), "empty lexeme beside 0x01");
    check_doc(doc_of({{B7, 1}, {B8, 2}, {B15, 3}, {Z, 4}}), "bytes 7, 8, 15");
    check_doc(doc_of({{HI, 1}, {LO, 2}}), "0x7f and 0x80");
    check_doc(doc_of({{B8, 1}, {B8, 2}, {B8, 3}}), "all equal");
    check_doc(doc_of({{B8, 0xFFFFFFFFu}, {B8, 1}}), "0xFFFFFFFF + 1");
    check_doc(doc_of({{B8, 0x80000000u}, {Z, 1}, {B8, 0x80000000u}}), "0x80000000 x 2");
    check_doc(doc_of({{B8, 0x7FFFFFFFu}, {B8, 0x7FFFFFFFu}, {B8, 0x7FFFFFFFu}}), "0x7FFFFFFF x 3");
    check_doc(doc_of({{B8, 0xFFFFFFF0u}, {B7, 0xFFFFFFF0u}}), "distinct keys, length saturates");
    std::mt19937_64 rng(7);
    for (int it = 0; it < 4000; ++it) {
        Doc d;
        const uint32_t n = it < 200 ? uint32_t(it % 67) : uint32_t(rng() % 130);
        const uint32_t distinct = 1 + uint32_t(rng() % (n + 1));  // few distinct keys: long runs of equals
        std::vector<Key> pool(distinct);
        for (Key &k : pool) {
            uint8_t b[16];
            const int mode = int(rng() % 4);
            for (int j = 0; j < 16; ++j) b[j] = mode == 0 ? uint8_t(rng()) : mode == 1 ? uint8_t(0x7f + (rng() & 1)) : mode == 2 ? uint8_t(rng() & 1) : uint8_t((j == 7 || j == 8) ? rng() : 0x33);
            k = key_of(b);
        }
        for (uint32_t i = 0; i < n; ++i) {
            d.key.push_back(pool[rng() % distinct]);
            const int mode = int(rng() % 8);
            d.count.push_back(mode == 0 ? 0xFFFFFFFFu : mode == 1 ? 0x80000000u : mode == 2 ? 0x7FFFFFFFu : 1u + uint32_t(rng() % 9));
        }
        check_doc(d, "random");
    }
}

static void test_fieldnorm_and_class() {
    // a table of the reference's shape: 0 .. 39 exact, then growing steps
    uint32_t t[256];
    for (uint32_t i = 0; i < 256; ++i) t[i] = i < 40 ? i : t[i - 1] + (1u << ((i - 40) / 8 + 3 > 24 ? 24 : (i - 40) / 8 + 3));
    std::mt19937_64 rng(3);
    for (int it = 0; it < 100000; ++it) {
        const uint32_t len = it < 300 ? uint32_t(it) : it & 1 ? uint32_t(rng()) : t[rng() % 256] + uint32_t(rng() % 3) - 1;
        uint32_t want = 0;
        for (uint32_t c = 0; c < 256; ++c)
            if (t[c] <= len) want = c;
        ++checked;
        EXPECT(fieldnorm_of(t, len) == want, "fieldnorm_of(%u) = %u, expected %u", len, fieldnorm_of(t, len), want);
    }
    EXPECT(fieldnorm_of(t, 0xFFFFFFFFu) == 255, "fieldnorm of the longest length");
    EXPECT(doc_class(0, 64, 2048) == CLASS_WAVE && doc_class(64, 64, 2048) == CLASS_WAVE && doc_class(65, 64, 2048) == CLASS_GROUP, "wave edge");
    EXPECT(doc_class(2048, 64, 2048) == CLASS_GROUP && doc_class(2049, 64, 2048) == CLASS_GENERAL, "group edge");
    EXPECT(doc_class(0, 0, 2048) == CLASS_GROUP && doc_class(5, 0, 0) == CLASS_GENERAL && doc_class(0, 0, 0) == CLASS_GENERAL, "classes off");
    EXPECT(doc_class(9, 8, 0) == CLASS_GENERAL && doc_class(8, 8, 0) == CLASS_WAVE && doc_class(9, 8, 16) == CLASS_GROUP, "lowered bounds");
    checked += 5;
}

int main() {
    test_compare();
    test_sums();
    test_documents();
    test_fieldnorm_and_class();
    std::printf("%ld checks\n", checked);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("fuzz done\n");
    return 0;
}
