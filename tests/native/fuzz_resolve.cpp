// fuzz_resolve.cpp -- csrc/resolve_lane.h on the CPU under AddressSanitizer + UBSan: intern_lane against vbm25::blake3 / vbm25_intern
// (csrc/blake3.cpp, linked into this program) and lookup_lane against std::lower_bound with memcmp.  Stand-alone, built and run by
// tests/test_resolve_host.py.
//
// Every lexeme is hashed through both loaders of resolve_lane.h:
//   ByteLoad   from a pool allocated EXACTLY (malloc of the pool's length, the lexeme under test ending at its last byte): any read
//              past the lexeme is a heap-buffer-overflow
//   WordLoad   (what the kernels use) from a pool whose allocation ends on the next multiple of 4 and not a byte later: any read past
//              the last word that holds a byte of the lexeme is a heap-buffer-overflow
// and with the chaining-value stack allocated to exactly stack_levels(len) slots.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/resolve_lane.h"
#include "../../vectorchord-bm25_amd/csrc/vbm25_internal.h"

namespace vbm25 {
int set_error(int code, const char *, ...) { return code; }  // the library defines it in error.cpp
}

using namespace vbm25::rsv;

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

static void seed_to_words(const uint8_t *seed32, uint32_t (&w)[8]) {
    for (int i = 0; i < 8; ++i) w[i] = uint32_t(seed32[4 * i]) | uint32_t(seed32[4 * i + 1]) << 8 | uint32_t(seed32[4 * i + 2]) << 16 | uint32_t(seed32[4 * i + 3]) << 24;
}

// the lexeme placed at offset `align` of a pool that ends with it, through both loaders; returns the key's 16 bytes
static void intern_both(const uint8_t *seed32, const std::vector<uint8_t> &lex, size_t align, uint8_t *key16) {
    uint32_t sw[8];
    seed_to_words(seed32, sw);
    const size_t n = align + lex.size();
    const uint32_t levels = stack_levels(lex.size());
    uint32_t *stack = levels ? static_cast<uint32_t *>(std::malloc(levels * 32)) : nullptr;
    // ByteLoad: the pool is n bytes and not one more
    uint8_t *exact = static_cast<uint8_t *>(std::malloc(n ? n : 1));
    std::memset(exact, 0xAB, n);
    if (!lex.empty()) std::memcpy(exact + align, lex.data(), lex.size());
    const Key kb = intern_lane(sw, ByteLoad{exact}, align, lex.size(), stack, 1);
    std::free(exact);
    // WordLoad: 4-byte aligned base (malloc's), n rounded up to 4 bytes and not one more; the padding is not zero
    const size_t n4 = (n + 3) / 4 * 4;
    uint8_t *words = static_cast<uint8_t *>(std::malloc(n4 ? n4 : 4));
    std::memset(words, 0xCD, n4);
    if (!lex.empty()) std::memcpy(words + align, lex.data(), lex.size());
    const Key kw = intern_lane(sw, WordLoad{reinterpret_cast<const uint32_t *>(words)}, align, lex.size(), stack, 1);
    std::free(words);
    std::free(stack);
    EXPECT(kb.x == kw.x && kb.y == kw.y, "ByteLoad and WordLoad differ: len %zu align %zu", lex.size(), align);
    std::memcpy(key16, &kb.x, 8);
    std::memcpy(key16 + 8, &kb.y, 8);
}

static void check_lexeme(const uint8_t *seed32, const std::vector<uint8_t> &lex, size_t align, const char *what) {
    uint8_t got[16], want[16];
    intern_both(seed32, lex, align, got);
    const int rc = vbm25_intern(seed32, lex.data(), lex.size(), want);
    EXPECT(rc == 0, "vbm25_intern refused %s len %zu", what, lex.size());
    EXPECT(!std::memcmp(got, want, 16), "%s: len %zu align %zu differs from vbm25_intern", what, lex.size(), align);
    ++checked;
}

static std::vector<uint8_t> pattern(size_t n) {  // the published vectors' input: byte i = i % 251
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = uint8_t(i % 251);
    return v;
}

static void hex(const uint8_t *p, size_t n, char *out) {
    for (size_t i = 0; i < n; ++i) std::sprintf(out + 2 * i, "%02x", p[i]);
}

static void test_intern() {
    const uint8_t *KEY = reinterpret_cast<const uint8_t *>("whats the Elvish word for friend");
    // the published keyed vectors (tests/test_blake3.py): intern of a hashed lexeme is the first 16 bytes
    struct {
        size_t n;
        const char *hex32;
    } keyed[] = {{0, "92b2b75604ed3c761f9d6f62392c8a9227ad0ea3f09573e783f1498a4ed60d26"},
                 {1, "6d7878dfff2f485635d39013278ae14f1454b8c0a3a2d34bc1ab38228a80c95b"}};
    for (auto &kv : keyed) {
        uint8_t h[32];
        char hx[65];
        vbm25::blake3(KEY, pattern(kv.n).data(), kv.n, h, 32);
        hex(h, 32, hx);
        EXPECT(!std::strcmp(hx, kv.hex32), "blake3.cpp misses the published keyed vector of length %zu", kv.n);
    }
    {  // length 1 of the published input is the byte 0: a NUL, so intern hashes it -- straight against the published bytes
        uint8_t got[16];
        char hx[33];
        intern_both(KEY, pattern(1), 0, got);
        hex(got, 16, hx);
        EXPECT(!std::strncmp(hx, keyed[1].hex32, 32), "intern_lane misses the published keyed vector of length 1: %s", hx);
    }
    // every length 0 .. 130 and the chunk / tree edges, of the published input (it starts with a NUL: all hashed) and of NUL-free bytes
    // (short ones padded), at every start alignment
    std::vector<size_t> lens;
    for (size_t n = 0; n <= 130; ++n) lens.push_back(n);
    for (size_t n : {1023, 1024, 1025, 2046, 2047, 2048, 2049, 3072, 3073, 4096, 4097, 8192, 8193}) lens.push_back(n);
    for (size_t n : lens) {
        std::vector<uint8_t> plain(n);
        for (size_t i = 0; i < n; ++i) plain[i] = uint8_t(1 + (i * 7 + n) % 255);
        for (size_t align = 0; align < 16; ++align) {
            check_lexeme(KEY, pattern(n), align, "published input");
            check_lexeme(KEY, plain, align, "NUL-free input");
        }
    }
    // a NUL at the first, a middle and the last byte
    for (size_t n : {1, 2, 3, 8, 15, 16, 17, 64, 65, 1024, 1025}) {
        for (size_t at : {size_t(0), n / 2, n - 1}) {
            std::vector<uint8_t> v(n, 'a');
            v[at] = 0;
            for (size_t align : {0, 1, 2, 3, 5, 15}) check_lexeme(KEY, v, align, "NUL inside");
        }
    }
    // a lexeme whose hash has byte 15 == 0 (about 1 in 256): the key's last byte becomes 1
    {
        bool found = false;
        for (uint32_t i = 0; i < 100000 && !found; ++i) {
            char s[40];
            const int n = std::snprintf(s, sizeof s, "byte15-is-zero-%u", i);
            uint8_t h[32];
            vbm25::blake3(KEY, reinterpret_cast<const uint8_t *>(s), size_t(n), h, 32);
            if (h[15] != 0) continue;
            found = true;
            std::vector<uint8_t> v(s, s + n);
            uint8_t got[16];
            intern_both(KEY, v, 3, got);
            EXPECT(got[15] == 1 && !std::memcmp(got, h, 15), "byte 15 == 0 is not forced to 1 (%s)", s);
            check_lexeme(KEY, v, 3, "byte 15 == 0");
        }
        EXPECT(found, "no lexeme with hash byte 15 == 0 in 100000 tries");
    }
    // random lexemes, random seeds
    std::mt19937_64 rng(20261019);
    for (int it = 0; it < 3000; ++it) {
        uint8_t seed[32];
        for (auto &b : seed) b = uint8_t(rng());
        const size_t n = (it % 10 == 0) ? rng() % 5000 : rng() % 200;
        std::vector<uint8_t> v(n);
        const bool text = it % 3 != 0;  // (text: no NUL, so short ones take the padded path)
        for (auto &b : v) b = text ? uint8_t(1 + rng() % 255) : uint8_t(rng());
        check_lexeme(seed, v, rng() % 16, "random");
    }
}

struct K16 {
    uint8_t b[16];
};
static bool k16_less(const K16 &a, const K16 &b) { return std::memcmp(a.b, b.b, 16) < 0; }

static void check_lookup(std::vector<K16> vocab, const std::vector<K16> &probes, const char *what) {
    std::sort(vocab.begin(), vocab.end(), k16_less);
    vocab.erase(std::unique(vocab.begin(), vocab.end(), [](const K16 &a, const K16 &b) { return !std::memcmp(a.b, b.b, 16); }), vocab.end());
    // exactly n keys, 16-byte aligned as the device's are
    Key *keys = vocab.empty() ? nullptr : static_cast<Key *>(std::aligned_alloc(16, 16 * vocab.size()));
    for (size_t i = 0; i < vocab.size(); ++i) std::memcpy(&keys[i], vocab[i].b, 16);
    auto probe = [&](const K16 &p) {
        Key k;
        std::memcpy(&k, p.b, 16);
        const uint32_t got = lookup_lane(keys, uint32_t(vocab.size()), k);
        auto it = std::lower_bound(vocab.begin(), vocab.end(), p, k16_less);
        const uint32_t want = (it != vocab.end() && !std::memcmp(it->b, p.b, 16)) ? uint32_t(it - vocab.begin()) : NOT_FOUND;
        EXPECT(got == want, "%s: lookup gives %u, lower_bound %u (vocabulary of %zu)", what, got, want, vocab.size());
        ++checked;
    };
    for (const K16 &p : probes) probe(p);
    for (const K16 &p : vocab) {  // every key itself, and its neighbours one bit away in bytes 0, 7, 8 and 15
        probe(p);
        for (int byte : {0, 7, 8, 15}) {
            K16 q = p;
            q.b[byte] ^= 1;
            probe(q);
            q = p;
            q.b[byte] ^= 0x80;
            probe(q);
        }
    }
    std::free(keys);
}

static K16 k16(std::initializer_list<int> head, int fill = 0) {
    K16 k;
    std::memset(k.b, fill, 16);
    int i = 0;
    for (int v : head) k.b[i++] = uint8_t(v);
    return k;
}

static void test_lookup() {
    K16 lowest = k16({}, 0), highest = k16({}, 0xFF);
    std::vector<K16> edge;
    // keys that differ only in byte 7, only in byte 8, only in byte 15
    for (int byte : {7, 8, 15})
        for (int v : {0x00, 0x01, 0x7F, 0x80, 0xFF}) {
            K16 k = k16({}, 0x40);
            k.b[byte] = uint8_t(v);
            edge.push_back(k);
        }
    // bytes >= 0x80 next to bytes < 0x80 (a signed compare would turn them round), at the first byte of either half
    edge.push_back(k16({0x7F, 0xFF}, 0x11));
    edge.push_back(k16({0x80, 0x00}, 0x11));
    edge.push_back(k16({0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x7F}, 0x22));
    edge.push_back(k16({0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x80}, 0x22));
    // 00 01 .. against 01 00 .. (byte order of the 64-bit compare)
    edge.push_back(k16({0x00, 0x01}, 0));
    edge.push_back(k16({0x01, 0x00}, 0));
    edge.push_back(k16({0x33, 0x33, 0x33, 0x33, 0x33, 0x33, 0x33, 0x33, 0x00, 0x01}, 0));
    edge.push_back(k16({0x33, 0x33, 0x33, 0x33, 0x33, 0x33, 0x33, 0x33, 0x01, 0x00}, 0));
    std::vector<K16> probes = edge;
    probes.push_back(lowest);
    probes.push_back(highest);

    check_lookup({}, probes, "0 keys");
    for (const K16 &k : edge) check_lookup({k}, probes, "1 key");
    for (size_t i = 0; i + 1 < edge.size(); ++i) check_lookup({edge[i], edge[i + 1]}, probes, "2 keys");
    check_lookup(edge, probes, "the edge keys");
    std::mt19937_64 rng(7);
    std::vector<K16> big = edge;
    while (big.size() < 1000) {
        K16 k;
        for (auto &b : k.b) b = uint8_t(rng());
        if (big.size() % 3 == 0) std::memcpy(k.b, big[rng() % big.size()].b, 8 + rng() % 8);  // shared prefixes of 8 .. 15 bytes
        big.push_back(k);
    }
    for (int i = 0; i < 2000; ++i) {
        K16 k;
        for (auto &b : k.b) b = uint8_t(rng());
        probes.push_back(k);
    }
    check_lookup(big, probes, "1000 keys");
}

int main() {
    test_intern();
    const long n_intern = checked;
    test_lookup();
    std::printf("intern: %ld lexemes checked; lookup: %ld probes checked\n", n_intern, checked - n_intern);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("fuzz done\n");
    return 0;
}
