// resolve_lane.h -- the per-lexeme and per-key functions of the query resolver (resolve.hip): intern (vector.rs:19-35) and
// address_tokens::read (address_tokens.rs:61-98) for ONE lexeme / ONE key.  __host__ __device__, and plain C++ as well: the kernels of
// resolve.hip are loops over these, and tests/native/fuzz_resolve.cpp compiles the same text with g++ under AddressSanitizer against
// blake3.cpp and std::lower_bound.
//
//   intern_lane   BLAKE3 keyed hash written from the specification (the BLAKE3 paper, section 2), one lane a lexeme.  The seven rounds
//                 are unrolled with the message permutation folded into compile-time indices (sched(R, i)): the 16 state words and
//                 the 16 message words are named by constants only and stay in registers.  The only array a lane indexes by a run-time
//                 value is the chaining-value stack of a lexeme of more than one chunk (> 1024 bytes): the caller hands it over as
//                 (pointer, stride) -- LDS in the kernel, one column a lane; a local array on the host -- with one slot per level,
//                 stack_levels(longest lexeme) of them.  A lexeme of one chunk never touches it (nullptr is fine).
//   message bytes come through a loader, because lexemes sit back to back in a byte pool and start at every alignment:
//                 ByteLoad   byte reads of the lexeme's own bytes, nothing else (the host harness: a pool allocated exactly)
//                 WordLoad   aligned 32-bit reads, two funnelled into each message word.  Only words that hold at least one byte of the
//                            lexeme are read, so the pool needs a 4-byte aligned base and an end rounded up to 4 bytes, nothing more
//                            (the kernels: the library owns the staging buffer)
//   lookup_lane   the bisection of vbm25_lookup_terms in key_cmp's order (growing.h): memcmp of 16 bytes = two big-endian u64
//                 compares, unsigned.
#ifndef VBM25_RESOLVE_LANE_H
#define VBM25_RESOLVE_LANE_H

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RSV_HD __host__ __device__ __forceinline__
#else
#define RSV_HD inline __attribute__((always_inline))
#endif

namespace vbm25 {
namespace rsv {

// a 16-byte token key as two little-endian loads of its bytes 0..7 and 8..15 (ulonglong2's layout)
struct alignas(16) Key {
    uint64_t x, y;
};

constexpr uint32_t NOT_FOUND = 0xFFFFFFFFu;
constexpr uint32_t B3_CHUNK_START = 1, B3_CHUNK_END = 2, B3_PARENT = 4, B3_ROOT = 8, B3_KEYED = 16;
constexpr uint32_t B3_BLOCK = 64, B3_CHUNK = 1024;

// the message permutation of the specification, and its R-th power: round R reads message word sched(R, i) where round 0 reads word i
constexpr int perm(int i) {
    constexpr int P[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
    return P[i];
}
constexpr int sched(int r, int i) { return r == 0 ? i : sched(r - 1, perm(i)); }
template <int V>
struct IC {
    static constexpr int v = V;
};

// n = 16, 12, 8, 7.  On the device one v_alignbit_b32 (a funnel shift of x with itself).
#if defined(__clang__)
RSV_HD uint32_t rotr(uint32_t x, uint32_t n) { return __builtin_rotateright32(x, n); }
#else
RSV_HD uint32_t rotr(uint32_t x, uint32_t n) { return (x >> n) | (x << (32 - n)); }
#endif

RSV_HD void g(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t mx, uint32_t my) {
    a = a + b + mx;
    d = rotr(d ^ a, 16);
    c = c + d;
    b = rotr(b ^ c, 12);
    a = a + b + my;
    d = rotr(d ^ a, 8);
    c = c + d;
    b = rotr(b ^ c, 7);
}

#define RSV_M(R, i) m[IC<sched(R, i)>::v]
template <int R>
RSV_HD void round_fn(uint32_t (&s)[16], const uint32_t (&m)[16]) {
    g(s[0], s[4], s[8], s[12], RSV_M(R, 0), RSV_M(R, 1));
    g(s[1], s[5], s[9], s[13], RSV_M(R, 2), RSV_M(R, 3));
    g(s[2], s[6], s[10], s[14], RSV_M(R, 4), RSV_M(R, 5));
    g(s[3], s[7], s[11], s[15], RSV_M(R, 6), RSV_M(R, 7));
    g(s[0], s[5], s[10], s[15], RSV_M(R, 8), RSV_M(R, 9));
    g(s[1], s[6], s[11], s[12], RSV_M(R, 10), RSV_M(R, 11));
    g(s[2], s[7], s[8], s[13], RSV_M(R, 12), RSV_M(R, 13));
    g(s[3], s[4], s[9], s[14], RSV_M(R, 14), RSV_M(R, 15));
}
#undef RSV_M

// the compression function; only the first 8 output words are ever needed here (a chaining value, or the first 32 root bytes)
RSV_HD void compress(const uint32_t (&cv)[8], const uint32_t (&m)[16], uint64_t counter, uint32_t block_len, uint32_t flags,
                     uint32_t (&out)[8]) {
    uint32_t s[16] = {cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7], 0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                      uint32_t(counter), uint32_t(counter >> 32), block_len, flags};
    round_fn<0>(s, m);
    round_fn<1>(s, m);
    round_fn<2>(s, m);
    round_fn<3>(s, m);
    round_fn<4>(s, m);
    round_fn<5>(s, m);
    round_fn<6>(s, m);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = s[i] ^ s[i + 8];
}

// the low `n` bytes of a word (n = 0 .. 4 and beyond)
RSV_HD uint32_t keep_bytes(uint32_t w, uint32_t n) { return n >= 4 ? w : (w & ((1u << (8 * n)) - 1u)); }

// bytes pos .. pos + n of the pool (n <= 64) -> 16 little-endian message words, zero padded
struct ByteLoad {
    const uint8_t *pool;
    RSV_HD void block(uint64_t pos, uint32_t n, uint32_t (&m)[16]) const {
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            uint32_t w = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (4 * i + j < n) w |= uint32_t(pool[pos + 4 * i + j]) << (8 * j);
            m[i] = w;
        }
    }
};
struct WordLoad {
    const uint32_t *pool;  // 4-byte aligned base; the allocation ends on a multiple of 4
    RSV_HD void block(uint64_t pos, uint32_t n, uint32_t (&m)[16]) const {
        const uint64_t a = pos >> 2;
        const uint32_t sh = uint32_t(pos & 3) * 8;
        const uint32_t need = (uint32_t(pos & 3) + n + 3) >> 2;  // aligned words that hold a byte of [pos, pos + n): <= 17
        uint32_t w[17];
#pragma unroll
        for (uint32_t i = 0; i < 17; ++i) w[i] = i < need ? pool[a + i] : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t v = uint32_t(((uint64_t(w[i + 1]) << 32) | w[i]) >> sh);
            m[i] = 4 * i < n ? keep_bytes(v, n - 4 * i) : 0u;
        }
    }
};

// slots of the chaining-value stack a lexeme of `len` bytes needs: one per bit of (its number of chunks - 1)
RSV_HD uint32_t stack_levels(uint64_t len) {
    if (len <= B3_CHUNK) return 0;
    uint64_t done = (len - 1) / B3_CHUNK;  // whole chunks in front of the last one: the stack holds popcount(done) values
    uint32_t levels = 0;
    while (done) {
        ++levels;
        done >>= 1;
    }
    return levels;
}

// true when the lexeme takes the hash: 16 bytes or more, or a NUL inside (`first` = its first block as message words)
RSV_HD bool needs_hash(const uint32_t (&first)[16], uint64_t len) {
    if (len >= 16) return true;
    bool nul = false;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (4 * i + j < len && ((first[i] >> (8 * j)) & 0xFFu) == 0) nul = true;
    }
    return nul;
}

// intern (vector.rs:19-35) of the lexeme at bytes [begin, begin + len) of the pool.  key[8] = the seed as little-endian words (not read
// when the lexeme is short and without NUL).  stack[(8 * level + word) * stride]: see the header comment.
template <class Load>
RSV_HD Key intern_lane(const uint32_t (&key)[8], const Load &ld, uint64_t begin, uint64_t len, uint32_t *stack, uint32_t stride) {
    uint32_t m[16];
    ld.block(begin, len < B3_BLOCK ? uint32_t(len) : B3_BLOCK, m);
    if (!needs_hash(m, len)) return Key{uint64_t(m[1]) << 32 | m[0], uint64_t(m[3]) << 32 | m[2]};

    const uint32_t kf = B3_KEYED;
    uint32_t cv[8], out[8];
    uint64_t pos = 0, chunk = 0;  // bytes consumed; chunks finished (= the counter of the current chunk)
    uint32_t sp = 0;
    // the node whose compression gives the last chunk's chaining value (or, alone, the root): cv, m, chunk, last_len, last_flags
    uint32_t last_len, last_flags;
    for (;;) {
        const uint64_t rest = len - pos;
        const uint32_t take = rest < B3_CHUNK ? uint32_t(rest) : B3_CHUNK;
#pragma unroll
        for (int i = 0; i < 8; ++i) cv[i] = key[i];
        uint32_t off = 0;
        // every block but the chunk's last chains through cv
        while (take - off > B3_BLOCK) {
            if (pos + off) ld.block(begin + pos + off, B3_BLOCK, m);  // (the lexeme's first block is loaded already)
            compress(cv, m, chunk, B3_BLOCK, kf | (off == 0 ? B3_CHUNK_START : 0u), out);
#pragma unroll
            for (int i = 0; i < 8; ++i) cv[i] = out[i];
            off += B3_BLOCK;
        }
        last_len = take - off;
        last_flags = kf | (off == 0 ? B3_CHUNK_START : 0u) | B3_CHUNK_END;
        if (pos + off) ld.block(begin + pos + off, last_len, m);
        if (pos + take == len) break;
        // a finished chunk that is not the last: its chaining value merges up the tree, one pop per trailing zero bit of the number
        // of chunks so far, and is pushed
        compress(cv, m, chunk, last_len, last_flags, out);
        ++chunk;
        for (uint64_t total = chunk; (total & 1) == 0; total >>= 1) {
            --sp;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                m[i] = stack[size_t(8 * sp + i) * stride];
                m[8 + i] = out[i];
                cv[i] = key[i];
            }
            compress(cv, m, 0, B3_BLOCK, kf | B3_PARENT, out);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) stack[size_t(8 * sp + i) * stride] = out[i];
        ++sp;
        pos += take;
    }
    // fold the stack from the right: the root is the last parent, or the only chunk
    uint64_t counter = chunk;
    while (sp > 0) {
        compress(cv, m, counter, last_len, last_flags, out);
        --sp;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            m[i] = stack[size_t(8 * sp + i) * stride];
            m[8 + i] = out[i];
            cv[i] = key[i];
        }
        counter = 0;
        last_len = B3_BLOCK;
        last_flags = kf | B3_PARENT;
    }
    compress(cv, m, counter, last_len, last_flags | B3_ROOT, out);
    if ((out[3] >> 24) == 0) out[3] |= 1u << 24;  // byte 15 forced to 1 when it is 0
    return Key{uint64_t(out[1]) << 32 | out[0], uint64_t(out[3]) << 32 | out[2]};
}

// memcmp order of two keys
RSV_HD int key_order(const Key &a, const Key &b) {
    const uint64_t a0 = __builtin_bswap64(a.x), b0 = __builtin_bswap64(b.x);
    if (a0 != b0) return a0 < b0 ? -1 : 1;
    const uint64_t a1 = __builtin_bswap64(a.y), b1 = __builtin_bswap64(b.y);
    return a1 < b1 ? -1 : a1 > b1 ? 1 : 0;
}

// address_tokens::read: the term id of `key` in the ascending vocabulary keys[0 .. n_terms), or NOT_FOUND
RSV_HD uint32_t lookup_lane(const Key *keys, uint32_t n_terms, const Key &key) {
    uint32_t lo = 0, hi = n_terms;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key_order(keys[mid], key) < 0) lo = mid + 1; else hi = mid;
    }
    return (lo < n_terms && key_order(keys[lo], key) == 0) ? lo : NOT_FOUND;
}

}  // namespace rsv
}  // namespace vbm25

#endif
