// tid_lane.h -- the per-document functions of the TID-set match (tid.hip): is a document's payload in a sorted set of ctids?
// __host__ __device__, and plain C++ as well: tid_match_kernel is a loop over these, and tests/native/fuzz_tid.cpp compiles the same
// text with g++ under AddressSanitizer and drives a model wave with them, against std::binary_search.
//
//   tid_key      a payload's three uint16_t -- [bi_hi, bi_lo, ip_posid], fetcher.rs:218-232 -- as one 48-bit integer, most significant
//                field first: ascending keys are ascending ctids
//   dir_shape    the directory of a set of n_keys sorted keys for a directory of at most 2^dir_log2 entries: entry j is key
//                j x stride (dir_source).  A set no larger than the directory is its own directory (stride 1); a larger one is cut
//                into runs of `stride` keys, the last one shorter, and the directory holds the first key of each.  The builder kernel
//                and the harness both take the shape from here.
//   tid_contains the lower-bound search in two stages.  Stage one finds the last directory entry <= key (the kernel holds the
//                directory in LDS); stage two finishes inside that entry's run of the sorted keys (HBM).  With stride 1 stage one
//                decides alone.  Exact for every n_keys >= 0.
//   tid_find     the same search over keys that may repeat, returning the first position of the key (reranker.hip's ctid -> document
//                lookup; tests/native/fuzz_tid_find.cpp checks it against std::lower_bound)
//   tid_first_live  tid_find's position walked forward over the entries of one ctid to the lowest document that is not dead, and
//                split_payload, where a document of a grown handle keeps its ctid (tests/native/fuzz_live_dead.cpp checks both)
//   live_rank_old, live_rank_delta   where an old and a new entry go when a sorted delta is merged into the sorted keys (live.hip's
//                merge kernel; tests/native/fuzz_live_merge.cpp checks them against std::merge), and live_sort_word / live_sort_step,
//                the word and the network of the delta's sort in LDS
//   match_word   a wave's ballot as the word it writes: XOR the invert mask, the bits of documents at or beyond n forced to zero
//   new_bits     the documents a word adds to an older one (the OR mode's count)
#ifndef VBM25_TID_LANE_H
#define VBM25_TID_LANE_H

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TID_HD __host__ __device__ __forceinline__
#else
#define TID_HD inline __attribute__((always_inline))
#endif

namespace vbm25 {
namespace tid {

constexpr uint32_t MAX_DIR_LOG2 = 12;      // 4096 entries: 32 KB of LDS a workgroup
// tools/tid_cost.py, profiles/tid_cost.json: 2048 entries are the fastest on documents in ctid order at every set size (what CREATE INDEX
// and VACUUM leave); on a shuffled payload plane 4096 are faster from a million TIDs up, and staging them costs the ordered case more
constexpr uint32_t DEFAULT_DIR_LOG2 = 11;
constexpr uint64_t KEY_MAX = (1ull << 48) - 1ull;

TID_HD uint64_t tid_key(const uint16_t p[3]) { return uint64_t(p[0]) << 32 | uint64_t(p[1]) << 16 | uint64_t(p[2]); }

struct DirShape {
    uint32_t n_dir;   // entries, <= 2^dir_log2 (0 for the empty set)
    uint32_t stride;  // keys a run (1: the directory is the set)
};

TID_HD DirShape dir_shape(uint64_t n_keys, uint32_t dir_log2) {
    const uint64_t cap = 1ull << (dir_log2 > MAX_DIR_LOG2 ? MAX_DIR_LOG2 : dir_log2);
    if (n_keys <= cap) return DirShape{uint32_t(n_keys), 1u};
    const uint64_t stride = (n_keys + cap - 1) / cap;
    return DirShape{uint32_t((n_keys + stride - 1) / stride), uint32_t(stride)};
}
TID_HD uint64_t dir_source(uint32_t j, uint32_t stride) { return uint64_t(j) * stride; }

TID_HD bool tid_contains(uint64_t key, const uint64_t *directory, uint32_t n_dir, const uint64_t *keys, uint64_t n_keys, uint32_t stride) {
    // stage one: lo = the number of directory entries <= key
    uint32_t lo = 0, hi = n_dir;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (directory[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return false;  // (below the smallest key, or the empty set)
    const uint32_t j = lo - 1;
    if (directory[j] == key) return true;
    if (stride == 1) return false;
    // stage two: the rest of run j, keys (j stride, min((j + 1) stride, n_keys)), all > directory[j]
    uint64_t a = dir_source(j, stride) + 1, b = dir_source(j, stride) + stride;
    if (b > n_keys) b = n_keys;
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (keys[mid] < key) a = mid + 1;
        else b = mid;
    }
    return a < n_keys && a < dir_source(j, stride) + stride && keys[a] == key;
}

constexpr uint64_t NOT_THERE = ~0ull;

// The same two stages over sorted keys that may REPEAT (reranker.hip: the payloads of a handle's documents, two documents may share
// a ctid): the FIRST position whose key equals `key`, or NOT_THERE.  Stage one finds the last directory entry < key: the first equal
// key lies in that entry's run or is the first key of the next one, so stage two is a lower bound over
// (j stride, min((j + 1) stride, n_keys)] -- one position more than a run, still a read inside keys[0 .. n_keys).  With stride 1 the
// directory is the keys and stage one decides alone.  Exact for every n_keys >= 0.
TID_HD uint64_t tid_find(uint64_t key, const uint64_t *directory, uint32_t n_dir, const uint64_t *keys, uint64_t n_keys, uint32_t stride) {
    // stage one: lo = the number of directory entries < key
    uint32_t lo = 0, hi = n_dir;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (directory[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    if (stride == 1) return lo < n_dir && directory[lo] == key ? uint64_t(lo) : NOT_THERE;
    // stage two: every key up to position a - 1 is < key, position b (when it exists) holds a key >= key
    uint64_t a = lo ? dir_source(lo - 1, stride) + 1 : 0, b = dir_source(lo, stride);
    if (b > n_keys) b = n_keys;
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (keys[mid] < key) a = mid + 1;
        else b = mid;
    }
    return a < n_keys && keys[a] == key ? a : NOT_THERE;
}

// ---- dead documents (live.hip: vbm25_doc_terms_delete*; reranker.hip: cand_lookup_kernel; tests/native/fuzz_live_dead.cpp) ----
// A handle's deletion bitmap: one bit a document, document d at bit d & 63 of word d >> 6, set = dead.
constexpr uint32_t NO_LIVE_DOC = 0xFFFFFFFFu;  // (rerank_shared.h's NO_DOC: the entry names no document)

TID_HD bool dead_bit(const uint64_t *dead, uint32_t d) { return (dead[d >> 6] >> (d & 63u)) & 1ull; }

// From tid_find's position `at` (the FIRST entry of `key`, at < n_keys) forward over the entries of the same key while their document
// is dead: equal keys lie by ascending document, so the first live one is the lowest live document of the ctid.  NO_LIVE_DOC when the
// run has none.
TID_HD uint32_t tid_first_live(uint64_t at, uint64_t key, const uint64_t *keys, const uint32_t *docs, uint64_t n_keys, const uint64_t *dead) {
    for (; at < n_keys && keys[at] == key; ++at) {
        const uint32_t d = docs[at];
        if (!dead_bit(dead, d)) return d;
    }
    return NO_LIVE_DOC;
}

// Where document d of a grown handle keeps its ctid: the plane of the documents it was bound with (d < base_docs), or the tail array
// of the appended ones.  A wave's 64 documents may straddle the split: each lane decides for itself.
TID_HD const uint16_t *split_payload(const uint16_t *base, const uint16_t *tail, uint32_t base_docs, uint64_t d) {
    return d < base_docs ? base + 3 * d : tail + 3 * (d - base_docs);
}

// ---- the merge of a sorted delta into the sorted keys (live.hip: vbm25_reranker_sync; tests/native/fuzz_live_merge.cpp) ----
// Old entries (key, doc) and delta entries (key, doc) are each sorted by key, equal keys by ascending doc, and every delta doc
// exceeds every old doc.  The merged order by (key, doc) then puts old entry i at i + #{delta keys < key_i} and delta entry j at
// j + #{old keys <= key_j}: a stable merge with the old entries first among equals, by ranks alone, one lane an entry.

// #{delta keys < key}: a lower bound over the delta's sorted keys
TID_HD uint64_t live_rank_old(uint64_t key, const uint64_t *delta_keys, uint64_t n_delta) {
    uint64_t a = 0, b = n_delta;
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (delta_keys[mid] < key) a = mid + 1;
        else b = mid;
    }
    return a;
}

// #{old keys <= key}: an upper bound in tid_find's two stages.  Stage one counts the directory entries <= key; the last of them
// opens the run in which the bound lies, and stage two finishes over (j stride, min((j + 1) stride, n_keys)] -- every key at or in
// front of position j stride is <= key, the key at (j + 1) stride (directory entry j + 1, when it exists) is > key.  With stride 1
// the directory is the keys and stage one decides alone.  Exact for every n_keys >= 0, repeated keys included.
TID_HD uint64_t live_rank_delta(uint64_t key, const uint64_t *directory, uint32_t n_dir, const uint64_t *keys, uint64_t n_keys, uint32_t stride) {
    uint32_t lo = 0, hi = n_dir;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (directory[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    if (stride == 1 || lo == 0) return lo;
    uint64_t a = dir_source(lo - 1, stride) + 1, b = dir_source(lo - 1, stride) + stride;
    if (b > n_keys) b = n_keys;
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (keys[mid] <= key) a = mid + 1;
        else b = mid;
    }
    return a;
}

// A delta of at most 2^LIVE_SORT_LOG2 rows sorted in LDS: row j's word is its key above its 12-bit position, so distinct words order
// the rows by (key, position) -- the stable order -- under any comparison sort.  The padding word exceeds every row's.
constexpr uint32_t LIVE_SORT_LOG2 = 12;
constexpr uint64_t LIVE_SORT_PAD = ~0ull;
TID_HD uint64_t live_sort_word(uint64_t key, uint32_t j) { return key << LIVE_SORT_LOG2 | uint64_t(j); }
TID_HD uint64_t live_sort_key(uint64_t word) { return word >> LIVE_SORT_LOG2; }
TID_HD uint32_t live_sort_row(uint64_t word) { return uint32_t(word) & ((1u << LIVE_SORT_LOG2) - 1u); }
// one compare-exchange of the bitonic network over `n` (a power of two) words: step (k, j) for pair index t in 0 .. n / 2
TID_HD void live_sort_step(uint64_t *w, uint32_t t, uint32_t k, uint32_t j) {
    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j;
    const bool up = (i & k) == 0;
    const uint64_t a = w[i], b = w[p];
    if ((a > b) == up) {
        w[i] = b;
        w[p] = a;
    }
}

// the word of documents first .. first + 63 of n from the wave's ballot (first < n, a multiple of 64)
TID_HD uint64_t match_word(uint64_t ballot, uint64_t first, uint64_t n, uint64_t invert_mask) {
    const uint64_t left = n - first;
    const uint64_t valid = left >= 64 ? ~0ull : (1ull << left) - 1ull;
    return (ballot ^ invert_mask) & valid;
}

TID_HD uint32_t popcount64(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return uint32_t(__popcll(w));
#else
    return uint32_t(__builtin_popcountll(w));
#endif
}
TID_HD uint32_t new_bits(uint64_t old_word, uint64_t word) { return popcount64(word & ~old_word); }

}  // namespace tid
}  // namespace vbm25

#endif
