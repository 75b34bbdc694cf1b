// cast_lane.h -- the plain C++ pieces of the document cast (cast.hip): cast_tsvector_to_document (src/datatype/tsvector.rs:84-94, its
// dedup at :107-127) for ONE document.  __host__ __device__, and plain C++ as well: the kernels of cast.hip are loops over these, and
// tests/native/fuzz_cast.cpp compiles the same text with g++ under AddressSanitizer against std::sort and a loop.
//
//   key_less / key_equal   memcmp order of two 16-byte keys: the halves as big-endian 64-bit values, unsigned (resolve_lane.h's Key)
//   sat_add / clamp_u32    the saturating u32 sum of equal keys' counts and of a document's length (vector.rs:76-83)
//   head_and_sum, rank_of  the rank-and-merge of one element against its document, through an accessor: the wave kernel hands over
//                          cross-lane reads, merge_document (the sequential form, what the harness runs) plain arrays
//   fieldnorm_of           length_to_fieldnorm (bm25.rs:278-283) by bisection of the 256 lengths
//   doc_class              which of the three sort kernels a document of n lexemes takes
//   pack_step / pack_flush, lane_document, seg_head_and_sum / seg_rank_of, lane_span
//                          several short documents a wave (cast_pack_kernel): the host's plan of runs, the document a lane belongs to
//                          and the rank-and-merge confined to it; tests/native/fuzz_cast_pack.cpp drives them lane by lane
#ifndef VBM25_CAST_LANE_H
#define VBM25_CAST_LANE_H

#include <cstdint>

#include "resolve_lane.h"

namespace vbm25 {
namespace cst {

using rsv::Key;

constexpr uint32_t CAST_WAVE_MAX = 64;     // the wave class: one lane a lexeme
constexpr uint32_t CAST_GROUP_MAX = 2048;  // the workgroup class: 16 + 4 bytes of LDS a lexeme, 40 KiB a workgroup

RSV_HD bool key_less(const Key &a, const Key &b) {
    const uint64_t a0 = __builtin_bswap64(a.x), b0 = __builtin_bswap64(b.x);
    if (a0 != b0) return a0 < b0;
    return __builtin_bswap64(a.y) < __builtin_bswap64(b.y);
}
RSV_HD bool key_equal(const Key &a, const Key &b) { return a.x == b.x && a.y == b.y; }

RSV_HD uint32_t sat_add(uint32_t a, uint32_t b) {
    const uint32_t s = a + b;
    return s < a ? 0xFFFFFFFFu : s;
}
RSV_HD uint32_t clamp_u32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(v); }

// Element i (key ki) against the n elements of its document, at(j, key, count) reading element j.  True when no element in front of
// it has its key (it is the one that stays); sum = the saturating sum of the counts of all elements with its key.
template <class At>
RSV_HD bool head_and_sum(const At &at, uint32_t n, uint32_t i, const Key &ki, uint32_t &sum) {
    bool head = true;
    sum = 0;
    for (uint32_t j = 0; j < n; ++j) {
        Key kj;
        uint32_t cj;
        at(j, kj, cj);
        const bool eq = key_equal(kj, ki);
        if (eq) sum = sat_add(sum, cj);
        head = head && !(eq && j < i);
    }
    return head;
}
// The position of key ki among the document's distinct keys: the number of heads (is_head(j)) with a smaller key.
template <class At, class IsHead>
RSV_HD uint32_t rank_of(const At &at, const IsHead &is_head, uint32_t n, const Key &ki) {
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) {
        Key kj;
        uint32_t cj;
        at(j, kj, cj);
        rank += (is_head(j) && key_less(kj, ki)) ? 1u : 0u;
    }
    return rank;
}

// One document, sequentially: n (key, count) pairs in any order -> the distinct keys ascending with their summed counts in
// out_key / out_tf (room for n), the document's length in *length.  head: n bytes of scratch.  Returns the number of elements.
inline uint32_t merge_document(const Key *key, const uint32_t *count, uint32_t n, Key *out_key, uint32_t *out_tf, uint8_t *head,
                               uint32_t *length) {
    struct At {
        const Key *key;
        const uint32_t *count;
        void operator()(uint32_t j, Key &k, uint32_t &c) const {
            k = key[j];
            c = count[j];
        }
    } at{key, count};
    struct IsHead {
        const uint8_t *head;
        bool operator()(uint32_t j) const { return head[j] != 0; }
    } is_head{head};
    uint32_t kept = 0, len = 0, sum = 0;
    for (uint32_t i = 0; i < n; ++i) head[i] = head_and_sum(at, n, i, key[i], sum) ? 1 : 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!head[i]) continue;
        (void)head_and_sum(at, n, i, key[i], sum);
        const uint32_t r = rank_of(at, is_head, n, key[i]);
        out_key[r] = key[i];
        out_tf[r] = sum;
        len = sat_add(len, sum);
        ++kept;
    }
    *length = len;
    return kept;
}

// length_to_fieldnorm: the last code whose length is <= len (lengths256 ascending, lengths256[0] == 0)
RSV_HD uint8_t fieldnorm_of(const uint32_t *lengths256, uint32_t len) {
    uint32_t lo = 0, hi = 256;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lengths256[mid] <= len) lo = mid; else hi = mid;
    }
    return uint8_t(lo);
}

// The sort a document of n lexemes takes.  wave_max / group_max: the classes' bounds (0: the class is off).
enum DocClass : uint32_t { CLASS_WAVE = 0, CLASS_GROUP = 1, CLASS_GENERAL = 2 };
RSV_HD DocClass doc_class(uint32_t n, uint32_t wave_max, uint32_t group_max) {
    if (wave_max && n <= wave_max) return CLASS_WAVE;
    if (group_max && n <= group_max) return CLASS_GROUP;
    return CLASS_GENERAL;
}

// ---- several short documents a wave (cast_pack_kernel) ----
// The plan: runs of consecutive wave-class documents, packed greedily while a run has at most PACK_LANES lexemes and at most
// PACK_LANES documents.  A run's lexemes are contiguous (doc_lex[first] .. doc_lex[first + count]), so one lane takes one of them.
constexpr uint32_t PACK_LANES = 64;
struct PackEntry {
    uint32_t first, count;  // documents first .. first + count
};
// The run that is open while the host walks the documents in order (count == 0: none is).
struct PackRun {
    uint32_t first = 0, count = 0, lex = 0;
};
// Document d of n lexemes comes next.  True when the open run had to end in front of it -- d is of another class, or would be the run's
// 65th document or take it past 64 lexemes -- and `done` is that run.  A wave-class d then opens, or joins, the run.
RSV_HD bool pack_step(PackRun &r, uint32_t d, uint32_t n, bool wave_class, PackEntry &done) {
    const bool close = r.count && (!wave_class || r.count == PACK_LANES || r.lex + n > PACK_LANES);
    if (close) {
        done = PackEntry{r.first, r.count};
        r.count = r.lex = 0;
    }
    if (wave_class) {
        if (!r.count) r.first = d;
        ++r.count;
        r.lex += n;
    }
    return close;
}
// Behind the last document: true when a run was still open.
RSV_HD bool pack_flush(PackRun &r, PackEntry &done) {
    if (!r.count) return false;
    done = PackEntry{r.first, r.count};
    r.count = r.lex = 0;
    return true;
}

// The document of lane l in a run of cnt documents (1 .. 64): bound(j), j < cnt, is the lane at which document j of the run begins
// (bound(0) == 0, ascending, equal bounds around empty documents).  The last j with bound(j) <= l: the one document that holds lane l
// when l is below the run's lexemes.  Always six steps and bound() in every one, so a wave may answer bound() by a cross-lane read.
template <class Bound>
RSV_HD uint32_t lane_document(const Bound &bound, uint32_t cnt, uint32_t l) {
    uint32_t lo = 0, hi = cnt;
#pragma unroll
    for (int step = 0; step < 6; ++step) {
        const uint32_t mid = lo + ((hi - lo) >> 1);  // (== lo once hi - lo is 1: bound(lo) <= l holds, nothing moves)
        const bool le = bound(mid) <= l;
        if (hi - lo > 1) {
            if (le) lo = mid; else hi = mid;
        }
    }
    return lo;
}

// head_and_sum / rank_of for element i of the document that is elements sb .. se of a run: step t looks at element sb + t of the
// element's OWN document, so a key in two documents of one wave never merges, and a run of short documents takes as many steps as its
// longest document has lexemes (`longest`, the same for every element of the run: every lane of a wave takes every step, and a lane
// whose document has ended reads its own element and ignores it).
template <class At>
RSV_HD bool seg_head_and_sum(const At &at, uint32_t longest, uint32_t i, const Key &ki, uint32_t sb, uint32_t se, uint32_t &sum) {
    bool head = true;
    sum = 0;
    for (uint32_t t = 0; t < longest; ++t) {
        const uint32_t j = sb + t;
        const bool in = j < se;
        Key kj;
        uint32_t cj;
        at(in ? j : i, kj, cj);
        const bool eq = in && key_equal(kj, ki);
        if (eq) sum = sat_add(sum, cj);
        head = head && !(eq && j < i);
    }
    return head;
}
template <class At, class IsHead>
RSV_HD uint32_t seg_rank_of(const At &at, const IsHead &is_head, uint32_t longest, uint32_t i, const Key &ki, uint32_t sb, uint32_t se) {
    uint32_t rank = 0;
    for (uint32_t t = 0; t < longest; ++t) {
        const uint32_t j = sb + t;
        const bool in = j < se;
        Key kj;
        uint32_t cj;
        at(in ? j : i, kj, cj);
        rank += (in && is_head(j) && key_less(kj, ki)) ? 1u : 0u;
    }
    return rank;
}
// bits a .. b - 1 of a wave's ballot (a <= b <= 64): the heads of the document that is lanes a .. b
RSV_HD uint64_t lane_span(uint32_t a, uint32_t b) {
    const uint64_t below_b = b >= 64 ? ~0ull : (1ull << b) - 1ull, below_a = a >= 64 ? ~0ull : (1ull << a) - 1ull;
    return below_b & ~below_a;
}

}  // namespace cst
}  // namespace vbm25

#endif
