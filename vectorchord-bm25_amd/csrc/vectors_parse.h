// vectors_parse.h -- the vectors tape (the growing segment) of a bm25 index relation in the reference's on-disk format: per-tuple
// and per-element functions shared by the device reader's kernels (csrc/pages_device.hip: one call per lane) and by the CPU harness
// that runs them under AddressSanitizer (tests/native/fuzz_vectors_device.cpp: one call per loop iteration).  The accept / refuse
// contract is the host reader's (vbm25_growing_from_pages, csrc/pages.cpp) followed by vbm25_growing_upload's check of the CSR.
// Same rules as pages_parse.h: no HIP include, nothing allocates, throws or touches an atomic; a value read from a page is
// range-checked before it indexes anything; what the host pass validated (the pages' tuple counts and their prefix) is trusted,
// and so is the call's own scratch.
//
// VectorTuple (tuples.rs; insert.rs writes a document as _2, any number of _1, _0):
//   tag 2 (16 bytes)    u64 tag, fieldnorm at 8: starts a document
//   tag 1 (>= 16)       u64 tag, elements_s / elements_e at 8 / 10: a continuation
//   tag 0 (>= 24)       u64 tag, deleted at 8, payload at 10, elements_s / elements_e at 16 / 18: ends the document
//   element (20 bytes)  key[16], tf
// The reader of search.rs:83-135 is a state machine over the tuples in tape order; here it is three scans (the caller's):
//   t_sum   inclusive sum of (tag == 2) << 32 | (tag == 0): the tuple's attempt number and the documents ended up to it
//   t_last  exclusive maximum of (g + 1) << 1 | (tag == 2) over the tuples of tag 2 and 0: bit 0 says the tuple is open (the last
//           _2 / _0 in front of it is a _2)
//   t_eoff  exclusive sum of the kept tuples' element counts
// An attempt (a _2 and what follows it up to the next _2) is kept when an open _0 finished it; a _2 followed by another _2 or by
// the end of the tape is an insert that did not finish: its tuples are validated and contribute nothing.
#ifndef VBM25_VECTORS_PARSE_H
#define VBM25_VECTORS_PARSE_H

#include "pages_parse.h"

namespace vbm25 {
namespace pgs {

// Reasons of a vectors tape, in the order the host reader meets them inside one tuple (1..3 are pages_parse.h's line pointer and
// length reasons).  V_KEYS is what vbm25_growing_upload refuses on the CSR; its position is the document.
enum VReason : uint32_t { V_TAG = 4, V_CONT, V_END, V_RANGE, V_KEYS = R_DESC };
PGS_HD inline const char *vreason_text(uint32_t r) {
    switch (r) {
    case R_TUPLE_SHORT: return "vector tuple too short";
    case V_TAG: return "vector tuple tag";
    case V_CONT: return "vector continuation without a start";
    case V_END: return "vector end without a start";
    case V_RANGE: return "vector tuple element range";
    default: return reason_text(r);
    }
}

constexpr uint32_t ELEMENT = 20, TAG_BAD = 3;

struct VecPlanes {
    TapeView tape;
    // scratch, per tuple of the tape
    uint32_t *t_meta;                   // tag (TAG_BAD: not a vector tuple) | byte 8 (fieldnorm / deleted) << 8 | page offset of the first element << 16
    uint32_t *t_cnt;                    // elements
    unsigned long long *t_mark;         // the input of t_last
    const unsigned long long *t_sum;    // see above
    const unsigned long long *t_last;
    uint8_t *finished;                  // n_tuples + 1, zeroed by the caller: attempt a was ended by an open _0
    uint32_t *t_kept;                   // n_tuples + 1, the last one stays 0: elements the tuple gives to the CSR
    const unsigned long long *t_eoff;   // n_tuples + 1
    // the CSR (vbm25_growing_desc's arrays)
    uint32_t n_docs;                    // tuples of tag 0
    unsigned long long n_el;            // t_eoff[n_tuples]
    unsigned long long *start;          // n_docs + 1, start[0] zeroed by the caller
    uint8_t *key;                       // 16 n_el, 16-byte aligned
    uint32_t *tf;
    uint8_t *fieldnorm, *deleted;
    uint16_t *payload;                  // 3 n_docs
};

PGS_HD inline unsigned long long tuple_increment(uint32_t meta) {
    const uint32_t tag = meta & 3u;
    return tag == 2 ? 1ull << 32 : tag == 0 ? 1ull : 0ull;
}

// Tuple (p, i): line pointer, length, tag, element range -> t_meta, t_cnt, t_mark.  A refused tuple is TAG_BAD (or keeps its tag and
// has no elements): the first refusal in tape order is the one reported, what comes after it does not matter.
PGS_HD inline uint32_t classify_lane(const VecPlanes &c, uint32_t p, uint32_t i) {
    const uint8_t *page = tape_page(c.tape, p);
    const size_t g = (size_t)c.tape.pre[p] + i;
    c.t_meta[g] = TAG_BAD;
    c.t_cnt[g] = 0;
    c.t_mark[g] = 0;
    uint32_t off, len;
    if (uint32_t r = line_pointer(page, i, 16, off, len)) return r;
    const uint8_t *t = page + off;
    const uint32_t tag = rd32(t);
    if (rd32(t + 4) != 0 || tag > 2) return V_TAG;
    if (tag == 2) {
        c.t_meta[g] = 2u | (uint32_t)t[8] << 8;
        c.t_mark[g] = (unsigned long long)(g + 1) << 1 | 1u;
        return R_OK;
    }
    if (tag == 0 && len < 24) return V_END;
    const uint32_t hdr = tag == 1 ? 8 : 16;
    const uint32_t s = rd16(t + hdr), e = rd16(t + hdr + 2);
    const bool fine = s <= e && e <= len && (e - s) % ELEMENT == 0;
    // a fine range lies inside the tuple and the tuple inside the page: off + s <= 8192, 16 bits hold it
    c.t_meta[g] = tag | (tag == 0 ? (uint32_t)t[8] << 8 : 0u) | (fine ? (off + s) << 16 : 0u);
    if (tag == 0) c.t_mark[g] = (unsigned long long)(g + 1) << 1;
    if (!fine) return V_RANGE;
    c.t_cnt[g] = (e - s) / ELEMENT;
    return R_OK;
}

PGS_HD inline bool tuple_open(const VecPlanes &c, size_t g) { return (c.t_last[g] & 1u) != 0; }
PGS_HD inline unsigned long long tuple_attempt(const VecPlanes &c, size_t g) { return c.t_sum[g] >> 32; }

// Tuple g after the scans t_sum and t_last: a continuation or an end needs an open document; an open _0 finishes its attempt
PGS_HD inline uint32_t resolve_lane(const VecPlanes &c, size_t g) {
    const uint32_t tag = c.t_meta[g] & 3u;
    if (tag == TAG_BAD || tag == 2) return R_OK;
    if (!tuple_open(c, g)) return tag == 1 ? V_CONT : V_END;
    if (tag == 0) c.finished[tuple_attempt(c, g)] = 1;  // (open: the attempt is >= 1; at most n_tuples)
    return R_OK;
}

PGS_HD inline bool tuple_kept(const VecPlanes &c, size_t g) {
    const uint32_t tag = c.t_meta[g] & 3u;
    const unsigned long long a = tuple_attempt(c, g);
    return tag != TAG_BAD && a > 0 && c.finished[a] != 0 && (tag == 2 || tuple_open(c, g));
}
// ... after resolve_lane of every tuple
PGS_HD inline void kept_lane(const VecPlanes &c, size_t g) { c.t_kept[g] = tuple_kept(c, g) ? c.t_cnt[g] : 0u; }

// Tuple (p, i) after the scan t_eoff, on a tape without a refusal: a kept _2 gives its document's fieldnorm, a kept _0 its deleted
// byte, payload and end.  The document is the number of _0 tuples in front.
PGS_HD inline void finish_lane(const VecPlanes &c, uint32_t p, uint32_t i) {
    const size_t g = (size_t)c.tape.pre[p] + i;
    if (!tuple_kept(c, g)) return;
    const uint32_t meta = c.t_meta[g], tag = meta & 3u;
    if (tag == 1) return;
    const uint32_t doc = (uint32_t)c.t_sum[g] - (tag == 0);
    if (doc >= c.n_docs) return;
    if (tag == 2) {
        c.fieldnorm[doc] = (uint8_t)(meta >> 8);
        return;
    }
    const uint8_t *page = tape_page(c.tape, p);
    uint32_t off, len;
    if (line_pointer(page, i, 24, off, len)) return;
    c.deleted[doc] = (uint8_t)(meta >> 8);
    for (uint32_t k = 0; k < 3; ++k) c.payload[3 * (size_t)doc + k] = (uint16_t)rd16(page + off + 10 + 2 * k);
    c.start[doc + 1] = c.t_eoff[g] + c.t_kept[g];
}

// elements page p gives to the CSR
PGS_HD inline uint32_t page_elements(const VecPlanes &c, uint32_t p) {
    return (uint32_t)(c.t_eoff[c.tape.pre[p + 1]] - c.t_eoff[c.tape.pre[p]]);
}
// the j-th of them (j < page_elements): its tuple, its number in the CSR and in the tuple.  false: not there
PGS_HD inline bool locate_element(const VecPlanes &c, uint32_t p, uint32_t j, size_t &g, unsigned long long &el, uint32_t &k) {
    size_t lo = c.tape.pre[p], hi = c.tape.pre[p + 1];
    if (lo == hi) return false;
    el = c.t_eoff[lo] + j;
    while (hi - lo > 1) {  // t_eoff[lo] <= el < t_eoff[hi]
        const size_t mid = lo + (hi - lo) / 2;
        if (c.t_eoff[mid] <= el) lo = mid;
        else hi = mid;
    }
    g = lo;
    if (el - c.t_eoff[g] >= c.t_kept[g] || el >= c.n_el) return false;
    k = (uint32_t)(el - c.t_eoff[g]);
    return true;
}

struct alignas(16) Key128 {
    uint32_t w[4];
};

// The j-th element page p gives: 16 key bytes and the tf into the CSR's planes.  Element addresses are 4-byte aligned in an intact
// page and arbitrary in a damaged one (rd32 takes both).
PGS_HD inline void copy_element_lane(const VecPlanes &c, uint32_t p, uint32_t j) {
    size_t g;
    unsigned long long el;
    uint32_t k;
    if (!locate_element(c, p, j, g, el, k)) return;
    const uint32_t at = (c.t_meta[g] >> 16) + ELEMENT * k;
    if (at + ELEMENT > BLCKSZ) return;
    const uint8_t *src = tape_page(c.tape, p) + at;
    Key128 key;
    for (uint32_t q = 0; q < 4; ++q) key.w[q] = rd32(src + 4 * q);
    reinterpret_cast<Key128 *>(c.key)[el] = key;
    c.tf[el] = rd32(src + 16);
}

PGS_HD inline uint64_t key_half_be(const uint8_t *p) {  // 8 key bytes as a number that orders like memcmp (p is 8-byte aligned)
    uint64_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8);
    return __builtin_bswap64(v);
}

// The j-th element page p gives, after every copy and finish_lane: Document::checked_new's rule (vector.rs:56-61), the keys of a
// document strictly ascending.  Returns V_KEYS and the document, or R_OK.
PGS_HD inline uint32_t check_element_lane(const VecPlanes &c, uint32_t p, uint32_t j, uint32_t &doc) {
    size_t g;
    unsigned long long el;
    uint32_t k;
    if (!locate_element(c, p, j, g, el, k)) return R_OK;
    doc = (uint32_t)c.t_sum[g] - ((c.t_meta[g] & 3u) == 0);
    if (doc >= c.n_docs || el <= c.start[doc]) return R_OK;
    const uint8_t *a = c.key + 16 * (el - 1), *b = c.key + 16 * el;
    const uint64_t a0 = key_half_be(a), b0 = key_half_be(b);
    const bool ascending = a0 != b0 ? a0 < b0 : key_half_be(a + 8) < key_half_be(b + 8);
    return ascending ? R_OK : V_KEYS;
}

// The host pass: Meta -> Jump -> the vectors tape by Opaque.next into w.pid[0] / w.pre[0], with walk_relation's per-page checks;
// "page linked twice" within this tape, as the host reader has it.  No tuple is touched.
// `first`: Jump.ptr_vectors of a Jump tuple the caller has read
template <class Sink>
bool walk_vectors_from(vbm25_read_page_fn fn, void *ctx, Walk &w, uint32_t first, Sink &&sink, int &sink_rc) {
    sink_rc = 0;
    if (first == NONE) return w.fail("no vectors tape", 0);  // search.rs:85
    std::unordered_set<uint32_t> walked;
    return walk_tape_pages(fn, ctx, w, 0, first, walked, sink, sink_rc);
}
template <class Sink>
bool walk_vectors(vbm25_read_page_fn fn, void *ctx, Walk &w, Sink &&sink, int &sink_rc) {
    sink_rc = 0;
    const uint8_t *j = read_meta_jump(fn, ctx, w);
    if (!j) return false;
    return walk_vectors_from(fn, ctx, w, host_rd32(j) /* Jump.ptr_vectors */, sink, sink_rc);
}

}  // namespace pgs
}  // namespace vbm25

#endif
