// pages_parse.h -- per-tuple parsing and validation of a bm25 index relation in the reference's on-disk format, shared by the
// device reader's kernels (csrc/pages_device.hip: one call per lane) and by the CPU harness that hunts out-of-bounds reads under
// AddressSanitizer (tests/native/fuzz_pages_device.cpp: one call per loop iteration).  The accept / refuse contract is the host
// reader's (csrc/pages.cpp); the tuple layouts are cited there (tuples.rs, tape.rs, storage.rs).
//
// No HIP include: PGS_HD is `__host__ __device__` under hipcc and empty under plain g++.  Nothing here allocates, throws or touches
// an atomic: a lane function writes its outputs at the position its (page, slot) owns and RETURNS a reason (0: fine); the caller
// folds the reasons into the call's one error word (smallest key wins: the first error in walk order).
//
// Safety rule of every function: a value read from a page is range-checked before it indexes anything.  What the host pass
// (walk_relation) has validated -- each page's tuple count, the prefix counts, the tape totals -- is trusted.
#ifndef VBM25_PAGES_PARSE_H
#define VBM25_PAGES_PARSE_H

#include <cstddef>
#include <cstdint>

#include <cstring>
#include <unordered_set>
#include <vector>

#include "../../include/vbm25.h"

#if defined(__HIPCC__)
#define PGS_HD __host__ __device__
#else
#define PGS_HD
#endif

namespace vbm25 {
namespace pgs {

constexpr uint32_t BLCKSZ = 8192, HDR = 24, NONE = 0xffffffffu;
constexpr uint32_t CHUNK_PAGES = 1024;  // page images travel and lie in chunks of at most this many pages (8 MiB)
constexpr uint32_t COPY_LANES = 16;     // lanes that share one block body in the copy
enum Tape : uint32_t { T_DOCS = 0, T_TOKENS = 1, T_SUMMARIES = 2, T_BLOCKS = 3, N_TAPES = 4 };

// Reasons.  1..63: the relation's structure (what pages.cpp throws as Corrupt); 64..: what check_desc (csrc/segment.cpp) refuses on
// the flattened arrays.  Structural reasons outrank the others whatever their position (error_key).
enum Reason : uint32_t {
    R_OK = 0,
    R_LP_FLAGS, R_LP_RANGE, R_TUPLE_SHORT, R_DF_ZERO, R_COVER, R_TOKEN_PTR, R_BLOCK_PTR, R_BLOCK_HDR,
    R_DESC = 64,
    R_DF_BLOCKS = R_DESC, R_BLOCK_N, R_BLOCK_META, R_BLOCK_RANGE, R_DF_SUM,
    N_REASONS
};
PGS_HD inline const char *reason_text(uint32_t r) {
    switch (r) {
    case R_LP_FLAGS: return "line pointer is not LP_NORMAL";
    case R_LP_RANGE: return "line pointer out of range";
    case R_TUPLE_SHORT: return "tuple too short";
    case R_DF_ZERO: return "a token without postings";
    case R_COVER: return "summaries do not cover the tokens";
    case R_TOKEN_PTR: return "a token's first summary is not where its pointer says";
    case R_BLOCK_PTR: return "a summary's block is not where its pointer says";
    case R_BLOCK_HDR: return "block tuple ranges do not match its codec metadata";
    case R_DF_BLOCKS: return "a token's df exceeds the document count";
    case R_BLOCK_N: return "bad posting count of a block";
    case R_BLOCK_META: return "bad codec metadata of a block";
    case R_BLOCK_RANGE: return "document range of a block out of order";
    case R_DF_SUM: return "a token's df differs from the postings of its blocks";
    default: return "unknown";
    }
}

// (class, tape, position in tape order, reason): the smallest key is the first error in walk order, whatever the launch order
constexpr uint64_t NO_ERROR = ~0ull;
PGS_HD inline uint64_t error_key(uint32_t tape, uint64_t pos, uint32_t reason) {
    return (uint64_t)(reason >= R_DESC) << 62 | (uint64_t)tape << 56 | pos << 8 | reason;
}
PGS_HD inline uint32_t key_reason(uint64_t k) { return (uint32_t)(k & 0xff); }
PGS_HD inline uint32_t key_tape(uint64_t k) { return (uint32_t)(k >> 56) & 3u; }
PGS_HD inline uint64_t key_pos(uint64_t k) { return (k >> 8) & 0xffffffffffffull; }

// Little-endian reads at any alignment (a damaged line pointer may point anywhere in the page): one aligned load when the address
// allows it, bytes otherwise
PGS_HD inline uint32_t rd16(const uint8_t *p) {
    if (((uintptr_t)p & 1u) == 0) {
        uint16_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(p, 2), 2);
        return v;
    }
    return (uint32_t)p[0] | (uint32_t)p[1] << 8;
}
PGS_HD inline uint32_t rd32(const uint8_t *p) {
    if (((uintptr_t)p & 3u) == 0) {
        uint32_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
        return v;
    }
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
// n <= 8 bytes at p, zero extended to 8
PGS_HD inline uint64_t rd64_part(const uint8_t *p, uint32_t n) {
    if (n == 8 && ((uintptr_t)p & 7u) == 0) {
        uint64_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8);
        return v;
    }
    uint64_t v = 0;
    for (uint32_t i = 0; i < n; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

// One tape as the device (or the harness) holds it: page images in tape order, in chunks; the relation's page id of every page; the
// exclusive prefix of the pages' tuple counts (n_pages + 1 entries)
struct TapeView {
    const uint8_t *const *chunk;
    const uint32_t *pid;
    const uint32_t *pre;
    uint32_t n_pages, n_tuples;
};
PGS_HD inline const uint8_t *tape_page(const TapeView &t, uint32_t p) {
    return t.chunk[p / CHUNK_PAGES] + (size_t)(p % CHUNK_PAGES) * BLCKSZ;
}
// the page that holds the tape's g-th tuple (g < n_tuples): the last p with pre[p] <= g
PGS_HD inline uint32_t page_of_tuple(const TapeView &t, uint32_t g) {
    uint32_t lo = 0, hi = t.n_pages;  // pre[lo] <= g < pre[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t.pre[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Everything the lane functions read and write.  The planes are vbm25_device_segment's; the rest is scratch of the call.
struct Planes {
    uint32_t n_docs;  // Jump.n_docs (== tape[T_DOCS].n_tuples, checked by the caller)
    TapeView tape[N_TAPES];
    uint8_t *doc_fieldnorm;   // per document
    uint16_t *doc_payload;    // 3 per document
    uint8_t *term_key;        // 16 per token (scratch: the segment keeps the keys on the host)
    uint8_t *term_wand_fn;
    uint32_t *term_wand_tf, *term_df;
    uint32_t *term_first_block;  // n_tokens + 1
    uint32_t *tok_page;          // scratch: TokenTuple's pointer to its first summary
    uint16_t *tok_slot;
    uint32_t *tok_nb;            // scratch: ceil(df / 128)
    const unsigned long long *tok_fb;  // scratch: exclusive prefix of tok_nb in 64 bits (the caller's scan)
    uint32_t *blk_min, *blk_max, *blk_wand_tf;
    uint8_t *blk_n, *blk_wand_fn, *blk_meta_doc, *blk_meta_tf;
    uint32_t *sum_blk_page;      // scratch: SummaryTuple's pointer to its block
    uint16_t *sum_blk_slot;
    uint8_t *blk_head;           // scratch, zeroed by the caller: 1 = the first block of a token
    uint32_t *len8;              // scratch: body length in 8-byte units, n_blocks + 1 entries (the last one stays 0)
    const uint32_t *off8;        // blk_off8: exclusive prefix of len8 (the caller's scan)
    uint8_t *blob;
};

// Line pointer i (0-based; i < the page's tuple count, which the host pass took from a validated header) -> the tuple's offset and
// length, validated as PageView::get does before the offset is used as an address
PGS_HD inline uint32_t line_pointer(const uint8_t *page, uint32_t i, uint32_t min_len, uint32_t &off, uint32_t &len) {
    const uint32_t iid = rd32(page + HDR + 4u * i);
    off = iid & 0x7fff;
    len = iid >> 17;
    if (((iid >> 15) & 3u) != 1u /* LP_NORMAL */) return R_LP_FLAGS;
    if (off < HDR || off + len > BLCKSZ) return R_LP_RANGE;
    if (len < min_len) return R_TUPLE_SHORT;
    return R_OK;
}

// DocumentTuple (>= 8 bytes): fieldnorm at 1, payload at 2; `deleted` is not read
PGS_HD inline uint32_t doc_lane(const Planes &c, uint32_t p, uint32_t i) {
    const uint8_t *page = tape_page(c.tape[T_DOCS], p);
    uint32_t off, len;
    if (uint32_t r = line_pointer(page, i, 8, off, len)) return r;
    const uint8_t *t = page + off;
    const size_t g = (size_t)c.tape[T_DOCS].pre[p] + i;
    c.doc_fieldnorm[g] = t[1];
    for (uint32_t k = 0; k < 3; ++k) c.doc_payload[3 * g + k] = (uint16_t)rd16(t + 2 + 2 * k);
    return R_OK;
}

// DocumentTuple.deleted (byte 0; the reference's Bool: != 0) of slot i of documents-tape page p, with doc_lane's line pointer check:
// what vbm25_sealed_deleted_from_pages reads, per lane (csrc/pages_device.hip: doc_deleted_kernel)
PGS_HD inline uint32_t doc_deleted_lane(const TapeView &docs, uint32_t p, uint32_t i, bool &deleted) {
    const uint8_t *page = tape_page(docs, p);
    uint32_t off, len;
    deleted = false;
    if (uint32_t r = line_pointer(page, i, 8, off, len)) return r;
    deleted = page[off] != 0;
    return R_OK;
}

// The 64 flags of one round of a wave (bit l of m: the document first + l) as the one or two words of the bitmap they fall into:
// lo for word first / 64, hi for the next one (0 when the round is word aligned; a shift by 64 is undefined)
PGS_HD inline void flag_round_words(uint64_t first, uint64_t m, uint64_t &lo, uint64_t &hi) {
    const uint32_t sh = (uint32_t)(first & 63u);
    lo = m << sh;
    hi = sh ? m >> (64u - sh) : 0;
}

// TokenTuple (>= 32 bytes): key at 0, wand fieldnorm at 17, first summary (page at 18, slot at 22), df at 24, wand tf at 28
PGS_HD inline uint32_t token_lane(const Planes &c, uint32_t p, uint32_t i) {
    const uint8_t *page = tape_page(c.tape[T_TOKENS], p);
    uint32_t off, len;
    if (uint32_t r = line_pointer(page, i, 32, off, len)) return r;
    const uint8_t *t = page + off;
    const size_t g = (size_t)c.tape[T_TOKENS].pre[p] + i;
    uint64_t *key = reinterpret_cast<uint64_t *>(c.term_key + 16 * g);  // the plane is 16-byte aligned
    key[0] = rd64_part(t, 8);
    key[1] = rd64_part(t + 8, 8);
    c.term_wand_fn[g] = t[17];
    c.tok_page[g] = rd32(t + 18);
    c.tok_slot[g] = (uint16_t)rd16(t + 22);
    const uint32_t df = rd32(t + 24);
    c.term_df[g] = df;
    c.term_wand_tf[g] = rd32(t + 28);
    c.tok_nb[g] = df / 128u + (df % 128u != 0);
    return R_OK;
}

// SummaryTuple (>= 24 bytes): min / max document at 0 / 4, block (page at 8, slot at 12), postings at 14, wand pair at 15 / 16
PGS_HD inline uint32_t summary_lane(const Planes &c, uint32_t p, uint32_t i) {
    const uint8_t *page = tape_page(c.tape[T_SUMMARIES], p);
    uint32_t off, len;
    if (uint32_t r = line_pointer(page, i, 24, off, len)) return r;
    const uint8_t *t = page + off;
    const size_t g = (size_t)c.tape[T_SUMMARIES].pre[p] + i;
    c.blk_min[g] = rd32(t + 0);
    c.blk_max[g] = rd32(t + 4);
    c.sum_blk_page[g] = rd32(t + 8);
    c.sum_blk_slot[g] = (uint16_t)rd16(t + 12);
    c.blk_n[g] = t[14];
    c.blk_wand_fn[g] = t[15];
    c.blk_wand_tf[g] = rd32(t + 16);
    return R_OK;
}

// Token t against the summaries (after token_lane and summary_lane of every tuple and the scan of tok_nb): its ceil(df / 128)
// summaries lie inside the tape and begin where its pointer says; the last token ends the tape.  Writes term_first_block and the
// head flag of its first block.  Then check_desc's per-term rules.
PGS_HD inline uint32_t term_lane(const Planes &c, uint32_t t) {
    const uint32_t n_tokens = c.tape[T_TOKENS].n_tuples, n_sum = c.tape[T_SUMMARIES].n_tuples;
    const uint32_t df = c.term_df[t], nb = c.tok_nb[t];
    const unsigned long long fb = c.tok_fb[t];
    if (df == 0) return R_DF_ZERO;
    if (fb + nb > n_sum || (t + 1 == n_tokens && fb + nb != n_sum)) return R_COVER;
    const uint32_t first = (uint32_t)fb;
    c.term_first_block[t] = first;
    if (t + 1 == n_tokens) c.term_first_block[n_tokens] = n_sum;
    c.blk_head[first] = 1;
    const TapeView &st = c.tape[T_SUMMARIES];
    const uint32_t sp = page_of_tuple(st, first);
    if (st.pid[sp] != c.tok_page[t] || first - st.pre[sp] + 1u != c.tok_slot[t]) return R_TOKEN_PTR;
    if (df > c.n_docs) return R_DF_BLOCKS;
    // every block but the last holds 128 postings (block_lane refuses the others), so the sum is df iff the last block's count fits
    if (128ull * (nb - 1) + c.blk_n[first + nb - 1] != df) return R_DF_SUM;
    return R_OK;
}

// body lengths of a block from its codec metadata (pages.cpp / check_desc): bit-packed 16 w bytes, byte-packed w n bytes
PGS_HD inline uint32_t body_bytes(uint8_t meta, uint32_t n) { return (meta >> 7) ? (meta & 127u) * n : 16u * (meta & 127u); }

// BlockTuple (>= 16 bytes): metadata at 0 / 1, doc range at 2 / 4, tf range at 6 / 8, body from 16.  Block j is the tape's j-th
// tuple: summary j must point here.  Writes the metadata and the padded body length; then check_desc's per-block rules.
// Needs summary_lane of every tuple, term_lane of every token (blk_head) and as many blocks as summaries (the caller's check).
PGS_HD inline uint32_t block_lane(const Planes &c, uint32_t p, uint32_t i) {
    const TapeView &bt = c.tape[T_BLOCKS];
    const uint8_t *page = tape_page(bt, p);
    const uint32_t j = bt.pre[p] + i;
    c.len8[j] = 0;
    uint32_t off, len;
    if (uint32_t r = line_pointer(page, i, 16, off, len)) return r;
    if (c.sum_blk_page[j] != bt.pid[p] || c.sum_blk_slot[j] != i + 1u) return R_BLOCK_PTR;
    const uint8_t *t = page + off;
    const uint8_t md = t[0], mt = t[1];
    const uint16_t ds = (uint16_t)rd16(t + 2), de = (uint16_t)rd16(t + 4), ts = (uint16_t)rd16(t + 6), te = (uint16_t)rd16(t + 8);
    const uint32_t n = c.blk_n[j];
    const uint32_t ld = body_bytes(md, n), lt = body_bytes(mt, n);
    if (ds != 16 || uint32_t(de - ds) != ld || ts != ((de + 7u) & ~7u) || uint32_t(te - ts) != lt || te > len) return R_BLOCK_HDR;
    c.blk_meta_doc[j] = md;
    c.blk_meta_tf[j] = mt;
    c.len8[j] = (ld + 7) / 8 + (lt + 7) / 8;
    const bool head = c.blk_head[j] != 0, last = j + 1 == bt.n_tuples || c.blk_head[j + 1] != 0;
    if (n < 1 || n > 128 || (!last && n != 128)) return R_BLOCK_N;
    const bool full = n == 128;
    for (int k = 0; k < 2; ++k) {
        const uint8_t mm = k ? mt : md;
        const uint32_t w = mm & 127u;
        if (full ? ((mm >> 7) != 0 || w > 32) : ((mm >> 7) != 1 || w < 1 || w > 4)) return R_BLOCK_META;
    }
    if (c.blk_min[j] > c.blk_max[j] || c.blk_max[j] >= c.n_docs || (!head && j > 0 && c.blk_min[j] <= c.blk_max[j - 1])) return R_BLOCK_RANGE;
    return R_OK;
}

// The body of block (p, i) into the blob: doc-id bytes, zero padding to 8, tf bytes, zero padding to 8.  `sub` of COPY_LANES lanes
// takes every COPY_LANES-th 8-byte unit.  Runs only after every block_lane returned R_OK: the header is valid.
PGS_HD inline void copy_lane(const Planes &c, uint32_t p, uint32_t i, uint32_t sub) {
    const TapeView &bt = c.tape[T_BLOCKS];
    const uint8_t *page = tape_page(bt, p);
    const uint32_t j = bt.pre[p] + i;
    uint32_t off, len;
    if (line_pointer(page, i, 16, off, len)) return;
    const uint8_t *t = page + off;
    const uint32_t de = rd16(t + 4), ts = rd16(t + 6), te = rd16(t + 8);
    if (de < 16 || te < ts || te > len || de > len) return;
    const uint32_t ld = de - 16, lt = te - ts, ud = (ld + 7) / 8, ut = (lt + 7) / 8;
    if (ud + ut != c.off8[j + 1] - c.off8[j]) return;
    uint64_t *out = reinterpret_cast<uint64_t *>(c.blob) + c.off8[j];
    for (uint32_t u = sub; u < ud + ut; u += COPY_LANES) {
        const bool doc = u < ud;
        const uint32_t at = doc ? 8 * u : 8 * (u - ud), total = doc ? ld : lt;
        out[u] = rd64_part(t + (doc ? 16u : ts) + at, total - at < 8 ? total - at : 8);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The host pass, the only sequential part: Meta -> Jump -> the four tapes by Opaque.next.  Per page the header is validated exactly as
// PageView::len() / next() do, "page linked twice" across all tapes, and the image is handed to `sink(tape, index in tape, image)`
// (returns 0, or a status that ends the walk).  No tuple is touched.
// ---------------------------------------------------------------------------------------------------------------------------------
struct Walk {
    double k1 = 0, b = 0;
    uint32_t n_docs = 0;
    uint64_t sum_len = 0;
    std::vector<uint32_t> pid[N_TAPES], pre[N_TAPES];  // pre: n_pages + 1 entries
    const char *what = nullptr;                        // a refusal: text and page id
    uint32_t bad_page = 0;
    bool fail(const char *w, uint32_t page) {
        what = w;
        bad_page = page;
        return false;
    }
};
inline uint32_t host_rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t host_rd32(const uint8_t *p) { return host_rd16(p) | host_rd16(p + 2) << 16; }
// PageView::len(): tuples of the page, -1 when the header is out of range
inline int page_tuples(const uint8_t *page) {
    const uint32_t lower = host_rd16(page + 12), upper = host_rd16(page + 14);
    if (lower < HDR || lower > upper || upper > BLCKSZ) return -1;
    return int((lower - HDR) / 4);
}
// slot 1 of a page (Meta, Jump), as PageView::get(1)
inline const uint8_t *first_tuple(Walk &w, const uint8_t *page, uint32_t id, uint32_t &len) {
    const int n = page_tuples(page);
    if (n < 0) return w.fail("page header out of range", id), nullptr;
    if (n < 1) return w.fail("slot out of range", id), nullptr;
    uint32_t off;
    const uint32_t r = line_pointer(page, 0, 0, off, len);
    if (r) return w.fail(reason_text(r), id), nullptr;
    return page + off;
}

// Meta (page 0, slot 1) and Jump (slot 1 of the page Meta names), as the host reader's read_meta_jump: k1, b, n_docs and sum_len go
// into `w`; returns the Jump tuple (at least 64 bytes), nullptr: refused (w.what / w.bad_page)
inline const uint8_t *read_meta_jump(vbm25_read_page_fn fn, void *ctx, Walk &w) {
    uint32_t len = 0;
    const uint8_t *mp = fn(ctx, 0);
    if (!mp) return w.fail("page cannot be read", 0), nullptr;
    const uint8_t *m = first_tuple(w, mp, 0, len);
    if (!m) return nullptr;
    if (len < 72 || std::memcmp(m, "vchordbm", 8) != 0) return w.fail("bad magic number", 0), nullptr;
    uint64_t version;
    std::memcpy(&version, m + 8, 8);
    if (version != 1) return w.fail("bad version number: REINDEX needed", 0), nullptr;
    std::memcpy(&w.k1, m + 16, 8);
    std::memcpy(&w.b, m + 24, 8);
    const uint32_t ptr_jump = host_rd32(m + 36);
    const uint8_t *jp = fn(ctx, ptr_jump);
    if (!jp) return w.fail("page cannot be read", ptr_jump), nullptr;
    const uint8_t *j = first_tuple(w, jp, ptr_jump, len);
    if (!j) return nullptr;
    if (len < 64) return w.fail("jump tuple too short", ptr_jump), nullptr;
    w.n_docs = host_rd32(j + 4);
    std::memcpy(&w.sum_len, j + 8, 8);
    return j;
}

// One tape from page `first` by Opaque.next into w.pid[t] / w.pre[t]; `walked` holds the pages seen so far.  false: refused
// (w.what / w.bad_page), or the sink's status in `sink_rc`.  special_last: the page whose special area is refused is handed to the
// sink and counted first, as the host readers meet its tuples before they follow its link (the vacuum reader's documents tape)
template <class Sink>
bool walk_tape_pages(vbm25_read_page_fn fn, void *ctx, Walk &w, uint32_t t, uint32_t first, std::unordered_set<uint32_t> &walked, Sink &&sink,
                     int &sink_rc, bool special_last = false) {
    uint64_t tuples = 0;
    w.pre[t].push_back(0);
    for (uint32_t cur = first; cur != NONE;) {
        if (!walked.insert(cur).second) return w.fail("page linked twice", cur);
        const uint8_t *page = fn(ctx, cur);
        if (!page) return w.fail("page cannot be read", cur);
        const int n = page_tuples(page);
        if (n < 0) return w.fail("page header out of range", cur);
        const bool opaque = host_rd16(page + 16) == BLCKSZ - 8;
        if (!opaque && !special_last) return w.fail("special area is not Opaque", cur);
        tuples += (uint32_t)n;
        if (tuples > 0xfffffff0ull || w.pid[t].size() >= 0xfffffff0ull) return w.fail("more than 2^32 tuples on a tape", cur);
        if ((sink_rc = sink(t, (uint32_t)w.pid[t].size(), page)) != 0) return false;
        w.pid[t].push_back(cur);
        w.pre[t].push_back((uint32_t)tuples);
        if (!opaque) return w.fail("special area is not Opaque", cur);
        cur = host_rd32(page + BLCKSZ - 8);
    }
    return true;
}

// false: refused (w.what / w.bad_page), or the sink's status in `sink_rc`
template <class Sink>
bool walk_relation(vbm25_read_page_fn fn, void *ctx, Walk &w, Sink &&sink, int &sink_rc) {
    sink_rc = 0;
    const uint8_t *j = read_meta_jump(fn, ctx, w);
    if (!j) return false;
    const uint32_t first[N_TAPES] = {host_rd32(j + 44), host_rd32(j + 48), host_rd32(j + 52), host_rd32(j + 56)};
    std::unordered_set<uint32_t> walked;
    for (uint32_t t = 0; t < N_TAPES; ++t)
        if (!walk_tape_pages(fn, ctx, w, t, first[t], walked, sink, sink_rc)) return false;
    // the counts the host reader compares while it flattens
    if (w.pre[T_DOCS].back() != w.n_docs) return w.fail("document count differs from the Jump tuple", first[T_DOCS]);
    if (w.pre[T_TOKENS].back() == 0 && w.pre[T_SUMMARIES].back() != 0)
        return w.fail("summaries left over after the last token", first[T_SUMMARIES]);
    if (w.pre[T_BLOCKS].back() != w.pre[T_SUMMARIES].back()) return w.fail("blocks and summaries differ in number", first[T_BLOCKS]);
    return true;
}

// the page id an error key names
inline uint32_t error_page(const Walk &w, uint64_t key) {
    const uint32_t t = key_tape(key);
    const uint64_t pos = key_pos(key);
    if (w.pid[t].empty()) return 0;
    size_t lo = 0, hi = w.pid[t].size();
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (w.pre[t][mid] <= pos) lo = mid;
        else hi = mid;
    }
    return w.pid[t][lo];
}

// What becomes of a relation whose walk and lanes are done (`key`: the smallest error key, NO_ERROR: none; keys_ascending: the host's
// memcmp pass over the downloaded keys): VBM25_OK or the host reader's code, in the host reader's order -- structure, then
// check_desc: an empty index is fine whatever k1 / b, parameters before the arrays
inline int verdict(const Walk &w, uint64_t key, bool keys_ascending, const char *&what) {
    what = nullptr;
    if (key != NO_ERROR && key_reason(key) < R_DESC) return what = reason_text(key_reason(key)), VBM25_ERR_CORRUPT;
    if (!w.n_docs) {
        if (w.pre[T_TOKENS].back() || w.pre[T_SUMMARIES].back()) return what = "terms or blocks without documents", VBM25_ERR_CORRUPT;
        return VBM25_OK;
    }
    if (!(w.k1 >= 1.2 && w.k1 <= 2.0) || !(w.b >= 0.0 && w.b <= 1.0)) return what = "k1 must be in [1.2, 2] and b in [0, 1]", VBM25_ERR_INVALID;
    if (key != NO_ERROR) return what = reason_text(key_reason(key)), VBM25_ERR_CORRUPT;
    if (!keys_ascending) return what = "token keys not strictly ascending", VBM25_ERR_CORRUPT;
    return VBM25_OK;
}
}  // namespace pgs
}  // namespace vbm25

#endif
