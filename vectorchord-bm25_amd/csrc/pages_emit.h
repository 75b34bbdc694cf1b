// pages_emit.h -- a sealed segment laid out as the reference's index pages: where every tuple goes, which page id every page gets
// and what every 8-byte word of every page image holds.  The inverse of pages_parse.h.  Shared by the device writer's kernels
// (csrc/pages_write.hip: one call per lane) and by the CPU harness that compares every page with the oracle's writer under
// AddressSanitizer (tests/native/fuzz_pages_write.cpp: one call per loop iteration).
//
// Follows flush.rs:40-158 (tape and allocation order), tape.rs:21-167 (push fails over to a new page; the backward tapes of the
// address trees), tuples.rs (Document, Token, Summary, Block, AddressDocuments, AddressTokens, Jump, Meta) and build.rs:22-71, over
// PostgreSQL's page layout: 24-byte header, 4-byte line pointers upwards, tuples MAXALIGNed downwards from the 8-byte special area
// {next, flags}.  A push fails over exactly when pd_lower + 4 > pd_upper - align8(len): a page takes tuples while the sum of their
// costs align8(len) + 4 stays within ROOM.
//
// No HIP include: PGE_HD is `__host__ __device__` under hipcc and empty under plain g++.  A page image is made of 1024 words of 8
// bytes and every word is written exactly once, zeros included: nothing is read back, no store depends on another one's order.
#ifndef VBM25_PAGES_EMIT_H
#define VBM25_PAGES_EMIT_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vbm25.h"

#if defined(__HIPCC__)
#define PGE_HD __host__ __device__
#else
#define PGE_HD
#endif

namespace vbm25 {
namespace pge {

constexpr uint32_t BLCKSZ = 8192, HDR = 24, NONE = 0xffffffffu, WORDS = BLCKSZ / 8;
constexpr uint32_t TOP = BLCKSZ - 8;   // pd_special: the tuples end here
constexpr uint32_t ROOM = TOP - HDR;   // bytes for line pointers and tuples
constexpr uint32_t CHUNK_PAGES = 1024;  // images are made and travel in chunks of at most this many pages (8 MiB)
constexpr uint32_t COPY_LANES = 16;     // lanes that share one block tuple in the fill
constexpr uint32_t DOC_SIZE = 8, TOKEN_SIZE = 32, SUMMARY_SIZE = 24;
constexpr uint32_t DOCS_PER_PAGE = ROOM / (DOC_SIZE + 4), TOKENS_PER_PAGE = ROOM / (TOKEN_SIZE + 4), SUMMARIES_PER_PAGE = ROOM / (SUMMARY_SIZE + 4);
constexpr uint32_t MAX_BLOCK_COST = 16 + 2 * 512 + 4, MIN_BLOCK_COST = 16 + 8 + 8 + 4;
constexpr uint32_t MAX_BLOCKS_PER_PAGE = ROOM / MIN_BLOCK_COST, MIN_BLOCKS_PER_PAGE = ROOM / MAX_BLOCK_COST;
// AddressDocumentsTuple::fit / AddressTokensTuple::fit on an empty page: ((ROOM - 4) & ~7) - 8 bytes of u32 / of Edge {key, u32}
constexpr uint32_t ADDR_DOCS_WIDTH = (((ROOM - 4) & ~7u) - 8) / 4, ADDR_TOKENS_WIDTH = (((ROOM - 4) & ~7u) - 8) / 20;
static_assert(DOCS_PER_PAGE == 680 && TOKENS_PER_PAGE == 226 && SUMMARIES_PER_PAGE == 291, "tuples per page of the reference's format");
static_assert(ADDR_DOCS_WIDTH == 2036 && ADDR_TOKENS_WIDTH == 407, "entries per address page of the reference's format");
static_assert(MAX_BLOCKS_PER_PAGE == 226 && MIN_BLOCKS_PER_PAGE == 7, "block tuples per page");
enum Tape : uint32_t { T_DOCS = 0, T_TOKENS = 1, T_SUMMARIES = 2, T_BLOCKS = 3, N_TAPES = 4 };

PGE_HD inline uint32_t pages_for(uint32_t tuples, uint32_t per_page) { return tuples ? (tuples - 1) / per_page + 1 : 1; }  // a tape has a page
PGE_HD inline uint64_t ld64(const void *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// Everything the layout and fill functions read.  The planes are vbm25_device_segment's; the rest is scratch of the call.
struct Emit {
    uint32_t n_docs, n_terms, n_blocks;
    uint32_t n_pages[N_TAPES];  // documents, tokens, summaries: arithmetic; blocks: the orbit's length (at least 1)
    const uint8_t *doc_fieldnorm;
    const uint16_t *doc_payload;
    const uint8_t *term_key;  // 16 per token (scratch: the segment keeps the keys on the host)
    const uint8_t *term_wand_fn;
    const uint32_t *term_wand_tf, *term_df, *term_first_block;
    const uint32_t *blk_min, *blk_max, *blk_wand_tf;
    const uint8_t *blk_n, *blk_wand_fn, *blk_meta_doc, *blk_meta_tf;
    const uint32_t *off8;
    const uint8_t *blob;
    const unsigned long long *cost;  // n_blocks + 1: cost[j] = the costs of the block tuples in front of j
    const uint32_t *page_start;      // n_pages[T_BLOCKS] + 1: the first block of every blocks page; the last entry is n_blocks
    uint32_t *tok_pid, *sum_pid, *blk_pid;  // the page id of every page of the three interleaved tapes
    const uint32_t *page_ids;        // the caller's ids in allocation order; NULL: first_page + allocation index
    uint32_t first_page;
};

// ---- the blocks tape: costs, the greedy successor, the page of a block

PGE_HD inline uint32_t body_bytes(uint8_t meta, uint32_t n) { return (meta >> 7) ? (meta & 127u) * n : 16u * (meta & 127u); }
PGE_HD inline uint32_t block_size(uint8_t md, uint8_t mt, uint32_t n) { return 16 + ((body_bytes(md, n) + 7) & ~7u) + ((body_bytes(mt, n) + 7) & ~7u); }
// the cost of a tuple whose metadata is outside the codec's range is clamped: the layout stays inside its pages whatever it reads
PGE_HD inline uint32_t block_cost(const uint8_t *blk_n, const uint8_t *md, const uint8_t *mt, uint32_t j) {
    const uint32_t c = block_size(md[j], mt[j], blk_n[j]) + 4;
    return c > MAX_BLOCK_COST ? MAX_BLOCK_COST : c;
}
// a page that begins with block j (< n) ends in front of block next_start(j): the largest e with cost[e] - cost[j] <= ROOM
PGE_HD inline uint32_t next_start(const unsigned long long *cost, uint32_t n, uint32_t j) {
    uint32_t lo = j + 1, hi = n - j > MAX_BLOCKS_PER_PAGE ? j + MAX_BLOCKS_PER_PAGE : n;  // cost[lo] - cost[j] <= MAX_BLOCK_COST
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (cost[mid] - cost[j] <= ROOM) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// entries of the ascending a[0 .. n) that are <= x
PGE_HD inline uint32_t count_le(const uint32_t *a, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
PGE_HD inline uint32_t page_of_block(const Emit &c, uint32_t j) { return count_le(c.page_start, c.n_pages[T_BLOCKS], j) - 1; }

// ---- page ids.  Allocation order (flush.rs): the documents tape's pages; the first pages of tokens, summaries, blocks; then the
// overflow pages of those three in the order the pushes meet them, i.e. by the key (block index, 0 = the block page that begins with
// it | 1 = the summary page that begins with its summary | 2 = the token page that begins with the token after the term whose last
// block it is).  Each of the three key sequences ascends: a rank is the own index plus two counts.

PGE_HD inline uint32_t page_id_of(const Emit &c, uint32_t alloc) { return c.page_ids ? c.page_ids[alloc] : c.first_page + alloc; }
// overflow block pages p >= 1 with page_start[p] <= x
PGE_HD inline uint32_t blocks_le(const Emit &c, uint32_t x) { return count_le(c.page_start, c.n_pages[T_BLOCKS], x) - 1; }
// overflow summary pages q >= 1 with SUMMARIES_PER_PAGE q <= x (x < n_blocks: below the tape's page count by itself)
PGE_HD inline uint32_t summaries_le(const Emit &, uint32_t x) { return x / SUMMARIES_PER_PAGE; }
// overflow token pages r >= 1 whose push comes after block x: term_first_block[TOKENS_PER_PAGE r + 1] <= x
PGE_HD inline uint32_t tokens_before(const Emit &c, uint32_t x) {
    uint32_t lo = 0, hi = c.n_pages[T_TOKENS] - 1;  // r = lo + 1 ..
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (c.term_first_block[(size_t)TOKENS_PER_PAGE * (mid + 1) + 1] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
PGE_HD inline uint32_t first_alloc(const Emit &c, uint32_t tape) { return tape == T_DOCS ? 0 : c.n_pages[T_DOCS] + tape - 1; }
PGE_HD inline uint32_t overflow_base(const Emit &c) { return c.n_pages[T_DOCS] + 3; }
PGE_HD inline uint32_t block_page_alloc(const Emit &c, uint32_t p) {
    if (p == 0) return first_alloc(c, T_BLOCKS);
    const uint32_t j = c.page_start[p];  // >= 1
    return overflow_base(c) + (p - 1) + summaries_le(c, j - 1) + tokens_before(c, j);
}
PGE_HD inline uint32_t summary_page_alloc(const Emit &c, uint32_t q) {
    if (q == 0) return first_alloc(c, T_SUMMARIES);
    const uint32_t j = SUMMARIES_PER_PAGE * q;
    return overflow_base(c) + (q - 1) + blocks_le(c, j) + tokens_before(c, j);
}
PGE_HD inline uint32_t token_page_alloc(const Emit &c, uint32_t r) {
    if (r == 0) return first_alloc(c, T_TOKENS);
    const uint32_t end = c.term_first_block[(size_t)TOKENS_PER_PAGE * r + 1];  // the page's first token is pushed behind its term's last block
    if (end == 0) return overflow_base(c) + (r - 1);                           // (terms without blocks: not a valid segment)
    return overflow_base(c) + (r - 1) + blocks_le(c, end - 1) + summaries_le(c, end - 1);
}
// unit u of the ids pass: the page ids of blocks page u, summaries page u and tokens page u
PGE_HD inline void page_ids_lane(const Emit &c, uint32_t u) {
    if (u < c.n_pages[T_BLOCKS]) c.blk_pid[u] = page_id_of(c, block_page_alloc(c, u));
    if (u < c.n_pages[T_SUMMARIES]) c.sum_pid[u] = page_id_of(c, summary_page_alloc(c, u));
    if (u < c.n_pages[T_TOKENS]) c.tok_pid[u] = page_id_of(c, token_page_alloc(c, u));
}
PGE_HD inline uint32_t tape_page_id(const Emit &c, uint32_t tape, uint32_t p) {
    return tape == T_DOCS ? page_id_of(c, p) : tape == T_TOKENS ? c.tok_pid[p] : tape == T_SUMMARIES ? c.sum_pid[p] : c.blk_pid[p];
}
PGE_HD inline uint32_t tape_next_id(const Emit &c, uint32_t tape, uint32_t p) { return p + 1 < c.n_pages[tape] ? tape_page_id(c, tape, p + 1) : NONE; }

// ---- page images, word by word

// the header's words 0 .. 2: pd_lsn; pd_checksum, pd_flags, pd_lower, pd_upper; pd_special, pd_pagesize_version, pd_prune_xid
PGE_HD inline uint64_t header_word(uint32_t w, uint32_t n_tuples, uint32_t upper) {
    if (w == 1) return (uint64_t)(HDR + 4 * n_tuples) << 32 | (uint64_t)upper << 48;
    if (w == 2) return (uint64_t)TOP | (uint64_t)(BLCKSZ | 4) << 16;
    return 0;
}
PGE_HD inline uint64_t special_word(uint32_t next) { return next; }  // Opaque {next, flags = 0}
PGE_HD inline uint32_t line_pointer(uint32_t off, uint32_t len) { return off | 1u << 15 /* LP_NORMAL */ | len << 17; }

// word k of the tape's g-th tuple
PGE_HD inline uint64_t doc_word(const Emit &c, uint32_t g, uint32_t) {  // {deleted = 0, fieldnorm, payload[3]}
    const uint16_t *p = c.doc_payload + 3 * (size_t)g;
    return (uint64_t)c.doc_fieldnorm[g] << 8 | (uint64_t)p[0] << 16 | (uint64_t)p[1] << 32 | (uint64_t)p[2] << 48;
}
PGE_HD inline uint64_t token_word(const Emit &c, uint32_t g, uint32_t k) {  // {key[16], pad, wand fieldnorm, first summary (u32, u16), df, wand tf}
    if (k < 2) return ld64(c.term_key + 16 * (size_t)g + 8 * k);
    if (k == 3) return (uint64_t)c.term_df[g] | (uint64_t)c.term_wand_tf[g] << 32;
    const uint32_t s = c.term_first_block[g];
    return (uint64_t)c.term_wand_fn[g] << 8 | (uint64_t)c.sum_pid[s / SUMMARIES_PER_PAGE] << 16 | (uint64_t)(s % SUMMARIES_PER_PAGE + 1) << 48;
}
PGE_HD inline uint64_t summary_word(const Emit &c, uint32_t g, uint32_t k) {  // {min, max, block (u32, u16), postings, wand fieldnorm, wand tf, pad}
    if (k == 0) return (uint64_t)c.blk_min[g] | (uint64_t)c.blk_max[g] << 32;
    if (k == 2) return c.blk_wand_tf[g];
    const uint32_t p = page_of_block(c, g);
    return (uint64_t)c.blk_pid[p] | (uint64_t)(g - c.page_start[p] + 1) << 32 | (uint64_t)c.blk_n[g] << 48 | (uint64_t)c.blk_wand_fn[g] << 56;
}
// BlockTuple {metadata, doc range, tf range, pad; doc bytes, zeros to 8; tf bytes, zeros to 8}: the blob's padding is not copied
PGE_HD inline uint64_t block_word(const Emit &c, uint32_t j, uint32_t u) {
    const uint8_t md = c.blk_meta_doc[j], mt = c.blk_meta_tf[j];
    const uint32_t n = c.blk_n[j], ld = body_bytes(md, n), lt = body_bytes(mt, n), ud = (ld + 7) / 8;
    if (u == 0) return (uint64_t)md | (uint64_t)mt << 8 | (uint64_t)16 << 16 | (uint64_t)(16 + ld) << 32 | (uint64_t)(16 + 8 * ud) << 48;
    if (u == 1) return 16 + 8 * ud + lt;
    const bool doc = u - 2 < ud;
    const uint32_t k = doc ? u - 2 : u - 2 - ud, left = (doc ? ld : lt) - 8 * k;
    const uint64_t v = ld64(c.blob + 8 * ((size_t)c.off8[j] + (doc ? 0 : ud) + k));
    return left >= 8 ? v : v & ((1ull << (8 * left)) - 1);
}

// Word w of page p of the documents, tokens or summaries tape: `per` tuples of `size` bytes a page
template <uint32_t TAPE>
PGE_HD inline uint64_t fixed_page_word(const Emit &c, uint32_t p, uint32_t w) {
    constexpr uint32_t per = TAPE == T_DOCS ? DOCS_PER_PAGE : TAPE == T_TOKENS ? TOKENS_PER_PAGE : SUMMARIES_PER_PAGE;
    constexpr uint32_t size = TAPE == T_DOCS ? DOC_SIZE : TAPE == T_TOKENS ? TOKEN_SIZE : SUMMARY_SIZE, tw = size / 8;
    const uint32_t total = TAPE == T_DOCS ? c.n_docs : TAPE == T_TOKENS ? c.n_terms : c.n_blocks;
    const uint32_t base = p * per, n = total - base < per ? total - base : per, upper = TOP - n * size;
    if (w < 3) return header_word(w, n, upper);
    if (w == WORDS - 1) return special_word(tape_next_id(c, TAPE, p));
    if (w < 3 + (n + 1) / 2) {
        const uint32_t i = 2 * (w - 3);
        return (uint64_t)line_pointer(TOP - (i + 1) * size, size) | (i + 1 < n ? (uint64_t)line_pointer(TOP - (i + 2) * size, size) << 32 : 0);
    }
    if (w < upper / 8) return 0;
    const uint32_t v = WORDS - 2 - w, i = v / tw, k = tw - 1 - v % tw;
    return TAPE == T_DOCS ? doc_word(c, base + i, k) : TAPE == T_TOKENS ? token_word(c, base + i, k) : summary_word(c, base + i, k);
}

// Page p of a tape into `out` (1024 words) by `lanes` lanes, this one being `lane`: word-major everywhere but in the block tuples,
// which groups of COPY_LANES lanes copy tuple by tuple (lanes is then a multiple of COPY_LANES)
template <uint32_t TAPE>
PGE_HD inline void fill_page(const Emit &c, uint32_t p, uint64_t *out, uint32_t lane, uint32_t lanes) {
    if (TAPE != T_BLOCKS) {
        for (uint32_t w = lane; w < WORDS; w += lanes) out[w] = fixed_page_word<TAPE == T_BLOCKS ? T_DOCS : TAPE>(c, p, w);
        return;
    }
    const uint32_t j0 = c.page_start[p], n = c.page_start[p + 1] - j0;
    const unsigned long long base = c.cost[j0];
    // bytes of the page's tuples 0 .. i - 1
    auto used = [&](uint32_t i) { return (uint32_t)(c.cost[j0 + i] - base) - 4 * i; };
    const uint32_t upper = TOP - used(n);
    for (uint32_t w = lane; w < upper / 8; w += lanes) {
        uint64_t v = 0;
        if (w < 3) v = header_word(w, n, upper);
        else if (w < 3 + (n + 1) / 2) {
            const uint32_t i = 2 * (w - 3), e0 = used(i), e1 = used(i + 1);
            v = line_pointer(TOP - e1, e1 - e0);
            if (i + 1 < n) v |= (uint64_t)line_pointer(TOP - used(i + 2), used(i + 2) - e1) << 32;
        }
        out[w] = v;
    }
    if (lane == 0) out[WORDS - 1] = special_word(tape_next_id(c, T_BLOCKS, p));
    for (uint32_t i = lane / COPY_LANES; i < n; i += lanes / COPY_LANES) {
        const uint32_t e0 = used(i), e1 = used(i + 1);
        uint64_t *t = out + (TOP - e1) / 8;
        for (uint32_t u = lane % COPY_LANES; u < (e1 - e0) / 8; u += COPY_LANES) t[u] = block_word(c, j0 + i, u);
    }
}

// ---- what the host does: the counts, the two address trees and the four pages build.rs puts around a flush (all tiny)

// pages of a backward tape (address_documents.rs:26-73, address_tokens.rs:26-60) over m entries: one at create, one after every tuple
inline uint32_t address_pages(uint32_t m, uint32_t width) {
    uint32_t pages = 1;
    while (m > 1) {
        m = (m - 1) / width + 1;
        pages += m;
    }
    return pages;
}
// allocations of flush() once the blocks tape's page count is known
inline uint64_t flush_pages(const uint32_t n_pages[N_TAPES], uint32_t n_docs, uint32_t n_terms) {
    return (uint64_t)n_pages[T_DOCS] + n_pages[T_TOKENS] + n_pages[T_SUMMARIES] + n_pages[T_BLOCKS] +
           address_pages(n_docs ? n_pages[T_DOCS] : 0, ADDR_DOCS_WIDTH) + address_pages(n_terms ? n_pages[T_TOKENS] : 0, ADDR_TOKENS_WIDTH);
}

struct HostPage {
    alignas(8) uint8_t b[BLCKSZ];
    explicit HostPage(uint32_t next) {
        std::memset(b, 0, BLCKSZ);
        put16(12, HDR);
        put16(14, TOP);
        put16(16, TOP);
        put16(18, BLCKSZ | 4);
        std::memcpy(b + TOP, &next, 4);
    }
    void put16(uint32_t at, uint32_t v) {
        const uint16_t x = (uint16_t)v;
        std::memcpy(b + at, &x, 2);
    }
    // the page's only tuple
    void set(const uint8_t *t, uint32_t len) {
        const uint32_t up = TOP - ((len + 7) & ~7u), lp = line_pointer(up, len);
        std::memcpy(b + HDR, &lp, 4);
        std::memcpy(b + up, t, len);
        put16(12, HDR + 4);
        put16(14, up);
    }
};

// One address tree: `entries` of `elem` bytes each (the page id in the last 4), `width` a tuple.  Pages are allocated from
// alloc onwards through id_of(alloc++) and handed to sink(page id, image) (non-zero: stop, returned).  Every level's tuple is
// {u16 start = 8, u16 end, pad; entries; zeros to 8}; the entry that stands for a tuple on the next level is its last entry with the
// tuple's page in it; the tape links backwards and ends on an empty page (free).
template <class IdOf, class Sink>
int address_tree(std::vector<uint8_t> entries, uint32_t elem, uint32_t width, uint32_t &alloc, IdOf &&id_of, Sink &&sink, uint32_t &depth,
                 uint32_t &start, uint32_t &free_page) {
    depth = 0;
    uint32_t head = id_of(alloc++), prev = NONE;
    while (entries.size() > elem) {
        ++depth;
        const size_t m = entries.size() / elem;
        std::vector<uint8_t> up;
        for (size_t i = 0; i < m; i += width) {
            const size_t n = m - i < width ? m - i : width;
            std::vector<uint8_t> t((8 + n * elem + 7) & ~size_t(7), 0);
            const uint16_t s = 8, e = (uint16_t)(8 + n * elem);
            std::memcpy(t.data(), &s, 2);
            std::memcpy(t.data() + 2, &e, 2);
            std::memcpy(t.data() + 8, entries.data() + i * elem, n * elem);
            HostPage pg(prev);
            pg.set(t.data(), (uint32_t)t.size());
            if (int rc = sink(head, pg.b)) return rc;
            up.insert(up.end(), entries.data() + (i + n - 1) * elem, entries.data() + (i + n) * elem);
            std::memcpy(up.data() + up.size() - 4, &head, 4);
            prev = head;
            head = id_of(alloc++);
        }
        entries.swap(up);
    }
    start = NONE;
    if (!entries.empty()) std::memcpy(&start, entries.data() + elem - 4, 4);
    free_page = head;
    HostPage last(prev);
    return sink(head, last.b);
}

// Both trees behind the four tapes and the values of the Jump tuple.  tok_pid: the page id of every tokens page; term_key: host.
template <class IdOf, class Sink>
int address_tapes(const uint32_t n_pages[N_TAPES], uint32_t n_docs, uint32_t n_terms, uint64_t sum_len, const uint8_t *term_key,
                  const uint32_t *tok_pid, uint32_t alloc, IdOf &&id_of, Sink &&sink, vbm25_flushed *f) {
    std::memset(f, 0, sizeof *f);
    f->number_of_documents = n_docs;
    f->sum_of_document_lengths = sum_len;
    f->width_1_documents = (uint16_t)ADDR_DOCS_WIDTH;
    f->width_0_documents = (uint16_t)(n_docs ? (n_docs < DOCS_PER_PAGE ? n_docs : DOCS_PER_PAGE) : 1);
    f->ptr_documents = id_of(0);
    f->ptr_tokens = id_of(n_pages[T_DOCS]);
    f->ptr_summaries = id_of(n_pages[T_DOCS] + 1);
    f->ptr_blocks = id_of(n_pages[T_DOCS] + 2);
    std::vector<uint8_t> e;
    if (n_docs) {
        e.resize(4 * (size_t)n_pages[T_DOCS]);
        for (uint32_t p = 0; p < n_pages[T_DOCS]; ++p) {
            const uint32_t id = id_of(p);
            std::memcpy(e.data() + 4 * (size_t)p, &id, 4);
        }
    }
    if (int rc = address_tree(std::move(e), 4, ADDR_DOCS_WIDTH, alloc, id_of, sink, f->depth_documents, f->start_documents, f->free_documents)) return rc;
    e.clear();
    if (n_terms) {
        e.resize(20 * (size_t)n_pages[T_TOKENS]);
        for (uint32_t r = 0; r < n_pages[T_TOKENS]; ++r) {  // Edge {the page's last key, the page}
            const uint64_t last = (uint64_t)TOKENS_PER_PAGE * (r + 1) < n_terms ? (uint64_t)TOKENS_PER_PAGE * (r + 1) - 1 : n_terms - 1;
            std::memcpy(e.data() + 20 * (size_t)r, term_key + 16 * last, 16);
            std::memcpy(e.data() + 20 * (size_t)r + 16, tok_pid + r, 4);
        }
    }
    return address_tree(std::move(e), 20, ADDR_TOKENS_WIDTH, alloc, id_of, sink, f->depth_tokens, f->start_tokens, f->free_tokens);
}

// build.rs:40-70 around a flush into pages 1 .. n: the empty vectors tape (n + 1), the Jump tuple (n + 2), the lock page (n + 3), Meta
template <class Sink>
int fixed_pages(const vbm25_flushed &f, uint32_t n, double k1, double b, const uint8_t *seed32, Sink &&sink) {
    const uint32_t vectors = n + 1, jump = n + 2, lock = n + 3;
    HostPage pv(NONE), pj(NONE), pl(NONE), pm(NONE);
    uint8_t jt[64] = {0}, mt[72] = {0};
    std::memcpy(jt, &vectors, 4);
    std::memcpy(jt + 4, &f.number_of_documents, 4);
    std::memcpy(jt + 8, &f.sum_of_document_lengths, 8);
    std::memcpy(jt + 16, &f.width_1_documents, 2);
    std::memcpy(jt + 18, &f.width_0_documents, 2);
    const uint32_t tail[10] = {f.depth_documents, f.start_documents, f.free_documents, f.depth_tokens, f.start_tokens,
                               f.free_tokens,     f.ptr_documents,   f.ptr_tokens,     f.ptr_summaries, f.ptr_blocks};
    std::memcpy(jt + 20, tail, 40);
    pj.set(jt, 64);
    const uint64_t version = 1;
    std::memcpy(mt, "vchordbm", 8);
    std::memcpy(mt + 8, &version, 8);
    std::memcpy(mt + 16, &k1, 8);
    std::memcpy(mt + 24, &b, 8);
    std::memcpy(mt + 32, &lock, 4);
    std::memcpy(mt + 36, &jump, 4);
    if (seed32) std::memcpy(mt + 40, seed32, 32);
    pm.set(mt, 72);
    if (int rc = sink(vectors, pv.b)) return rc;
    if (int rc = sink(jump, pj.b)) return rc;
    if (int rc = sink(lock, pl.b)) return rc;
    return sink(0u, pm.b);
}

}  // namespace pge
}  // namespace vbm25

#endif
