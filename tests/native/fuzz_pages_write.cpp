// AddressSanitizer harness for the device writer's layout and fill functions (vectorchord-bm25_amd/csrc/pages_emit.h, compiled here
// by plain g++): the passes of csrc/pages_write.hip as plain loops over the kernels' grids, one loop iteration per thread or lane, in
// the kernels' order, with every buffer sized exactly as the device allocates it (prefix sums, jump tables, page starts, page ids, one
// chunk of CHUNK_PAGES images).  Every page of the relation must equal the page the oracle's writer (oracle/pages.cpp:
// orc_pages_build) makes of the same index, without any out-of-bounds access.  Built and run by tests/test_pages_write_host.py.
//
// argv[1] (optional): a case file written by the test -- u32 n_relations, per relation u32 n_pages and the oracle's page images -- each
// read by the host reader (vbm25_segment_from_pages) and written again; run before the 2000 random segments.
// argv[2] (optional): "only" -- the case file and nothing else.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/vbm25.h"
#include "../../oracle/oracle.h"
#include "../../vectorchord-bm25_amd/csrc/pages_emit.h"

namespace vbm25 {
int set_error(int code, const char *, ...) { return code; }  // the library defines it in error.cpp
}

using namespace vbm25::pge;

template <class T>
static std::unique_ptr<T[]> exact(size_t n) {  // n elements and not one more: AddressSanitizer sees the first byte past them
    return std::unique_ptr<T[]>(new T[n]());
}
template <class T>
static std::unique_ptr<T[]> exact_copy(const T *src, size_t n) {  // the segment's planes, sized as the device segment sizes them
    auto p = exact<T>(n);
    if (n) std::memcpy(p.get(), src, n * sizeof(T));
    return p;
}

typedef std::vector<std::vector<uint8_t>> PageList;

// the device writer's write_relation with loops for kernels
static PageList write_like_the_device(const orc_index_view &v, const uint8_t *seed32) {
    const uint32_t n = v.n_blocks;
    auto doc_fieldnorm = exact_copy(v.doc_fieldnorm, v.n_docs);
    auto doc_payload = exact_copy(v.doc_payload, 3ull * v.n_docs);
    auto term_key = exact_copy(v.term_key, 16ull * v.n_terms);
    auto term_wand_fn = exact_copy(v.term_wand_fn, v.n_terms);
    auto term_wand_tf = exact_copy(v.term_wand_tf, v.n_terms), term_df = exact_copy(v.term_df, v.n_terms);
    auto tfb = exact<uint32_t>(v.n_terms + 1ull);
    if (v.n_terms) std::memcpy(tfb.get(), v.term_first_block, 4ull * (v.n_terms + 1ull));
    auto blk_min = exact_copy(v.blk_min_doc, n), blk_max = exact_copy(v.blk_max_doc, n), blk_wand_tf = exact_copy(v.blk_wand_tf, n);
    auto blk_n = exact_copy(v.blk_n, n), blk_wand_fn = exact_copy(v.blk_wand_fn, n), blk_md = exact_copy(v.blk_meta_doc, n), blk_mt = exact_copy(v.blk_meta_tf, n);
    auto off8 = exact<uint32_t>(n + 1ull);
    if (n) std::memcpy(off8.get(), v.blk_off8, 4ull * (n + 1ull));
    auto blob = exact_copy(v.blob, (size_t)v.blob_bytes);

    Emit c{};
    c.n_docs = v.n_docs;
    c.n_terms = v.n_terms;
    c.n_blocks = n;
    c.n_pages[T_DOCS] = pages_for(v.n_docs, DOCS_PER_PAGE);
    c.n_pages[T_TOKENS] = pages_for(v.n_terms, TOKENS_PER_PAGE);
    c.n_pages[T_SUMMARIES] = pages_for(n, SUMMARIES_PER_PAGE);
    c.n_pages[T_BLOCKS] = 1;
    c.doc_fieldnorm = doc_fieldnorm.get();
    c.doc_payload = doc_payload.get();
    c.term_key = term_key.get();
    c.term_wand_fn = term_wand_fn.get();
    c.term_wand_tf = term_wand_tf.get();
    c.term_df = term_df.get();
    c.term_first_block = tfb.get();
    c.blk_min = blk_min.get();
    c.blk_max = blk_max.get();
    c.blk_wand_tf = blk_wand_tf.get();
    c.blk_n = blk_n.get();
    c.blk_wand_fn = blk_wand_fn.get();
    c.blk_meta_doc = blk_md.get();
    c.blk_meta_tf = blk_mt.get();
    c.off8 = off8.get();
    c.blob = blob.get();

    // ---- the layout: scan, next_kernel, double_kernel's rounds, count_kernel
    const uint32_t cap = n / MIN_BLOCKS_PER_PAGE + 2;
    auto cost = exact<unsigned long long>(n + 1ull);
    auto page_start = exact<uint32_t>(cap);
    if (n) {
        for (uint32_t j = 0; j < n; ++j) cost[j + 1] = cost[j] + block_cost(c.blk_n, c.blk_meta_doc, c.blk_meta_tf, j);
        std::unique_ptr<uint32_t[]> jump[2] = {exact<uint32_t>(n + 1ull), exact<uint32_t>(n + 1ull)};
        for (uint32_t j = 0; j <= n; ++j) jump[0][j] = j < n ? next_start(cost.get(), n, j) : n;
        int cur = 0;
        for (uint64_t have = 1; have < cap; have *= 2, cur ^= 1) {
            const bool last = 2 * have >= cap;
            for (uint32_t t = 0; t < std::max<uint64_t>(n + 1ull, have); ++t) {
                if (t < have && t + have < cap) page_start[t + have] = jump[cur][page_start[t]];
                if (t <= n && !last) jump[cur ^ 1][t] = jump[cur][jump[cur][t]];
            }
        }
        uint32_t b = 0;
        for (uint32_t k = 0; k + 1 < cap; ++k)
            if (page_start[k] < n && page_start[k + 1] >= n) b = k + 1;
        if (!b) return {};
        c.n_pages[T_BLOCKS] = b;
    }
    c.cost = cost.get();
    c.page_start = page_start.get();
    const uint32_t total = (uint32_t)flush_pages(c.n_pages, v.n_docs, v.n_terms);
    c.first_page = 1;

    // ---- ids_kernel
    auto tok_pid = exact<uint32_t>(c.n_pages[T_TOKENS]), sum_pid = exact<uint32_t>(c.n_pages[T_SUMMARIES]), blk_pid = exact<uint32_t>(c.n_pages[T_BLOCKS]);
    c.tok_pid = tok_pid.get();
    c.sum_pid = sum_pid.get();
    c.blk_pid = blk_pid.get();
    for (uint32_t u = 0; u < std::max(c.n_pages[T_BLOCKS], std::max(c.n_pages[T_SUMMARIES], c.n_pages[T_TOKENS])); ++u) page_ids_lane(c, u);

    // ---- fill_kernel, a chunk at a time
    PageList out(total + 4ull);
    uint64_t delivered = 0;
    auto sink = [&](uint32_t id, const uint8_t *image) {
        if (id >= out.size() || !out[id].empty()) return 1;
        out[id].assign(image, image + BLCKSZ);
        ++delivered;
        return 0;
    };
    for (uint32_t tape = 0; tape < N_TAPES; ++tape)
        for (uint32_t p0 = 0; p0 < c.n_pages[tape]; p0 += CHUNK_PAGES) {
            const uint32_t np = std::min(CHUNK_PAGES, c.n_pages[tape] - p0);
            auto img = exact<uint64_t>((size_t)np * WORDS);  // (the device keeps CHUNK_PAGES images and uses the first np)
            auto pid = exact<uint32_t>(np);
            std::memset(img.get(), 0xa5, (size_t)np * BLCKSZ);  // a word that is not written shows
            for (uint32_t i = 0; i < np; ++i)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    uint64_t *o = img.get() + (size_t)i * WORDS;
                    if (tape == T_DOCS) fill_page<T_DOCS>(c, p0 + i, o, lane, 64);
                    else if (tape == T_TOKENS) fill_page<T_TOKENS>(c, p0 + i, o, lane, 64);
                    else if (tape == T_SUMMARIES) fill_page<T_SUMMARIES>(c, p0 + i, o, lane, 64);
                    else fill_page<T_BLOCKS>(c, p0 + i, o, lane, 64);
                    if (lane == 0) pid[i] = tape_page_id(c, tape, p0 + i);
                }
            for (uint32_t i = 0; i < np; ++i)
                if (sink(pid[i], reinterpret_cast<const uint8_t *>(img.get() + (size_t)i * WORDS))) return {};
        }
    // ---- the host's share
    auto id_of = [&](uint32_t alloc) { return 1 + alloc; };
    const uint32_t alloc = c.n_pages[T_DOCS] + c.n_pages[T_TOKENS] + c.n_pages[T_SUMMARIES] + c.n_pages[T_BLOCKS];
    vbm25_flushed f;
    if (address_tapes(c.n_pages, v.n_docs, v.n_terms, v.sum_len, v.term_key, tok_pid.get(), alloc, id_of, sink, &f)) return {};
    if (delivered != total) return {};
    if (fixed_pages(f, total, v.k1, v.b, seed32, sink)) return {};
    return out;
}

static bool compare(const PageList &got, const PageList &want, const char *what, long which) {
    if (got.size() != want.size()) return std::printf("%s %ld: %zu pages written, the oracle's relation has %zu\n", what, which, got.size(), want.size()), false;
    for (size_t p = 0; p < want.size(); ++p)
        if (got[p].size() != BLCKSZ || std::memcmp(got[p].data(), want[p].data(), BLCKSZ) != 0) {
            size_t at = 0;
            while (got[p].size() == BLCKSZ && got[p][at] == want[p][at]) ++at;
            return std::printf("%s %ld: page %zu differs from the oracle's at byte %zu\n", what, which, p, at), false;
        }
    return true;
}

struct Rel {
    PageList pages;
};
static const uint8_t *read_page(void *ctx, uint32_t id) {
    auto *r = static_cast<Rel *>(ctx);
    return id < r->pages.size() ? r->pages[id].data() : nullptr;
}

static bool run_case_file(const char *path) {
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return std::printf("cannot open %s\n", path), false;
    auto u32 = [&] {
        uint32_t v = 0;
        if (std::fread(&v, 4, 1, fp) != 1) v = 0;
        return v;
    };
    const uint32_t n_rel = u32();
    for (uint32_t it = 0; it < n_rel; ++it) {
        Rel r;
        for (uint32_t i = u32(); i; --i) {
            r.pages.emplace_back(BLCKSZ);
            if (std::fread(r.pages.back().data(), BLCKSZ, 1, fp) != 1) return std::fclose(fp), false;
        }
        vbm25_segment *seg = nullptr;
        uint8_t seed[32];
        if (vbm25_segment_from_pages(read_page, &r, &seg) != VBM25_OK || vbm25_pages_seed(read_page, &r, seed) != VBM25_OK)
            return std::printf("relation %u of the file is refused by the host reader\n", it), std::fclose(fp), false;
        vbm25_index_desc d;
        vbm25_segment_desc(seg, &d);
        orc_index_view v{};
        v.n_docs = d.n_docs, v.n_terms = d.n_terms, v.n_blocks = d.n_blocks, v.sum_len = d.sum_len, v.blob_bytes = d.blob_bytes, v.k1 = d.k1, v.b = d.b;
        v.term_key = d.term_key, v.term_df = d.term_df, v.term_wand_fn = d.term_wand_fn, v.term_wand_tf = d.term_wand_tf;
        v.term_first_block = d.term_first_block, v.blk_min_doc = d.blk_min_doc, v.blk_max_doc = d.blk_max_doc, v.blk_n = d.blk_n;
        v.blk_wand_fn = d.blk_wand_fn, v.blk_wand_tf = d.blk_wand_tf, v.blk_meta_doc = d.blk_meta_doc, v.blk_meta_tf = d.blk_meta_tf;
        v.blk_off8 = d.blk_off8, v.blob = d.blob, v.doc_fieldnorm = d.doc_fieldnorm, v.doc_payload = d.doc_payload;
        const bool ok = compare(write_like_the_device(v, seed), r.pages, "relation", it);
        vbm25_segment_free(seg);
        if (!ok) return std::fclose(fp), false;
    }
    std::fclose(fp);
    std::printf("case file done: %u relations rewritten\n", n_rel);
    return true;
}

int main(int argc, char **argv) {
    if (argc > 1 && !run_case_file(argv[1])) return 1;
    if (argc > 2) return std::strcmp(argv[2], "only") == 0 ? 0 : (std::printf("unknown argument %s\n", argv[2]), 1);
    // 2000 random segments: 1 .. 3000 documents, 1 .. 600 terms, df 1 .. 400; most of them small, the ranges' ends among them
    std::mt19937_64 rng(11);
    uint64_t pages = 0, multi_block_pages = 0;
    for (int it = 0; it < 2000; ++it) {
        const uint32_t n_docs = it == 0 ? 3000 : it == 1 ? 1 : 1 + rng() % 3000;
        const uint32_t n_terms = it == 0 ? 600 : it == 1 ? 1 : 1 + (rng() % 600 >> rng() % 5);
        const uint32_t df_cap = it == 0 ? 400 : std::min<uint32_t>(n_docs, 1 + (rng() % 400 >> rng() % 5));
        std::vector<uint32_t> doc_len(n_docs, 0), post_doc, post_tf;
        std::vector<uint16_t> payload(3ull * n_docs);
        for (auto &x : payload) x = uint16_t(rng());
        std::vector<uint64_t> term_start{0};
        std::vector<uint8_t> keys(16ull * n_terms, 0);
        const uint32_t gap_bits = rng() % 3, tf_bits = 1 + rng() % 20;
        for (uint32_t t = 0; t < n_terms; ++t) {
            std::snprintf(reinterpret_cast<char *>(&keys[16ull * t]), 16, "k%05u", t);
            const uint32_t df = it == 0 ? 400 - t % 3 : 1 + rng() % df_cap;
            // df ascending documents: a random start, then steps that leave room for the rest
            uint32_t d = 0, left = n_docs;
            for (uint32_t i = 0; i < df; ++i) {
                const uint32_t room = left - (df - i);  // documents that may be skipped
                const uint32_t skip = room ? rng() % (std::min<uint32_t>(room, (1u << (4 * gap_bits)) + 2) + 1) : 0;
                d += skip;
                left -= skip + 1;
                post_doc.push_back(d++);
                post_tf.push_back(1 + uint32_t(rng() % (1ull << tf_bits)) % (rng() % 4 ? 4 : 1u << tf_bits));
                doc_len[post_doc.back()] += post_tf.back();
            }
            term_start.push_back(post_doc.size());
        }
        for (auto &l : doc_len) l = l ? l : 1;
        orc_index *ix = orc_index_build(1.2 + (it % 5) * 0.2, (it % 3) * 0.5, n_docs, doc_len.data(), payload.data(), n_terms, keys.data(),
                                        term_start.data(), post_doc.data(), post_tf.data());
        uint8_t seed[32];
        for (auto &x : seed) x = uint8_t(rng());
        orc_pages *op = orc_pages_build(ix, it % 2 ? seed : nullptr);
        PageList want;
        for (uint32_t i = 0; i < orc_pages_count(op); ++i) want.emplace_back(orc_pages_get(op, i), orc_pages_get(op, i) + BLCKSZ);
        orc_index_view v;
        orc_index_get_view(ix, &v);
        const bool ok = compare(write_like_the_device(v, it % 2 ? seed : nullptr), want, "random segment", it);
        pages += want.size();
        multi_block_pages += v.n_blocks > MAX_BLOCKS_PER_PAGE;
        orc_pages_free(op);
        orc_index_free(ix);
        if (!ok) return 1;
    }
    std::printf("fuzz done: 2000 segments, %llu pages equal to the oracle's, %llu segments with more than one blocks page\n",
                (unsigned long long)pages, (unsigned long long)multi_block_pages);
    return multi_block_pages > 100 ? 0 : 1;
}
