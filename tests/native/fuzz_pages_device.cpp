// AddressSanitizer harness for the device reader's per-tuple functions (vectorchord-bm25_amd/csrc/pages_parse.h, compiled here
// by plain g++): the host pass and then the same (page, slot) grid the kernels of csrc/pages_device.hip run, one loop iteration per
// lane, in the kernels' order, with every array sized exactly as the device allocates it (page images per chunk, planes per tuple
// count).  A relation must be accepted or refused exactly as vbm25_segment_from_pages does, with equal arrays when accepted, and
// without any out-of-bounds access.  Built and run by tests/test_pages_device_host.py.
//
// argv[1] (optional): a case file written by the test -- u32 n_pages, the page images, u32 n_cases, per case u32 n_edits and n_edits x
// (u32 page, u32 position, u32 byte) -- run before the 4000 damaged relations of tests/native/fuzz_pages.cpp's generator.
// argv[2] (optional): "only" -- the case file and nothing else (a relation of several chunks of CHUNK_PAGES pages takes seconds per
// case under AddressSanitizer).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/vbm25.h"
#include "../../oracle/oracle.h"
#include "../../vectorchord-bm25_amd/csrc/pages_parse.h"

namespace vbm25 {
int set_error(int code, const char *, ...) { return code; }  // the library defines it in error.cpp
}

using namespace vbm25::pgs;

struct Rel {
    std::vector<std::vector<uint8_t>> pages;
};
static const uint8_t *read_page(void *ctx, uint32_t id) {
    auto *r = static_cast<Rel *>(ctx);
    return id < r->pages.size() ? r->pages[id].data() : nullptr;
}

template <class T>
static std::unique_ptr<T[]> exact(size_t n) {  // n elements and not one more: AddressSanitizer sees the first byte past them
    return std::unique_ptr<T[]>(new T[n]());
}

struct Flat {
    uint32_t n_docs = 0, n_terms = 0, n_blocks = 0;
    uint64_t sum_len = 0, blob_bytes = 0;
    double k1 = 0, b = 0;
    std::unique_ptr<uint8_t[]> doc_fieldnorm, term_key, term_wand_fn, blk_n, blk_wand_fn, blk_meta_doc, blk_meta_tf, blob;
    std::unique_ptr<uint16_t[]> doc_payload;
    std::unique_ptr<uint32_t[]> term_wand_tf, term_df, term_first_block, blk_min, blk_max, blk_wand_tf, blk_off8;
};

// the device reader with loops for kernels; returns VBM25_OK or the refusal's code
static int read_like_the_device(vbm25_read_page_fn fn, void *ctx, Flat &f) {
    Walk w;
    std::vector<std::unique_ptr<uint8_t[]>> chunks[N_TAPES];
    std::vector<uint8_t> staging;  // one chunk being filled
    uint32_t staged_tape = 0;
    auto flush = [&] {
        if (staging.empty()) return;
        auto d = exact<uint8_t>(staging.size());
        std::memcpy(d.get(), staging.data(), staging.size());
        chunks[staged_tape].push_back(std::move(d));
        staging.clear();
    };
    int sink_rc = 0;
    const bool walked = walk_relation(fn, ctx, w, [&](uint32_t tape, uint32_t, const uint8_t *image) {
        if (tape != staged_tape || staging.size() == size_t(CHUNK_PAGES) * BLCKSZ) {
            flush();
            staged_tape = tape;
        }
        staging.insert(staging.end(), image, image + BLCKSZ);
        return 0;
    }, sink_rc);
    if (!walked) return VBM25_ERR_CORRUPT;
    flush();
    const uint32_t n_docs = w.n_docs, n_tok = w.pre[T_TOKENS].back(), n_sum = w.pre[T_SUMMARIES].back();

    std::vector<const uint8_t *> chunk_ptr[N_TAPES];
    std::unique_ptr<uint32_t[]> pid[N_TAPES], pre[N_TAPES];
    Planes c{};
    c.n_docs = n_docs;
    for (uint32_t t = 0; t < N_TAPES; ++t) {
        const size_t np = w.pid[t].size();
        for (const auto &d : chunks[t]) chunk_ptr[t].push_back(d.get());
        pid[t] = exact<uint32_t>(np);
        pre[t] = exact<uint32_t>(np + 1);
        std::copy(w.pid[t].begin(), w.pid[t].end(), pid[t].get());
        std::copy(w.pre[t].begin(), w.pre[t].end(), pre[t].get());
        c.tape[t] = TapeView{chunk_ptr[t].data(), pid[t].get(), pre[t].get(), uint32_t(np), w.pre[t].back()};
    }
    f.n_docs = n_docs;
    f.n_terms = n_tok;
    f.n_blocks = n_sum;
    f.sum_len = w.sum_len;
    f.k1 = w.k1;
    f.b = w.b;
    f.doc_fieldnorm = exact<uint8_t>(n_docs);
    f.doc_payload = exact<uint16_t>(3ull * n_docs);
    f.term_key = exact<uint8_t>(16ull * n_tok);
    f.term_wand_fn = exact<uint8_t>(n_tok);
    f.term_wand_tf = exact<uint32_t>(n_tok);
    f.term_df = exact<uint32_t>(n_tok);
    f.term_first_block = exact<uint32_t>(n_tok + 1ull);
    f.blk_min = exact<uint32_t>(n_sum);
    f.blk_max = exact<uint32_t>(n_sum);
    f.blk_wand_tf = exact<uint32_t>(n_sum);
    f.blk_n = exact<uint8_t>(n_sum);
    f.blk_wand_fn = exact<uint8_t>(n_sum);
    f.blk_meta_doc = exact<uint8_t>(n_sum);
    f.blk_meta_tf = exact<uint8_t>(n_sum);
    f.blk_off8 = exact<uint32_t>(n_sum + 1ull);
    auto tok_page = exact<uint32_t>(n_tok), tok_nb = exact<uint32_t>(n_tok), sum_page = exact<uint32_t>(n_sum), len8 = exact<uint32_t>(n_sum + 1ull);
    auto tok_slot = exact<uint16_t>(n_tok), sum_slot = exact<uint16_t>(n_sum);
    auto tok_fb = exact<unsigned long long>(n_tok);
    auto head = exact<uint8_t>(n_sum + 1ull);
    c.doc_fieldnorm = f.doc_fieldnorm.get();
    c.doc_payload = f.doc_payload.get();
    c.term_key = f.term_key.get();
    c.term_wand_fn = f.term_wand_fn.get();
    c.term_wand_tf = f.term_wand_tf.get();
    c.term_df = f.term_df.get();
    c.term_first_block = f.term_first_block.get();
    c.tok_page = tok_page.get();
    c.tok_slot = tok_slot.get();
    c.tok_nb = tok_nb.get();
    c.tok_fb = tok_fb.get();
    c.blk_min = f.blk_min.get();
    c.blk_max = f.blk_max.get();
    c.blk_wand_tf = f.blk_wand_tf.get();
    c.blk_n = f.blk_n.get();
    c.blk_wand_fn = f.blk_wand_fn.get();
    c.blk_meta_doc = f.blk_meta_doc.get();
    c.blk_meta_tf = f.blk_meta_tf.get();
    c.sum_blk_page = sum_page.get();
    c.sum_blk_slot = sum_slot.get();
    c.blk_head = head.get();
    c.len8 = len8.get();
    c.off8 = f.blk_off8.get();

    uint64_t key = NO_ERROR;
    auto report = [&](uint32_t tape, uint64_t pos, uint32_t r) {
        if (r) key = std::min(key, error_key(tape, pos, r));
    };
    auto tape_loop = [&](uint32_t tape, uint32_t (*lane)(const Planes &, uint32_t, uint32_t)) {
        for (uint32_t p = 0; p < c.tape[tape].n_pages; ++p)
            for (uint32_t i = 0, base = c.tape[tape].pre[p]; i < c.tape[tape].pre[p + 1] - base; ++i) report(tape, uint64_t(base) + i, lane(c, p, i));
    };
    tape_loop(T_DOCS, doc_lane);
    tape_loop(T_TOKENS, token_lane);
    unsigned long long at = 0;
    for (uint32_t t = 0; t < n_tok; ++t) tok_fb[t] = at, at += tok_nb[t];
    tape_loop(T_SUMMARIES, summary_lane);
    for (uint32_t t = 0; t < n_tok; ++t) report(T_TOKENS, t, term_lane(c, t));
    tape_loop(T_BLOCKS, block_lane);
    uint64_t total8 = 0;
    for (uint32_t j = 0; j <= n_sum; ++j) f.blk_off8[j] = uint32_t(total8), total8 += len8[j];

    bool ascending = true;
    for (uint32_t t = 1; t < n_tok && ascending; ++t) ascending = std::memcmp(&f.term_key[16ull * (t - 1)], &f.term_key[16ull * t], 16) < 0;
    const char *what = nullptr;
    if (int rc = verdict(w, key, ascending, what)) return rc;
    if (total8 > 0xffffffffull) return VBM25_ERR_UNSUPPORTED;
    f.blob_bytes = 8 * total8;
    f.blob = exact<uint8_t>(f.blob_bytes);
    c.blob = f.blob.get();
    for (uint32_t p = 0; p < c.tape[T_BLOCKS].n_pages; ++p)
        for (uint32_t i = 0; i < c.tape[T_BLOCKS].pre[p + 1] - c.tape[T_BLOCKS].pre[p]; ++i)
            for (uint32_t sub = 0; sub < COPY_LANES; ++sub) copy_lane(c, p, i, sub);
    return VBM25_OK;
}

template <class T>
static bool same(const T *a, const T *b, size_t n) {
    return n == 0 || std::memcmp(a, b, n * sizeof(T)) == 0;
}

// both readers on one relation: 1 accepted, 0 refused, -1 they disagree
static int compare(Rel &r) {
    vbm25_segment *seg = nullptr;
    const int host_rc = vbm25_segment_from_pages(read_page, &r, &seg);
    Flat f;
    const int dev_rc = read_like_the_device(read_page, &r, f);
    if (host_rc != dev_rc) {
        std::printf("codes differ: host reader %d, device reader's functions %d\n", host_rc, dev_rc);
        if (seg) vbm25_segment_free(seg);
        return -1;
    }
    if (host_rc != VBM25_OK) return 0;
    vbm25_index_desc d;
    vbm25_segment_desc(seg, &d);
    const bool eq = d.n_docs == f.n_docs && d.n_terms == f.n_terms && d.n_blocks == f.n_blocks && d.sum_len == f.sum_len && d.k1 == f.k1 &&
                    d.b == f.b && d.blob_bytes == f.blob_bytes && same(d.term_key, f.term_key.get(), 16ull * d.n_terms) &&
                    same(d.term_df, f.term_df.get(), d.n_terms) && same(d.term_wand_fn, f.term_wand_fn.get(), d.n_terms) &&
                    same(d.term_wand_tf, f.term_wand_tf.get(), d.n_terms) && same(d.term_first_block, f.term_first_block.get(), d.n_terms + 1ull) &&
                    same(d.blk_min_doc, f.blk_min.get(), d.n_blocks) && same(d.blk_max_doc, f.blk_max.get(), d.n_blocks) &&
                    same(d.blk_n, f.blk_n.get(), d.n_blocks) && same(d.blk_wand_fn, f.blk_wand_fn.get(), d.n_blocks) &&
                    same(d.blk_wand_tf, f.blk_wand_tf.get(), d.n_blocks) && same(d.blk_meta_doc, f.blk_meta_doc.get(), d.n_blocks) &&
                    same(d.blk_meta_tf, f.blk_meta_tf.get(), d.n_blocks) && same(d.blk_off8, f.blk_off8.get(), d.n_blocks + 1ull) &&
                    same(d.blob, f.blob.get(), d.blob_bytes) && same(d.doc_fieldnorm, f.doc_fieldnorm.get(), d.n_docs) &&
                    same(d.doc_payload, f.doc_payload.get(), 3ull * d.n_docs);
    vbm25_segment_free(seg);
    if (!eq) {
        std::printf("both readers accept, the arrays differ\n");
        return -1;
    }
    return 1;
}

static bool run_case_file(const char *path) {
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return std::printf("cannot open %s\n", path), false;
    auto u32 = [&] {
        uint32_t v = 0;
        if (std::fread(&v, 4, 1, fp) != 1) v = 0;
        return v;
    };
    Rel clean;
    const uint32_t n_pages = u32();
    for (uint32_t i = 0; i < n_pages; ++i) {
        clean.pages.emplace_back(8192);
        if (std::fread(clean.pages.back().data(), 8192, 1, fp) != 1) return std::fclose(fp), false;
    }
    const uint32_t n_cases = u32();
    int ok = 0, bad = 0;
    for (uint32_t it = 0; it < n_cases; ++it) {
        Rel r = clean;
        for (uint32_t e = u32(); e; --e) {
            const uint32_t pg = u32(), pos = u32(), val = u32();
            if (pg < r.pages.size() && pos < 8192) r.pages[pg][pos] = uint8_t(val);
        }
        const int got = compare(r);
        if (got < 0) return std::printf("case %u of the file\n", it), std::fclose(fp), false;
        (got ? ok : bad) += 1;
    }
    std::fclose(fp);
    std::printf("case file done: %d flattened, %d rejected\n", ok, bad);
    return true;
}

int main(int argc, char **argv) {
    if (argc > 1 && !run_case_file(argv[1])) return 1;
    if (argc > 2) return std::strcmp(argv[2], "only") == 0 ? 0 : (std::printf("unknown argument %s\n", argv[2]), 1);
    // the corpus and the damage of tests/native/fuzz_pages.cpp: 40 terms over 3000 documents, 30 inserted documents
    std::mt19937_64 rng(7);
    const uint32_t n_docs = 3000, n_terms = 40;
    std::vector<uint32_t> doc_len(n_docs, 0), post_doc, post_tf;
    std::vector<uint16_t> payload(3 * n_docs, 1);
    std::vector<uint64_t> term_start{0};
    std::vector<uint8_t> keys(16 * n_terms, 0);
    for (uint32_t t = 0; t < n_terms; ++t) {
        std::snprintf(reinterpret_cast<char *>(&keys[16 * t]), 16, "k%03u", t);
        for (uint32_t d = 0; d < n_docs; ++d)
            if (rng() % 7 == 0) {
                post_doc.push_back(d);
                post_tf.push_back(1 + rng() % 4);
                doc_len[d] += post_tf.back();
            }
        term_start.push_back(post_doc.size());
    }
    for (auto &l : doc_len) l = l ? l : 1;
    orc_index *ix = orc_index_build(1.2, 0.75, n_docs, doc_len.data(), payload.data(), n_terms, keys.data(), term_start.data(),
                                    post_doc.data(), post_tf.data());
    orc_pages *op = orc_pages_build(ix, nullptr);
    for (int i = 0; i < 30; ++i) {
        const uint16_t pl[3] = {uint16_t(i), 2, 3};
        std::vector<uint32_t> tfs(1 + rng() % 600, 2);
        std::vector<uint8_t> k(16 * tfs.size(), 0);
        for (size_t j = 0; j < tfs.size(); ++j) std::snprintf(reinterpret_cast<char *>(&k[16 * j]), 16, "g%05zu", j);
        orc_pages_insert(op, pl, uint32_t(tfs.size()), k.data(), tfs.data());
    }
    Rel clean;
    for (uint32_t i = 0; i < orc_pages_count(op); ++i) clean.pages.emplace_back(orc_pages_get(op, i), orc_pages_get(op, i) + 8192);
    int ok = 0, bad = 0;
    for (int it = 0; it < 4000; ++it) {
        Rel r = clean;
        if (it) {
            const int flips = 1 + rng() % 4;
            for (int f = 0; f < flips; ++f) {
                auto &pg = r.pages[rng() % r.pages.size()];
                const uint32_t pos = (rng() % 3 == 0) ? 12 + rng() % 60 : (rng() % 3 == 0 ? 8184 + rng() % 8 : rng() % 8192);
                pg[pos] = uint8_t(rng());
            }
        }
        const int got = compare(r);
        if (got < 0) return std::printf("damaged relation %d\n", it), 1;
        (got ? ok : bad) += 1;
    }
    std::printf("fuzz done: %d flattened, %d rejected\n", ok, bad);
    orc_pages_free(op);
    orc_index_free(ix);
    return ok > 0 && bad > 0 ? 0 : 1;
}
