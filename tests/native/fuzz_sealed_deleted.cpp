// AddressSanitizer harness for the flags half of the device reader of VACUUM's inputs (vbm25_device_vacuum_from_pages): the per-tuple
// function doc_deleted_lane and the word packing flag_round_words of vectorchord-bm25_amd/csrc/pages_parse.h, compiled here by plain
// g++.  The host pass is the reader's (Meta, Jump, the documents tape by walk_tape_pages with the special area looked at last), then
// doc_deleted_kernel's grid as loops: one iteration per page, per round of 64 slots and per lane, the ballot as a loop over the
// lanes, the atomic ORs as plain ORs, with the page images per chunk and the words sized exactly as the device allocates them.
// Built and run by tests/test_vacuum_device_host.py, which compares what is printed here with vbm25_sealed_deleted_from_pages;
// nothing of this file is loaded into another process.
//
// argv[1]: a case file as tests/pages_device_data.py's write_case_file writes it.  Per case one line:
//   case I: rc 0 docs N deleted D crc WORDS        (CRC-32 of the ceil(N / 64) words' bytes, as zlib.crc32)
//   case I: rc -2 page P what TEXT                 (the host reader's refusal)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <unordered_set>
#include <vector>

#include "../../include/vbm25.h"
#include "../../vectorchord-bm25_amd/csrc/pages_parse.h"

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

static uint32_t crc32(const void *data, size_t n) {
    static uint32_t table[256];
    if (!table[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    uint32_t c = 0xffffffffu;
    const uint8_t *p = static_cast<const uint8_t *>(data);
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

static const char *doc_reason_text(uint32_t r) { return r == R_TUPLE_SHORT ? "document tuple too short" : reason_text(r); }

static void read_like_the_device(uint32_t it, vbm25_read_page_fn fn, void *ctx) {
    Walk w;
    const uint8_t *j = read_meta_jump(fn, ctx, w);
    if (!j) {
        std::printf("case %u: rc %d page %u what %s\n", it, VBM25_ERR_CORRUPT, w.bad_page, w.what);
        return;
    }
    const uint32_t ptr_documents = host_rd32(j + 44), n_docs = w.n_docs;
    std::vector<std::unique_ptr<uint8_t[]>> chunks;
    std::vector<uint8_t> staging;  // one chunk being filled
    auto flush = [&] {
        if (staging.empty()) return;
        auto d = exact<uint8_t>(staging.size());
        std::memcpy(d.get(), staging.data(), staging.size());
        chunks.push_back(std::move(d));
        staging.clear();
    };
    int sink_rc = 0;
    std::unordered_set<uint32_t> seen;
    const bool walked = walk_tape_pages(fn, ctx, w, T_DOCS, ptr_documents, seen, [&](uint32_t, uint32_t, const uint8_t *image) {
        if (staging.size() == size_t(CHUNK_PAGES) * BLCKSZ) flush();
        staging.insert(staging.end(), image, image + BLCKSZ);
        return 0;
    }, sink_rc, true);
    flush();
    const size_t np = w.pid[T_DOCS].size(), n_words = (size_t(n_docs) + 63) / 64;
    std::vector<const uint8_t *> chunk_ptr;
    for (const auto &d : chunks) chunk_ptr.push_back(d.get());
    auto pre = exact<uint32_t>(np + 1);
    std::copy(w.pre[T_DOCS].begin(), w.pre[T_DOCS].end(), pre.get());
    auto words = exact<uint64_t>(n_words);
    const TapeView docs{chunk_ptr.data(), nullptr, pre.get(), uint32_t(np), w.pre[T_DOCS].back()};

    uint64_t key = NO_ERROR;
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t base = pre[p], n = pre[p + 1] - base;
        for (uint32_t r = 0; r < n; r += 64) {
            uint64_t m = 0;  // the wave's ballot
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t i = r + lane;
                bool deleted = false;
                if (i < n) {
                    if (const uint32_t reason = doc_deleted_lane(docs, p, i, deleted)) key = std::min(key, error_key(T_DOCS, uint64_t(base) + i, reason));
                    if (uint64_t(base) + i >= n_docs) deleted = false;
                }
                if (deleted) m |= 1ull << lane;
            }
            if (!m) continue;
            const uint64_t first = uint64_t(base) + r;
            uint64_t lo, hi;
            flag_round_words(first, m, lo, hi);
            if (lo) words[first >> 6] |= lo;
            if (hi) words[(first >> 6) + 1] |= hi;
        }
    }
    uint32_t deleted = 0;
    for (size_t i = 0; i < n_words; ++i) deleted += uint32_t(__builtin_popcountll(words[i]));
    if (key != NO_ERROR) {
        std::printf("case %u: rc %d page %u what %s\n", it, VBM25_ERR_CORRUPT, error_page(w, key), doc_reason_text(key_reason(key)));
        return;
    }
    if (!walked) {
        std::printf("case %u: rc %d page %u what %s\n", it, VBM25_ERR_CORRUPT, w.bad_page, w.what);
        return;
    }
    if (w.pre[T_DOCS].back() != n_docs) {
        std::printf("case %u: rc %d page %u what %s\n", it, VBM25_ERR_CORRUPT, ptr_documents, "document count differs from the Jump tuple");
        return;
    }
    std::printf("case %u: rc 0 docs %u deleted %u crc %08x\n", it, n_docs, deleted, crc32(words.get(), 8 * n_words));
}

int main(int argc, char **argv) {
    if (argc < 2) return std::printf("usage: %s case-file\n", argv[0]), 2;
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) return std::printf("cannot open %s\n", argv[1]), 2;
    auto u32 = [&] {
        uint32_t v = 0;
        if (std::fread(&v, 4, 1, fp) != 1) v = 0;
        return v;
    };
    Rel clean;
    const uint32_t n_pages = u32();
    for (uint32_t i = 0; i < n_pages; ++i) {
        clean.pages.emplace_back(8192);
        if (std::fread(clean.pages.back().data(), 8192, 1, fp) != 1) return std::fclose(fp), 2;
    }
    const uint32_t n_cases = u32();
    for (uint32_t it = 0; it < n_cases; ++it) {
        std::vector<std::pair<uint32_t, std::vector<uint8_t>>> saved;  // the pages a case edits, as they were
        for (uint32_t e = u32(); e; --e) {
            const uint32_t pg = u32(), pos = u32(), val = u32();
            if (pg >= clean.pages.size() || pos >= 8192) continue;
            if (std::none_of(saved.begin(), saved.end(), [&](const auto &s) { return s.first == pg; })) saved.emplace_back(pg, clean.pages[pg]);
            clean.pages[pg][pos] = uint8_t(val);
        }
        read_like_the_device(it, read_page, &clean);
        for (auto &s : saved) clean.pages[s.first] = std::move(s.second);
    }
    std::fclose(fp);
    std::printf("done: %u cases\n", n_cases);
    return 0;
}
