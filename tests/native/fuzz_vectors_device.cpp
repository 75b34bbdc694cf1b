// AddressSanitizer harness for the device reader of the vectors tape (vectorchord-bm25_amd/csrc/vectors_parse.h, compiled here by
// plain g++): the host pass and then the grids the kernels of csrc/pages_device.hip run for vbm25_device_growing_from_pages, one
// loop iteration per lane, in the kernels' order, the scans as plain prefix loops, with every array sized exactly as the device
// allocates it (page images per chunk, scratch per tuple count, the CSR per document and element count).  Built and run by
// tests/test_vectors_device_host.py, which compares what is printed here with vbm25_growing_from_pages (and, where that reader
// accepts, with vbm25_growing_upload's rule on the keys); nothing of this file is loaded into another process.
//
// argv[1]: a case file as tests/pages_device_data.py's write_case_file writes it -- u32 n_pages, the page images, u32 n_cases, per
// case u32 n_edits and n_edits x (u32 page, u32 position, u32 byte).  Per case one line:
//   case I: rc 0 docs N elements M crc START KEY TF FIELDNORM PAYLOAD DELETED      (CRC-32 of the six arrays' bytes, as zlib.crc32)
//   case I: rc -2 page P what TEXT                                                 (the host reader's refusal)
//   case I: rc -1 document G                                                       (keys not strictly ascending)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/vbm25.h"
#include "../../vectorchord-bm25_amd/csrc/vectors_parse.h"

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

// the device reader with loops for kernels; prints the case's line
static void read_like_the_device(uint32_t it, vbm25_read_page_fn fn, void *ctx) {
    Walk w;
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
    const bool walked = walk_vectors(fn, ctx, w, [&](uint32_t, uint32_t, const uint8_t *image) {
        if (staging.size() == size_t(CHUNK_PAGES) * BLCKSZ) flush();
        staging.insert(staging.end(), image, image + BLCKSZ);
        return 0;
    }, sink_rc);
    if (!walked) {
        std::printf("case %u: rc %d page %u what %s\n", it, VBM25_ERR_CORRUPT, w.bad_page, w.what);
        return;
    }
    flush();
    const size_t np = w.pid[0].size(), n = w.pre[0].back();

    std::vector<const uint8_t *> chunk_ptr;
    for (const auto &d : chunks) chunk_ptr.push_back(d.get());
    auto pre = exact<uint32_t>(np + 1);
    std::copy(w.pre[0].begin(), w.pre[0].end(), pre.get());
    auto t_meta = exact<uint32_t>(n), t_cnt = exact<uint32_t>(n), t_kept = exact<uint32_t>(n + 1);
    auto t_mark = exact<unsigned long long>(n), t_sum = exact<unsigned long long>(n), t_last = exact<unsigned long long>(n);
    auto t_eoff = exact<unsigned long long>(n + 1);
    auto finished = exact<uint8_t>(n + 1);
    VecPlanes c{};
    c.tape = TapeView{chunk_ptr.data(), nullptr, pre.get(), uint32_t(np), uint32_t(n)};
    c.t_meta = t_meta.get();
    c.t_cnt = t_cnt.get();
    c.t_mark = t_mark.get();
    c.t_sum = t_sum.get();
    c.t_last = t_last.get();
    c.finished = finished.get();
    c.t_kept = t_kept.get();
    c.t_eoff = t_eoff.get();

    uint64_t key = NO_ERROR;
    auto report = [&](uint64_t pos, uint32_t r) {
        if (r) key = std::min(key, error_key(0, pos, r));
    };
    for (uint32_t p = 0; p < np; ++p)
        for (uint32_t i = 0, base = pre[p]; i < pre[p + 1] - base; ++i) report(uint64_t(base) + i, classify_lane(c, p, i));
    unsigned long long sum = 0, last = 0;
    for (size_t g = 0; g < n; ++g) {
        t_sum[g] = sum += tuple_increment(t_meta[g]);
        t_last[g] = last;
        last = std::max(last, t_mark[g]);
    }
    for (size_t g = 0; g < n; ++g) report(g, resolve_lane(c, g));
    for (size_t g = 0; g < n; ++g) kept_lane(c, g);
    unsigned long long n_el = 0;
    for (size_t g = 0; g <= n; ++g) t_eoff[g] = n_el, n_el += t_kept[g];
    if (key != NO_ERROR) {
        std::printf("case %u: rc %d page %u what %s\n", it, VBM25_ERR_CORRUPT, error_page(w, key), vreason_text(key_reason(key)));
        return;
    }
    const uint32_t n_docs = n ? uint32_t(t_sum[n - 1]) : 0;

    auto start = exact<unsigned long long>(n_docs + 1ull);
    auto g_key = exact<Key128>(n_el);
    auto tf = exact<uint32_t>(n_el);
    auto fieldnorm = exact<uint8_t>(n_docs), deleted = exact<uint8_t>(n_docs);
    auto payload = exact<uint16_t>(3ull * n_docs);
    c.n_docs = n_docs;
    c.n_el = n_el;
    c.start = start.get();
    c.key = reinterpret_cast<uint8_t *>(g_key.get());
    c.tf = tf.get();
    c.fieldnorm = fieldnorm.get();
    c.deleted = deleted.get();
    c.payload = payload.get();
    for (uint32_t p = 0; p < np; ++p)
        for (uint32_t i = 0; i < pre[p + 1] - pre[p]; ++i) finish_lane(c, p, i);
    for (uint32_t p = 0; p < np; ++p)
        for (uint32_t j = 0, m = page_elements(c, p); j < m; ++j) copy_element_lane(c, p, j);
    for (uint32_t p = 0; p < np; ++p)
        for (uint32_t j = 0, m = page_elements(c, p); j < m; ++j) {
            uint32_t doc = 0;
            const uint32_t r = check_element_lane(c, p, j, doc);
            report(doc, r);
        }
    if (key != NO_ERROR) {
        std::printf("case %u: rc %d document %u\n", it, VBM25_ERR_INVALID, uint32_t(key_pos(key)));
        return;
    }
    std::printf("case %u: rc 0 docs %u elements %llu crc %08x %08x %08x %08x %08x %08x\n", it, n_docs, n_el,
                crc32(start.get(), 8 * (n_docs + 1ull)), crc32(g_key.get(), 16 * n_el), crc32(tf.get(), 4 * n_el),
                crc32(fieldnorm.get(), n_docs), crc32(payload.get(), 6ull * n_docs), crc32(deleted.get(), n_docs));
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
