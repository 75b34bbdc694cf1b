// fuzz_bigk_win.cpp -- csrc/bigk_win_lane.h (and the sbig:: functions it rests on) under AddressSanitizer + UBSan on the CPU: the
// functions bigk_scan_win_kernel's tiles are made of, driven as its workgroup drives them.  A stand-alone program
// (tests/test_bigk_win_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_bigk_win.cpp -o fuzz_bigk_win && ./fuzz_bigk_win
// A case is one item: up to 16 terms with sorted runs of document ids over up to six windows (thin, crowded, clustered, identical),
// a run of whole windows [win_lo, win_hi) and a tile span g_tile.  The item is walked as wave 0 walks it -- the longest run of whole
// windows that fits (fit_windows), else the window in halving parts -- and every tile carried out thread by thread: chunk loads from
// exactly sized vectors, posting_window / tile_id, mark, word prefix, slot_of, the add per term.  The sums must equal a std::map
// accumulation, every posting counted once.  Then field_at over both packings, every bit width 1 .. 32 and byte width 1 .. 4, against
// a bit-by-bit extraction.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/bigk_win_lane.h"

using namespace vbm25;

struct Term {
    std::vector<uint32_t> doc;      // ascending
    std::vector<uint16_t> id16;     // padded to whole blocks of 128, as post_id16
    std::vector<uint32_t> win_off;  // n_win + 1
};

static int one_case(uint32_t seed, uint32_t *tiles, uint32_t *slow, uint32_t *multi) {
    std::mt19937_64 rng(seed);
    const uint32_t n_win = 1 + uint32_t(rng() % 6);
    const uint32_t n_docs = (n_win - 1) * sbig::WIN + 1 + uint32_t(rng() % sbig::WIN);
    const uint32_t m = seed % 5 == 0 ? sbig::MAX_T : 1 + uint32_t(rng() % sbig::MAX_T);
    const int shape = int(seed % 4);  // thin | crowded | one cluster of consecutive documents | every term the same documents
    std::vector<Term> terms(m);
    for (uint32_t t = 0; t < m; ++t) {
        Term &T = terms[t];
        const uint32_t df = shape == 0 ? uint32_t(rng() % 300) : shape == 1 ? 2000 + uint32_t(rng() % 6000) : 300 + uint32_t(rng() % 1500);
        std::vector<uint32_t> d;
        const uint32_t at = uint32_t(rng() % n_docs);
        if (shape == 3 && t) d = terms[0].doc;
        else for (uint32_t i = 0; i < df; ++i) d.push_back(shape == 2 ? std::min(at + i, n_docs - 1) : uint32_t(rng() % n_docs));
        std::sort(d.begin(), d.end());
        d.erase(std::unique(d.begin(), d.end()), d.end());
        T.doc = d;
        T.id16.assign((d.size() + 127) / 128 * 128, 0xffff);
        for (size_t i = 0; i < d.size(); ++i) T.id16[i] = uint16_t(d[i] & 0xffff);
        T.win_off.assign(n_win + 1, 0);
        for (uint32_t w = 0; w < n_win; ++w) T.win_off[w] = uint32_t(std::lower_bound(d.begin(), d.end(), w << 16) - d.begin());
        T.win_off[n_win] = uint32_t(d.size());
    }
    uint32_t win_lo = uint32_t(rng() % n_win), win_hi = 1 + uint32_t(rng() % n_win);
    if (win_lo >= win_hi || seed % 3 == 0) win_lo = 0, win_hi = n_win;
    const uint32_t g_tile = seed % 4 == 3 ? 1 + uint32_t(rng() % bwin::MAX_G) : bwin::MAX_G;
    std::map<uint32_t, uint64_t> want, got;
    for (uint32_t t = 0; t < m; ++t)
        for (uint32_t d : terms[t].doc)
            if ((d >> 16) >= win_lo && (d >> 16) < win_hi) want[d] += (t + 1) * 1000ull + d % 7;

    std::vector<uint32_t> bm(bwin::BM_WORDS, 0), pre(bwin::BM_WORDS, 0), sid(sbig::CAP, 0);
    std::vector<uint64_t> acc(sbig::CAP, 0);
    std::vector<uint32_t> sa(m), sb(m), cb(m + 1), inner(m * bwin::INNER, 0);
    uint32_t w = win_lo, cur = 0, W = sbig::WIN, part_hi = 0;
    bool slow_mode = false;
    while (slow_mode || w < win_hi) {
        uint32_t g = 1, posts = 0, chunks = 0, pw = w;
        auto total = [&]() {
            posts = chunks = 0;
            for (uint32_t t = 0; t < m; ++t) cb[t] = chunks, posts += sb[t] - sa[t], chunks += sbig::chunks_of(sa[t], sb[t]);
            cb[m] = chunks;
        };
        if (!slow_mode) {
            const uint32_t gmax = bwin::tile_windows(g_tile, win_hi - w);
            if (gmax < 1 || gmax > bwin::MAX_G || w + gmax > win_hi) return std::printf("FAIL case %u: tile_windows %u\n", seed, gmax), 1;
            g = bwin::fit_windows([&](uint32_t n, uint32_t &p, uint32_t &c) {
                for (uint32_t t = 0; t < m; ++t) sa[t] = terms[t].win_off.at(w), sb[t] = terms[t].win_off.at(w + n);
                total();
                p = posts, c = chunks; }, gmax);
            if (g) {
                for (uint32_t t = 0; t < m; ++t)
                    for (uint32_t i = 0; i + 1 < bwin::MAX_G; ++i) inner[t * bwin::INNER + i] = terms[t].win_off.at(w + std::min(i + 1, gmax));
                w += g;
                *multi += g > 1 && posts;
            } else {
                slow_mode = true;
                cur = w << 16, part_hi = sbig::part_end(w, n_docs), W = sbig::WIN >> 1;
                for (uint32_t t = 0; t < m; ++t) sa[t] = terms[t].win_off.at(w);
            }
        }
        if (slow_mode) {
            g = 1;
            uint32_t tend;
            std::vector<uint32_t> a0 = sa;
            for (;;) {
                tend = sbig::tile_end(cur, W, part_hi);
                if (tend <= cur || tend > part_hi) return std::printf("FAIL case %u: tile [%u, %u)\n", seed, cur, tend), 1;
                for (uint32_t t = 0; t < m; ++t) {
                    const Term &T = terms[t];
                    sa[t] = a0[t];
                    sb[t] = tend == part_hi ? T.win_off.at(w + 1) : sbig::run_lower_bound([&](uint32_t i) { return T.id16.at(i); }, sa[t], T.win_off.at(w + 1), tend & (sbig::WIN - 1));
                }
                total();
                if (sbig::tile_fits(posts, chunks)) break;
                if (W == 1) return std::printf("FAIL case %u: a tile of one document does not fit\n", seed), 1;
                W = sbig::halve(W);
            }
            *slow += posts != 0;
            cur = tend;
            W = sbig::widen(W);
            if (cur >= part_hi) slow_mode = false, ++w;
        }
        if (posts) {
            ++*tiles;
            struct Thread { uint32_t t, mask, start, idw[4]; };
            std::vector<Thread> th(chunks);
            if (chunks > sbig::THREADS || posts > sbig::CAP) return std::printf("FAIL case %u: %u chunks, %u postings\n", seed, chunks, posts), 1;
            for (uint32_t c = 0; c < chunks; ++c) {  // load + mark
                Thread &x = th[c];
                x.t = sbig::chunk_term(cb.data(), m, c);
                const Term &T = terms[x.t];
                x.start = sbig::chunk_start(sa[x.t], cb[x.t], c);
                x.mask = sbig::chunk_mask(x.start, sa[x.t], sb[x.t]);
                if (x.start % sbig::CHUNK || !x.mask) return std::printf("FAIL case %u: chunk %u start %u mask %u\n", seed, c, x.start, x.mask), 1;
                for (uint32_t e = 0; e < 4; ++e) x.idw[e] = uint32_t(T.id16.at(x.start + 2 * e)) | uint32_t(T.id16.at(x.start + 2 * e + 1)) << 16;
                for (uint32_t e = 0; e < sbig::CHUNK; ++e)
                    if ((x.mask >> e) & 1) {
                        const uint32_t rid = bwin::tile_id(bwin::posting_window(x.start + e, &inner[x.t * bwin::INNER], g), sbig::chunk_id(x.idw, e));
                        bm.at(rid >> 5) |= 1u << (rid & 31);
                    }
            }
            uint32_t n_slots = 0;
            for (uint32_t i = 0; i < bwin::BM_WORDS; ++i) pre[i] = n_slots, n_slots += sbig::popc(bm[i]);  // rank
            if (n_slots > sbig::CAP) return std::printf("FAIL case %u: %u slots\n", seed, n_slots), 1;
            for (uint32_t t = 0; t < m; ++t)  // add, term after term
                for (uint32_t c = cb[t]; c < cb[t + 1]; ++c) {
                    Thread &x = th[c];
                    if (x.t != t) return std::printf("FAIL case %u: chunk %u is term %u's, not %u's\n", seed, c, x.t, t), 1;
                    for (uint32_t e = 0; e < sbig::CHUNK; ++e)
                        if ((x.mask >> e) & 1) {
                            const uint32_t rid = bwin::tile_id(bwin::posting_window(x.start + e, &inner[t * bwin::INNER], g), sbig::chunk_id(x.idw, e));
                            const uint32_t s = sbig::slot_of(pre.at(rid >> 5), bm.at(rid >> 5), rid & 31);
                            acc.at(s) += (t + 1) * 1000ull + ((pw << 16) + rid) % 7;
                            sid.at(s) = rid;
                        }
                }
            for (uint32_t s = 0; s < n_slots; ++s) {  // sweep
                const uint32_t d = (pw << 16) + sid[s];
                if ((d >> 16) < pw || (d >> 16) >= pw + g || d >= n_docs || got.count(d)) return std::printf("FAIL case %u: document %u in the tile of windows [%u, %u)\n", seed, d, pw, pw + g), 1;
                got[d] = acc[s];
                acc[s] = 0;
            }
            std::fill(bm.begin(), bm.end(), 0u);
        }
        if (slow_mode)
            for (uint32_t t = 0; t < m; ++t) sa[t] = sb[t];
    }
    if (got != want) return std::printf("FAIL case %u (%u terms, shape %d, windows [%u, %u) of %u, g %u): the sums differ from the map's\n", seed, m, shape, win_lo, win_hi, n_win, g_tile), 1;
    return 0;
}

// n fields of `width` bits (bit-packed: four interleaved LSB-first streams of 32-bit words) or bytes, written and read back bit by bit
static int field_cases() {
    std::mt19937_64 rng(7);
    uint32_t checked = 0;
    for (uint32_t packing = 0; packing < 2; ++packing)
        for (uint32_t width = 1; width <= (packing ? 4u : 32u); ++width)
            for (uint32_t n : {128u, 1u, 77u}) {
                if (!packing && n != 128u) continue;  // (bit-packed blocks are full)
                const uint32_t meta = packing << 7 | width, bits = packing ? 8 * width : width;
                std::vector<uint32_t> v(n);
                for (uint32_t &x : v) x = uint32_t(rng()) & (bits == 32 ? 0xffffffffu : (1u << bits) - 1u);
                v[0] = bits == 32 ? 0xffffffffu : (1u << bits) - 1u;
                const uint32_t bytes = bwin::payload_bytes(meta, n);
                if (bytes != (packing ? width * n : 16 * width)) return std::printf("FAIL payload_bytes(%u, %u)\n", meta, n), 1;
                std::vector<uint32_t> words((bytes + 3) / 4, 0);  // exactly sized: a read past the payload is a heap overflow here
                uint8_t *p = reinterpret_cast<uint8_t *>(words.data());
                for (uint32_t i = 0; i < n; ++i)
                    for (uint32_t b = 0; b < bits; ++b) {
                        if (!((v[i] >> b) & 1)) continue;
                        const uint32_t bit = packing ? 8 * width * i + b : (i >> 2) * width + b;  // byte-packed: the byte stream; bit-packed: stream i % 4
                        if (packing) p[bit >> 3] |= uint8_t(1u << (bit & 7));
                        else words[4 * (bit >> 5) + (i & 3)] |= 1u << (bit & 31);
                    }
                for (uint32_t i = 0; i < n; ++i, ++checked)
                    if (bwin::field_at(p, meta, i) != v[i]) return std::printf("FAIL field_at: packing %u width %u field %u of %u\n", packing, width, i, n), 1;
                // tf_fields: the next multiple of 8 behind the id payload
                if (bwin::tf_fields(p, meta, n) - p != ((bytes + 7) & ~7u)) return std::printf("FAIL tf_fields\n"), 1;
            }
    const uint32_t tfw[4] = {0x01020304u, 0u, 0x00010000u, 0u};
    if (bwin::wide_pair(tfw, 0) || !bwin::wide_pair(tfw, 2) || !bwin::wide_pair(tfw, 3) || bwin::wide_pair(tfw, 5) || !bwin::wide_pair(tfw, 7)) return std::printf("FAIL wide_pair\n"), 1;
    std::printf("%u fields\n", checked);
    return 0;
}

int main() {
    uint32_t tiles = 0, slow = 0, multi = 0;
    for (uint32_t seed = 0; seed < 200; ++seed)
        if (one_case(seed, &tiles, &slow, &multi)) return 1;
    std::printf("200 cases, %u tiles, %u on the slow path, %u over several windows\n", tiles, slow, multi);
    if (tiles < 400 || slow < 100 || (bwin::MAX_G > 1 && multi < 50)) return std::printf("FAIL the cases do not exercise the slow path or the multi-window tiles\n"), 1;
    if (field_cases()) return 1;
    std::printf("fuzz done\n");
    return 0;
}
