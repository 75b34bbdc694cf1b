// fuzz_sparse_big.cpp -- csrc/sparse_big_lane.h under AddressSanitizer + UBSan on the CPU: the functions scan_sparse_big_kernel's tiles
// are made of, driven as its workgroup drives them.  A stand-alone program (tests/test_sparse_big_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/fuzz_sparse_big.cpp -o fuzz_sparse_big && ./fuzz_sparse_big
// A case is one item: up to 16 terms with random sorted runs of document ids over a few windows (thin, crowded, clustered, runs that
// start at every alignment), a document range [lo, hi) that cuts windows.  The item is walked as wave 0 walks it -- tile_end, the
// slices by run_lower_bound, halving until tile_fits -- and every tile carried out thread by thread: chunk_term / chunk_start /
// chunk_mask (the two "loads" read exactly sized vectors: a chunk outside the term's padded blocks is a heap overflow here), mark,
// word prefix, slot_of, the add per term.  The sums must equal a std::map accumulation of the same postings, every posting counted once.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../../vectorchord-bm25_amd/csrc/sparse_big_lane.h"

using namespace vbm25;

struct Term {
    std::vector<uint32_t> doc;      // ascending
    std::vector<uint16_t> id16;     // padded to whole blocks of 128, as post_id16
    std::vector<uint32_t> win_off;  // n_win + 1
};

static int one_case(uint32_t seed, uint32_t *tiles, uint32_t *slow, uint32_t *halved) {
    std::mt19937_64 rng(seed);
    const uint32_t n_win = 1 + uint32_t(rng() % 3);
    const uint32_t n_docs = (n_win - 1) * sbig::WIN + 1 + uint32_t(rng() % sbig::WIN);
    const uint32_t m = seed % 5 == 0 ? sbig::MAX_T : 1 + uint32_t(rng() % sbig::MAX_T);
    const int shape = int(seed % 4);  // thin | crowded | one cluster of consecutive documents | every term the same documents
    std::vector<Term> terms(m);
    for (uint32_t t = 0; t < m; ++t) {
        Term &T = terms[t];
        const uint32_t df = shape == 0 ? uint32_t(rng() % 400) : shape == 1 ? 2000 + uint32_t(rng() % 6000) : 300 + uint32_t(rng() % 1500);
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
        for (uint32_t w = 0; w <= n_win; ++w)
            T.win_off[w] = uint32_t(std::lower_bound(d.begin(), d.end(), w << 16) - d.begin());  // (n_win <= 3)
        T.win_off[n_win] = uint32_t(d.size());
    }
    uint32_t lo = uint32_t(rng() % n_docs), hi = uint32_t(rng() % (n_docs + 1));
    if (lo > hi) std::swap(lo, hi);
    if (seed % 3 == 0) lo = 0, hi = n_docs;
    std::map<uint32_t, uint64_t> want, got;  // document -> sum of (term + 1) * 1000 + position-independent weight
    for (uint32_t t = 0; t < m; ++t)
        for (uint32_t d : terms[t].doc)
            if (d >= lo && d < hi) want[d] += (t + 1) * 1000ull + d % 7;

    std::vector<uint32_t> bm(sbig::BM_WORDS, 0), pre(sbig::BM_WORDS, 0);
    std::vector<uint64_t> acc(sbig::CAP, 0);
    std::vector<uint32_t> sid(sbig::CAP, 0);
    uint32_t cur = lo, W = sbig::WIN, wl = 0xffffffffu;
    std::vector<uint32_t> sa(m), sb(m), wo0(m), wo1(m), cb(m + 1);
    while (cur < hi) {
        const uint32_t w = cur >> 16;
        if (w != wl) {
            for (uint32_t t = 0; t < m; ++t) {
                const Term &T = terms[t];
                wo0[t] = T.win_off.at(w), wo1[t] = T.win_off.at(w + 1);
                sa[t] = (cur & (sbig::WIN - 1)) ? sbig::run_lower_bound([&](uint32_t i) { return T.id16.at(i); }, wo0[t], wo1[t], cur & (sbig::WIN - 1)) : wo0[t];
            }
            wl = w;
            W = sbig::WIN;
        }
        const uint32_t part_hi = sbig::part_end(w, hi);
        uint32_t tend, posts, chunks;
        for (;;) {
            tend = sbig::tile_end(cur, W, part_hi);
            if (tend <= cur || tend > part_hi) return std::printf("FAIL case %u: tile [%u, %u)\n", seed, cur, tend), 1;
            const bool to_end = (tend & (sbig::WIN - 1)) == 0 || tend == n_docs;
            posts = chunks = 0;
            for (uint32_t t = 0; t < m; ++t) {
                const Term &T = terms[t];
                sb[t] = to_end ? wo1[t] : sbig::run_lower_bound([&](uint32_t i) { return T.id16.at(i); }, sa[t], wo1[t], tend & (sbig::WIN - 1));
                cb[t] = chunks;
                posts += sb[t] - sa[t];
                chunks += sbig::chunks_of(sa[t], sb[t]);
            }
            cb[m] = chunks;
            if (sbig::tile_fits(posts, chunks)) break;
            if (W == 1) return std::printf("FAIL case %u: a tile of one document does not fit\n", seed), 1;
            W = sbig::halve(W);
            ++*halved;
        }
        if (posts) {
            ++*tiles;
            *slow += !sbig::whole_window(cur, tend, n_docs);
            struct Thread { uint32_t t, mask, idw[4], tfw[4]; };
            std::vector<Thread> th(chunks);
            if (chunks > sbig::THREADS) return std::printf("FAIL case %u: %u chunks\n", seed, chunks), 1;
            for (uint32_t c = 0; c < chunks; ++c) {  // load + mark
                Thread &x = th[c];
                x.t = sbig::chunk_term(cb.data(), m, c);
                const Term &T = terms[x.t];
                const uint32_t start = sbig::chunk_start(sa[x.t], cb[x.t], c);
                x.mask = sbig::chunk_mask(start, sa[x.t], sb[x.t]);
                if (start % sbig::CHUNK || !x.mask) return std::printf("FAIL case %u: chunk %u start %u mask %u\n", seed, c, start, x.mask), 1;
                for (uint32_t e = 0; e < 4; ++e) {
                    x.idw[e] = uint32_t(T.id16.at(start + 2 * e)) | uint32_t(T.id16.at(start + 2 * e + 1)) << 16;
                    // (tf = term + 1 in the low bytes, fieldnorm = id % 7 in the high ones)
                    x.tfw[e] = (x.t + 1) | (x.t + 1) << 8 | (T.id16.at(start + 2 * e) % 7u) << 16 | (T.id16.at(start + 2 * e + 1) % 7u) << 24;
                }
                for (uint32_t e = 0; e < sbig::CHUNK; ++e)
                    if ((x.mask >> e) & 1) {
                        const uint32_t id = sbig::chunk_id(x.idw, e);
                        bm.at(id >> 5) |= 1u << (id & 31);
                    }
            }
            uint32_t n_slots = 0;
            for (uint32_t i = 0; i < sbig::BM_WORDS; ++i) pre[i] = n_slots, n_slots += sbig::popc(bm[i]);  // rank
            if (n_slots > sbig::CAP) return std::printf("FAIL case %u: %u slots\n", seed, n_slots), 1;
            for (uint32_t t = 0; t < m; ++t)  // add, term after term
                for (uint32_t c = cb[t]; c < cb[t + 1]; ++c) {
                    Thread &x = th[c];
                    if (x.t != t) return std::printf("FAIL case %u: chunk %u is term %u's, not %u's\n", seed, c, x.t, t), 1;
                    for (uint32_t e = 0; e < sbig::CHUNK; ++e)
                        if ((x.mask >> e) & 1) {
                            const uint32_t id = sbig::chunk_id(x.idw, e);
                            const uint32_t s = sbig::slot_of(pre.at(id >> 5), bm.at(id >> 5), id & 31);
                            if (sbig::chunk_tf(x.tfw, e) != t + 1 || sbig::chunk_fn(x.tfw, e) != id % 7) return std::printf("FAIL case %u: tf / fieldnorm bytes\n", seed), 1;
                            acc.at(s) += sbig::chunk_tf(x.tfw, e) * 1000ull + ((w << 16) + id) % 7;
                            sid.at(s) = id;
                        }
                }
            for (uint32_t s = 0; s < n_slots; ++s) {  // sweep
                const uint32_t d = (w << 16) + sid[s];
                if (d < cur || d >= tend || got.count(d)) return std::printf("FAIL case %u: document %u in tile [%u, %u)\n", seed, d, cur, tend), 1;
                got[d] = acc[s];
                acc[s] = 0;
            }
            std::fill(bm.begin(), bm.end(), 0u);
        }
        cur = tend;
        sa = sb;
        W = sbig::widen(W);
    }
    if (got != want) return std::printf("FAIL case %u (%u terms, shape %d, [%u, %u) of %u): the sums differ from the map's\n", seed, m, shape, lo, hi, n_docs), 1;
    return 0;
}

int main() {
    uint32_t tiles = 0, slow = 0, halved = 0;
    for (uint32_t seed = 0; seed < 200; ++seed)
        if (one_case(seed, &tiles, &slow, &halved)) return 1;
    std::printf("200 cases, %u tiles, %u on the slow path, %u halvings\n", tiles, slow, halved);
    if (tiles < 400 || slow < 200 || halved < 200) return std::printf("FAIL the cases do not exercise the slow path or the halving\n"), 1;
    std::printf("fuzz done\n");
    return 0;
}
