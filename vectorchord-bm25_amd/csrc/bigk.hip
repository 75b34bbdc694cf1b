// bigk.hip -- the sparse half of the k > 1024 route (run_exhaustive, search.hip): batched over queries, its cost grows with the
// postings the queries touch, not with the index.  A query whose document frequencies sum to at most bigk_cand_max takes it; the
// others of the batch keep the per-query path of search.hip (an accumulator per document, one launch per term, a radix sort of every
// document).  Records are byte for byte that path's.  Per chunk of queries (their candidate segments fit the batch's scratch) at most
// one launch of each scan kernel and three more, whatever the queries:
//   bigk_scan_win_kernel   the queries of 1 .. 16 terms that all have a window table (switch bigk_win): work item = (query, run of
//                          2^16-document windows); the candidate scan fed from post_id16 / post_tfn / win_off -- its comment below
//   bigk_scan_kernel       work item = (query, run of 8192-document windows), one workgroup of 8 waves.  Per window the query's terms
//                          in ascending position; per term the waves take the term's blocks that intersect the window (a 64-ary
//                          search of the wave over the blocks' last ids), decode them with decode_doc_ids / decode_fields and add
//                          (tf * s0) / (tf + s1[fn]) -- bigk_accum_kernel's expression -- into the window's f64 accumulators in LDS,
//                          setting the document's bit in the LDS bitmap.  A workgroup barrier separates the terms: within a term no
//                          two postings share a document, so a document's sum is formed in term order as acc[d] is by the per-term
//                          launches.  The sweep reads the bitmap a word a wave, applies the filter's bit, drops zeros, appends
//                          (key, doc) to the query's candidate segment (one atomic add a wave on the query's cursor, ballot rank
//                          within it) and clears what it read: no window-sized wipe.
//   bigk_select_kernel     a workgroup a query: at most k candidates -- all survive; more -- an MSD radix select of the k-th entry of
//                          "key descending, doc ascending" (bigk_lane.h: 8-bit digits through the key, then the inverted doc,
//                          histograms in LDS, stopping when the boundary bucket holds exactly the missing count), then a
//                          compaction of the entries at or above the boundary: exactly min(k, candidates) survivors.
//   bigk_sort_kernel       a workgroup a tile of 4096 survivors: bitonic sort in LDS on rerank_lane.h's schedule, padded with a
//                          worst entry.
//   bigk_rank_emit_kernel  a thread a survivor: its rank is its index in its tile plus, per other tile of the query, the entries of
//                          that tile that beat it (bisection); the record goes to its rank as bigk_emit_kernel writes it, and
//                          n_hits[q] is the survivor count.
// The dense half (switch bigk_dense, an index of at least bigk_dense_min_docs documents): the other queries of the batch, in chunks of
// their own behind the sparse chunks.  Their candidate lists cannot hold every touched document, so bigk_dense_scan_kernel finds a
// threshold first -- histogram scans and bigk_dense_walk_kernel, level after level -- and its emit instantiation lists the entries above
// it; the select, the sort and the emit above take it from there (bigk_dense.h).  No query of it goes back to the per-query path.
// The growing segment of such a batch (switch bigk_grow): growing_bigk.h's scan and merge around the select and the sort here, on
// candidate segments of their own -- growing_bigk_scratch / growing_bigk_run at the end of this file.
// Host: bigk_create sizes the scratch when the batch is made, bigk_plan cuts queries into chunks and items at set_queries (no device
// planning pass), bigk_run enqueues.  Nothing is allocated in a run, and nothing in it waits for the device.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "vbm25_internal.h"
#include "host_objects.h"
#include "decode.h"
#include "block_fetch.h"
#include "topk_reg.h"
#include "rerank_lane.h"
#include "bigk_lane.h"
#include "bigk_win_lane.h"
#include "bigk_dense.h"
#include "growing_bigk.h"

namespace vbm25 {

using ull = unsigned long long;

namespace {

constexpr uint32_t SCAN_WAVES = bgk::SCAN_THREADS / 64;
constexpr uint32_t SWEEP_WORDS = bgk::WINDOW_WORDS / SCAN_WAVES;  // bitmap words a wave sweeps: one a lane of its first lanes
static_assert(bgk::TERM_TABLE >= (uint32_t)MAX_TERMS, "the LDS term table holds every indexed term of a query");
static_assert(SWEEP_WORDS >= 1 && SWEEP_WORDS <= 64, "a wave reads its bitmap words one a lane");
constexpr uint32_t SELECT_THREADS = 1024, SORT_THREADS = 1024, EMIT_THREADS = 256;
constexpr uint32_t ITEM_TARGET = 2048;  // work items of a batch (all its chunks together) the automatic cut aims at: a few per CU

struct Args {
    const BigkQuery *qd;
    const BigkItem *items;
    const uint32_t *terms;
    uint32_t *cursor, *surv_cnt;
    uint64_t *cand_key, *surv_key;
    uint32_t *cand_doc, *surv_doc;
    const ull *filt_words;   // NULL: no filter
    const uint32_t *filt_sel;
    uint32_t filt_stride;
    uint32_t k, surv_stride;
    vbm25_hit *hits;
    uint32_t *n_hits;
    uint32_t *error_flag;
};

// (wave_lower_bound, the wave's 64-ary search over the blocks' last ids: block_fetch.h -- bigk_dense.h's scan uses it too)

__global__ void __launch_bounds__(256) bigk_clear_kernel(uint32_t *v, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = 0;
}

__global__ void __launch_bounds__(bgk::SCAN_THREADS) bigk_scan_kernel(DevIndex ix, Args a, uint32_t item0) {
    __shared__ double s_acc[bgk::WINDOW];
    __shared__ ull s_bits[bgk::WINDOW_WORDS];
    __shared__ uint32_t s_jlo[bgk::TERM_TABLE], s_jhi[bgk::TERM_TABLE];
    __shared__ double s_s0[bgk::TERM_TABLE];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const BigkItem it = a.items[item0 + blockIdx.x];
    const BigkQuery qd = a.qd[it.s];
    const uint32_t nt = qd.term_hi - qd.term_lo;
    if (nt > bgk::TERM_TABLE) {  // (set_queries refuses such a query)
        if (tid == 0) atomicOr(a.error_flag, 8u);
        return;
    }
    const uint32_t doc_lo = it.win_lo * bgk::WINDOW;
    const uint32_t doc_hi = (uint32_t)min((ull)it.win_hi * bgk::WINDOW, (ull)ix.n_docs);
    for (uint32_t i = tid; i < bgk::WINDOW; i += bgk::SCAN_THREADS) s_acc[i] = 0.0;
    for (uint32_t i = tid; i < bgk::WINDOW_WORDS; i += bgk::SCAN_THREADS) s_bits[i] = 0ull;
    // the term table: per term the blocks that can hold a document of the item, and s0
    for (uint32_t p = tid; p < nt; p += bgk::SCAN_THREADS) {
        const uint32_t t = a.terms[qd.term_lo + p];
        const uint32_t j0 = ix.term_first_block[t], j1 = ix.term_first_block[t + 1];
        uint32_t lo = j0, hi = j1;
        while (lo < hi) {  // first block whose last id is >= doc_lo
            const uint32_t mid = (lo + hi) >> 1;
            if (ix.blk_max_doc[mid] >= doc_lo) hi = mid;
            else lo = mid + 1u;
        }
        const uint32_t jlo = lo;
        hi = j1;
        while (lo < hi) {  // first block whose first id is >= doc_hi
            const uint32_t mid = (lo + hi) >> 1;
            if (ix.blk_min_doc[mid] >= doc_hi) hi = mid;
            else lo = mid + 1u;
        }
        s_jlo[p] = jlo;
        s_jhi[p] = lo;
        s_s0[p] = ix.term_s0[t];
    }
    __syncthreads();
    const ull *filt = nullptr;
    if (a.filt_words) {
        const uint32_t sel = a.filt_sel[qd.q];
        if (sel != UINT32_MAX) filt = a.filt_words + size_t(sel) * a.filt_stride;
    }
    uint64_t *ckey = a.cand_key + qd.cand_base;
    uint32_t *cdoc = a.cand_doc + qd.cand_base;
    for (uint32_t w = it.win_lo; w < it.win_hi; ++w) {
        const uint32_t w0 = w * bgk::WINDOW;
        if (w0 >= doc_hi) break;
        const uint32_t w1 = min(w0 + bgk::WINDOW, doc_hi);
        for (uint32_t p = 0; p < nt; ++p) {
            const uint32_t jlo = s_jlo[p], jhi = s_jhi[p];
            if (jlo >= jhi) continue;  // (the whole workgroup: the term has no posting in the item)
            const double s0 = s_s0[p];
            const uint32_t js = wave_lower_bound(ix.blk_max_doc, jlo, jhi, w0, lane);
            for (uint32_t j = js + wave; j < jhi && ix.blk_min_doc[j] < w1; j += SCAN_WAVES) {
                const uint4 bm = ix.blk_meta[j];
                const uint32_t n = bm.w & 0xff, md = (bm.w >> 8) & 0xff, mt = (bm.w >> 16) & 0xff;
                const uint8_t *body = ix.blob + 8ull * bm.z;
                uint32_t d0, d1, f0, f1;
                decode_doc_ids(body, md, n, bm.x, lane, d0, d1);
                decode_fields(body + ((payload_bytes(md, n) + 7u) & ~7u), mt, n, lane, f0, f1);
                const uchar2 fn = reinterpret_cast<const uchar2 *>(ix.post_fn + 128ull * j)[lane];
                if (2 * lane < n && d0 >= w0 && d0 < w1) {
                    const double tf = (double)f0;
                    const uint32_t r = d0 - w0;
                    s_acc[r] = s_acc[r] + (tf * s0) / (tf + ix.s1[fn.x]);  // Cache::evaluate, bm25.rs:355-358
                    atomicOr(&s_bits[r >> 6], 1ull << (r & 63u));
                }
                if (2 * lane + 1 < n && d1 >= w0 && d1 < w1) {
                    const double tf = (double)f1;
                    const uint32_t r = d1 - w0;
                    s_acc[r] = s_acc[r] + (tf * s0) / (tf + ix.s1[fn.y]);
                    atomicOr(&s_bits[r >> 6], 1ull << (r & 63u));
                }
            }
            __syncthreads();  // the next term's adds see this term's sums
        }
        // sweep: every wave its own words of the bitmap
        const uint32_t wbase = wave * SWEEP_WORDS;
        const ull mine = lane < SWEEP_WORDS ? s_bits[wbase + lane] : 0ull;
        ull nz = __ballot(mine != 0ull);
        while (nz) {
            const uint32_t l = (uint32_t)__ffsll((long long)nz) - 1u;
            nz &= nz - 1ull;
            const uint32_t wi = wbase + l;
            const ull word = s_bits[wi];
            ull key = 0;
            if ((word >> lane) & 1ull) {
                key = (ull)__double_as_longlong(s_acc[wi * 64u + lane]);
                s_acc[wi * 64u + lane] = 0.0;
            }
            if (filt && !((filt[(w0 >> 6) + wi] >> lane) & 1ull)) key = 0;  // (bigk_mask_kernel's word and bit)
            const ull m = __ballot(key != 0ull);
            if (m) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(a.cursor + it.s, (uint32_t)__popcll(m));
                base = __shfl(base, 0);
                const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (key != 0ull) {
                    if (slot < qd.cand_cap) {
                        ckey[slot] = key;
                        cdoc[slot] = w0 + wi * 64u + lane;
                    } else {
                        atomicOr(a.error_flag, 8u);
                    }
                }
            }
            if (lane == 0) s_bits[wi] = 0ull;
        }
        __syncthreads();  // the next window's adds find zeros
    }
}

// bigk_scan_win_kernel -- bigk_scan_kernel's contract (the candidates of a work item appended to the query's segment, arrival order
// arbitrary, error flag 8 past cand_cap) fed from the window planes: no block decode, no block search, no hash.  A work item is a
// sparse query of 1 .. 16 indexed terms, every one with a window table, and a run of whole 2^16-document windows; one workgroup of 8
// waves.  bigk_win_lane.h and sparse_big_lane.h have the per-lane functions.
//   plan   wave 0, lane t = term t.  FAST PATH: the longest run of up to g_tile <= MAX_G whole windows [w, w + g) whose slices hold at
//          most 4096 postings in at most 512 chunks of 8.  A term's postings of consecutive windows are contiguous, so its slice is
//          the single run [win_off[w], win_off[w + g]); the g - 1 inner entries go to LDS.  SLOW PATH (one window does not fit): the
//          window in power-of-two aligned parts, the lane bisecting its run, the width halving until the part fits (width 1 does).
//          Empty tiles are passed over by wave 0 alone.
//   load   thread c owns chunk c: 8 ids from post_id16, 8 (tf, tf, fieldnorm, fieldnorm) bytes from post_tfn, one 16-byte load each.
//   mark   a posting's window inside the tile = the inner entries at or below its posting number; its bit in the bitmap of
//          MAX_G x 2^16 bits is window << 16 | id.  Barrier.
//   rank   every thread counts 4 MAX_G consecutive words; a wave scan and one LDS hop give every word the bits before it.  A
//          document's accumulator slot is its rank in the bitmap.  Two barriers.
//   add    term after term in ascending query position, (tf * s0) / (tf + s1[fn]) in f64 without contraction, ONE BARRIER BEHIND
//          EVERY TERM THAT HAS A POSTING IN THE TILE.  Within a term no two postings share a document, so no two threads share a slot
//          between two barriers; across terms the barrier orders the adds.  Every document's sum is therefore formed term after term
//          from 0.0, as acc[d] is by the per-query path's per-term launches (0.0 + x is exact): the keys are bit for bit that path's,
//          whatever the tiles -- the argument bigk_scan_kernel and scan_sparse_big_kernel rest on.  A zero word in post_tfn (a term
//          frequency wider than a byte in the pair): the owning lane reads the exact tf of posting p from block
//          term_first_block + p / 128 (one field, bwin::field_at) and the fieldnorm from post_fn.  Nothing is given up.
//   sweep  a thread a slot: the sum read and cleared, the query's filter bit applied, zeros dropped, (key, doc) appended with one
//          atomic on cursor[s] per wave and round (ballot ranks).  Every thread clears the bitmap words it counted: the LDS is clean
//          for the next tile.
struct BigkWinLds {
    double acc[sbig::CAP];               // 32 KB: a slot's sum, zero between tiles
    uint32_t bm[bwin::BM_WORDS];         // MAX_G x 8 KB: the tile's bitmap, zero between tiles
    uint16_t pre[bwin::BM_WORDS];        // MAX_G x 4 KB: bits set before every word (<= 4096)
    uint32_t sid[sbig::CAP];             // 16 KB: a slot's tile id
    double s1[256];
    double t_s0[sbig::MAX_T];
    uint32_t t_fb[sbig::MAX_T];
    uint32_t p_a[sbig::MAX_T], p_b[sbig::MAX_T], p_cb[sbig::MAX_T + 1];  // the tile's plan: slices and chunk prefix
    uint32_t p_in[sbig::MAX_T][bwin::INNER];                              // ... and the terms' inner window bounds
    uint32_t wsum[SCAN_WAVES];
    uint32_t bad, p_win, p_g, p_done;
};
static_assert(sbig::THREADS == bgk::SCAN_THREADS, "a chunk a thread");

// stats: [0] tiles on the slow path, [1] wide postings decoded (vbm25_batch_debug_bigk_win)
__global__ void __launch_bounds__(bgk::SCAN_THREADS, 4) bigk_scan_win_kernel(DevIndex ix, Args a, uint32_t item0, uint32_t g_tile, uint32_t *stats) {
    __shared__ BigkWinLds S;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);
    const BigkItem it = a.items[item0 + blockIdx.x];
    const BigkQuery qd = a.qd[it.s];
    const uint32_t m = qd.term_hi - qd.term_lo;
    const uint32_t win_hi = min(it.win_hi, ix.n_win);
    for (uint32_t i = tid; i < 256u; i += bgk::SCAN_THREADS) S.s1[i] = ix.s1[i];
    for (uint32_t i = tid; i < sbig::CAP; i += bgk::SCAN_THREADS) S.acc[i] = 0.0;
    for (uint32_t i = tid; i < bwin::BM_WORDS; i += bgk::SCAN_THREADS) S.bm[i] = 0u;
    const uint16_t *id16 = reinterpret_cast<const uint16_t *>(ix.post_id16);
    uint32_t st_slow = 0, st_wide = 0;

    // ---- item setup (wave 0, lane t = term t): the terms' tables, first blocks and s0
    uint32_t tw = 0, fb = 0;  // (wave 0's plan registers)
    bool act = false;
    if (wave == 0) {
        act = lane < m && m <= sbig::MAX_T;
        if (act) {
            const uint32_t term = a.terms[qd.term_lo + lane];
            tw = ix.term_win[term];
            fb = ix.term_first_block[term];
            S.t_fb[lane] = fb;
            S.t_s0[lane] = ix.term_s0[term];
        }
        const bool no_table = __ballot(act && tw == NONE32) != 0ull;  // (never: the host gives this kernel queries whose terms all have one)
        if (lane == 0) S.bad = (m == 0u || m > sbig::MAX_T || no_table) ? 1u : 0u;
    }
    __syncthreads();
    if (uni(S.bad)) {
        if (tid == 0) atomicOr(a.error_flag, 8u);
        return;
    }
    const ull *filt = nullptr;
    if (a.filt_words) {
        const uint32_t sel = a.filt_sel[qd.q];
        if (sel != UINT32_MAX) filt = a.filt_words + size_t(sel) * a.filt_stride;
    }
    uint64_t *ckey = a.cand_key + qd.cand_base;
    uint32_t *cdoc = a.cand_doc + qd.cand_base;

    // wave 0's cursor over the item: the next window w; inside a window on the slow path: document cur, the width to try, the end of
    // the lane's run and its slice start at cur
    uint32_t w = it.win_lo, cur = 0, W = sbig::WIN, wo1 = 0, sa = 0, part_hi = 0;
    bool slow = false;
    auto id_at = [&](uint32_t i) { return id16[128ull * fb + i]; };
    for (;;) {
        // ---- plan (wave 0): the next tile with a posting in it
        if (wave == 0) {
            bool found = false, unfit = false;
            uint32_t ta = 0, tb = 0, ch = 0, incl = 0, g = 1, pw = 0;
            uint32_t o[bwin::MAX_G + 1u] = {};  // the lane's win_off entries of the windows w .. w + MAX_G
            while (!found && !unfit && (slow || w < win_hi)) {
                if (!slow) {
                    const uint32_t gmax = bwin::tile_windows(g_tile, win_hi - w);
#pragma unroll
                    for (uint32_t i = 0; i <= bwin::MAX_G; ++i) o[i] = act ? ix.win_off[tw + w + min(i, gmax)] : 0u;
                    uint32_t posts_all = 0;
                    auto totals = [&](uint32_t n, uint32_t &posts, uint32_t &chunks) {
                        tb = o[0];
#pragma unroll
                        for (uint32_t i = 1; i <= bwin::MAX_G; ++i) tb = i == n ? o[i] : tb;
                        ch = act ? sbig::chunks_of(o[0], tb) : 0u;
                        incl = wave_incl_scan_u32(ch);
                        posts = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(act ? tb - o[0] : 0u), 63);
                        chunks = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                        posts_all = posts;
                    };
                    g = uni(bwin::fit_windows(totals, gmax));
                    if (g) {
                        if (posts_all) {
                            found = true;
                            ta = o[0];
                            pw = w;
                        }
                        w += g;
                        continue;
                    }
                    slow = true;  // the window alone does not fit: its halves first
                    cur = w << 16;
                    part_hi = sbig::part_end(w, ix.n_docs);
                    W = sbig::WIN >> 1;
                    sa = o[0];
                    wo1 = o[1];
                }
                uint32_t tend = cur, sb = sa, posts = 0;
                for (;;) {
                    tend = sbig::tile_end(cur, W, part_hi);
                    sb = tend == part_hi || !act ? wo1 : sbig::run_lower_bound(id_at, sa, wo1, tend & (sbig::WIN - 1u));
                    ch = act ? sbig::chunks_of(sa, sb) : 0u;
                    incl = wave_incl_scan_u32(ch);
                    posts = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(act ? sb - sa : 0u), 63);
                    if (sbig::tile_fits(posts, (uint32_t)__builtin_amdgcn_readlane((int)incl, 63))) break;
                    if (W == 1u) {  // (never: one document holds at most MAX_T postings -- the index's ids ascend strictly)
                        unfit = true;
                        break;
                    }
                    W = sbig::halve(W);
                }
                if (unfit) break;
                if (posts) {
                    found = true;
                    ta = sa;
                    tb = sb;
                    g = 1;
                    pw = w;
                    ++st_slow;
                }
                cur = tend;
                sa = sb;
                W = sbig::widen(W);
                if (cur >= part_hi) {
                    slow = false;
                    ++w;
                }
            }
            if (found && act) {
                S.p_a[lane] = ta;
                S.p_b[lane] = tb;
                S.p_cb[lane] = incl - ch;
#pragma unroll
                for (uint32_t i = 0; i + 1u < bwin::MAX_G; ++i) S.p_in[lane][i] = o[i + 1u];
            }
            if (lane == 0) {
                S.p_cb[m] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                S.p_win = pw;
                S.p_g = g;
                S.p_done = found ? 0u : 1u;
                if (unfit) S.bad = 1u;
            }
        }
        __syncthreads();  // the plan, and the bitmap clean
        if (uni(S.p_done)) break;
        const uint32_t nch = uni(S.p_cb[m]), win = uni(S.p_win), g = uni(S.p_g);
        // the terms with a posting in the tile, read here: wave 0 may write the next plan while another wave is still in the sweep
        uint32_t has = 0;
        for (uint32_t tt = 0; tt < m; ++tt) has |= (S.p_cb[tt + 1u] != S.p_cb[tt] ? 1u : 0u) << tt;
        has = uni(has);

        // ---- load: the thread's chunk
        const bool own = tid < nch;
        uint32_t t = 0, mask = 0, start = 0;
        uint32_t idw[4] = {0, 0, 0, 0}, tfw[4] = {0, 0, 0, 0}, inner[bwin::INNER] = {0, 0, 0};
        if (own) {
            t = sbig::chunk_term(S.p_cb, m, tid);
            const uint32_t sl_a = S.p_a[t], sl_b = S.p_b[t];
            start = sbig::chunk_start(sl_a, S.p_cb[t], tid);
            mask = sbig::chunk_mask(start, sl_a, sl_b);
            const size_t v = 16ull * S.t_fb[t] + (start >> 3);  // (16 chunks a block; the planes are 256 bytes a block)
            const uint4 i4 = reinterpret_cast<const uint4 *>(ix.post_id16)[v];
            const uint4 f4 = reinterpret_cast<const uint4 *>(ix.post_tfn)[v];
            idw[0] = i4.x, idw[1] = i4.y, idw[2] = i4.z, idw[3] = i4.w;
            tfw[0] = f4.x, tfw[1] = f4.y, tfw[2] = f4.z, tfw[3] = f4.w;
#pragma unroll
            for (uint32_t i = 0; i + 1u < bwin::MAX_G; ++i) inner[i] = S.p_in[t][i];
        }
        // ---- mark
        uint32_t rid[sbig::CHUNK];
#pragma unroll
        for (uint32_t e = 0; e < sbig::CHUNK; ++e) {
            rid[e] = bwin::tile_id(bwin::posting_window(start + e, inner, g), sbig::chunk_id(idw, e));
            if ((mask >> e) & 1u) atomicOr(&S.bm[rid[e] >> 5], 1u << (rid[e] & 31u));
        }
        __syncthreads();
        // ---- rank: bits before every word, documents of the tile
        uint32_t n_slots;
        {
            uint32_t c[bwin::RANK_WORDS], own_c = 0;
#pragma unroll
            for (uint32_t j = 0; j < bwin::RANK_WORDS; j += 4) {
                const uint4 bw = *reinterpret_cast<const uint4 *>(&S.bm[bwin::RANK_WORDS * tid + j]);
                c[j] = sbig::popc(bw.x), c[j + 1] = sbig::popc(bw.y), c[j + 2] = sbig::popc(bw.z), c[j + 3] = sbig::popc(bw.w);
                own_c += c[j] + c[j + 1] + c[j + 2] + c[j + 3];
            }
            const uint32_t incl = wave_incl_scan_u32(own_c);
            if (lane == 63u) S.wsum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (uint32_t w2 = 0; w2 < SCAN_WAVES; ++w2) {
                const uint32_t x = S.wsum[w2];
                before += w2 < wave ? x : 0u;
                all += x;
            }
            n_slots = uni(all);
            uint32_t ex = before + incl - own_c;  // (<= CAP: 16 bits hold it)
#pragma unroll
            for (uint32_t j = 0; j < bwin::RANK_WORDS; j += 2) {
                reinterpret_cast<uint32_t *>(S.pre)[(bwin::RANK_WORDS * tid + j) >> 1] = ex | (ex + c[j]) << 16;
                ex += c[j] + c[j + 1];
            }
        }
        __syncthreads();
        uint32_t slot[sbig::CHUNK];
#pragma unroll
        for (uint32_t e = 0; e < sbig::CHUNK; ++e) {
            slot[e] = 0;
            if ((mask >> e) & 1u) slot[e] = sbig::slot_of(S.pre[rid[e] >> 5], S.bm[rid[e] >> 5], rid[e] & 31u);
        }
        // ---- add: term after term in ascending query position, a barrier behind every term that has a posting in the tile
        for (uint32_t tt = 0; tt < m; ++tt) {
            if (!((has >> tt) & 1u)) continue;
            if (own && t == tt) {
                const double s0 = S.t_s0[tt];
#pragma unroll
                for (uint32_t e = 0; e < sbig::CHUNK; ++e)
                    if ((mask >> e) & 1u) {
                        uint32_t tfv = sbig::chunk_tf(tfw, e), fn = sbig::chunk_fn(tfw, e);
                        if (bwin::wide_pair(tfw, e)) {  // rare: the posting's own field of its block, its fieldnorm from post_fn
                            const uint32_t p = start + e, j = S.t_fb[tt] + (p >> 7), i = p & 127u;
                            const uint4 bm = ix.blk_meta[j];
                            const uint32_t n = bm.w & 0xffu, md = (bm.w >> 8) & 0xffu, mt = (bm.w >> 16) & 0xffu;
                            tfv = bwin::field_at(bwin::tf_fields(ix.blob + 8ull * bm.z, md, n), mt, i);
                            fn = ix.post_fn[128ull * j + i];
                            ++st_wide;
                        }
                        const double tf = (double)tfv;
                        const double sc = (tf * s0) / (tf + S.s1[fn]);  // Cache::evaluate, bm25.rs:355-358
                        S.acc[slot[e]] = S.acc[slot[e]] + sc;
                        S.sid[slot[e]] = rid[e];
                    }
            }
            __syncthreads();  // the next term's adds see this term's sums
        }
        // ---- sweep: a thread a slot; whole waves take every round (the ballot)
        const uint32_t doc0 = win << 16;
        for (uint32_t r0 = 0; r0 < n_slots; r0 += bgk::SCAN_THREADS) {
            const uint32_t s = r0 + tid;
            ull key = 0;
            uint32_t d = 0;
            if (s < n_slots) {
                key = (ull)__double_as_longlong(S.acc[s]);
                S.acc[s] = 0.0;
                d = doc0 + S.sid[s];
                if (filt && !((filt[d >> 6] >> (d & 63u)) & 1ull)) key = 0;  // (bigk_mask_kernel's word and bit)
            }
            const ull hm = __ballot(key != 0ull);
            if (hm) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(a.cursor + it.s, (uint32_t)__popcll(hm));
                base = __shfl(base, 0);
                const uint32_t at = base + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
                if (key != 0ull) {
                    if (at < qd.cand_cap) {
                        ckey[at] = key;
                        cdoc[at] = d;
                    } else {
                        atomicOr(a.error_flag, 8u);
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < bwin::RANK_WORDS; j += 4) *reinterpret_cast<uint4 *>(&S.bm[bwin::RANK_WORDS * tid + j]) = make_uint4(0, 0, 0, 0);
    }
    if (uni(S.bad) && tid == 0) atomicOr(a.error_flag, 8u);
    if (stats) {
        if (tid == 0 && st_slow) atomicAdd(&stats[0], st_slow);
        if (st_wide) atomicAdd(&stats[1], st_wide);
    }
}

__global__ void __launch_bounds__(SELECT_THREADS) bigk_select_kernel(Args a, uint32_t s0) {
    __shared__ uint32_t s_hist[bgk::BINS];
    __shared__ uint64_t s_bkey;
    __shared__ uint32_t s_bdoc, s_need, s_levels, s_exact, s_out;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t s = s0 + blockIdx.x;
    const BigkQuery qd = a.qd[s];
    const uint32_t n = min(a.cursor[s], qd.cand_cap), k = a.k;
    const uint64_t *ckey = a.cand_key + qd.cand_base;
    const uint32_t *cdoc = a.cand_doc + qd.cand_base;
    uint64_t *okey = a.surv_key + size_t(blockIdx.x) * a.surv_stride;
    uint32_t *odoc = a.surv_doc + size_t(blockIdx.x) * a.surv_stride;
    if (n <= k) {
        for (uint32_t i = tid; i < n; i += SELECT_THREADS) {
            okey[i] = ckey[i];
            odoc[i] = cdoc[i];
        }
        if (tid == 0) a.surv_cnt[s] = n;
        return;
    }
    if (tid == 0) {
        s_bkey = 0ull;
        s_bdoc = 0xffffffffu;
        s_need = k;
        s_out = 0;
    }
    const uint32_t n_round = (n + SELECT_THREADS - 1u) / SELECT_THREADS * SELECT_THREADS;
    for (uint32_t level = 0; level < bgk::LEVELS; ++level) {
        for (uint32_t i = tid; i < bgk::BINS; i += SELECT_THREADS) s_hist[i] = 0;
        __syncthreads();
        const uint64_t bkey = s_bkey;
        const uint32_t bdoc = s_bdoc;
        for (uint32_t i = tid; i < n_round; i += SELECT_THREADS) {  // (whole waves: the ballot below)
            bool in = false;
            uint32_t d = 0;
            if (i < n) {
                const uint64_t key = ckey[i];
                const uint32_t doc = cdoc[i];
                in = bgk::same_prefix(key, doc, bkey, bdoc, level);
                d = bgk::digit(key, doc, level);
            }
            // the high digits of scores are mostly one value: the lanes that share the first live lane's digit add once
            const ull live = __ballot(in);
            if (!live) continue;
            const uint32_t first = (uint32_t)__ffsll((long long)live) - 1u;
            const uint32_t dl = __shfl(d, first);
            const ull same = __ballot(in && d == dl);
            if (lane == first) atomicAdd(&s_hist[dl], (uint32_t)__popcll(same));
            if (in && d != dl) atomicAdd(&s_hist[d], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t need = s_need, bd = s_bdoc;
            uint64_t bk = s_bkey;
            bool exact = false;
            const uint32_t d = bgk::walk_digits(s_hist, need, exact);
            bgk::set_digit(bk, bd, level, d);
            s_bkey = bk;
            s_bdoc = bd;
            s_need = need;
            s_levels = level + 1u;
            s_exact = exact ? 1u : 0u;
        }
        __syncthreads();
        if (s_exact) break;
    }
    const uint64_t bkey = s_bkey;
    const uint32_t bdoc = s_bdoc, levels = s_levels;
    for (uint32_t i = tid; i < n_round; i += SELECT_THREADS) {
        uint64_t key = 0;
        uint32_t doc = 0;
        bool keep = false;
        if (i < n) {
            key = ckey[i];
            doc = cdoc[i];
            keep = bgk::keeps(key, doc, bkey, bdoc, levels);
        }
        const ull m = __ballot(keep);
        if (!m) continue;
        uint32_t base = 0;
        if (lane == (uint32_t)__ffsll((long long)m) - 1u) base = atomicAdd(&s_out, (uint32_t)__popcll(m));
        base = __shfl(base, (int)((uint32_t)__ffsll((long long)m) - 1u));
        const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (keep) {
            if (slot < k) {
                okey[slot] = key;
                odoc[slot] = doc;
            } else {
                atomicOr(a.error_flag, 16u);
            }
        }
    }
    if (tid == 0) a.surv_cnt[s] = k;
}

// grid (tiles of k, queries of the chunk): the tile's survivors sorted best first, in place
__global__ void __launch_bounds__(SORT_THREADS) bigk_sort_kernel(Args a, uint32_t s0) {
    __shared__ uint64_t s_key[bgk::TILE];
    __shared__ uint32_t s_doc[bgk::TILE];
    const uint32_t tid = threadIdx.x;
    const uint32_t ns = min(a.surv_cnt[s0 + blockIdx.y], a.k);
    const uint32_t first = blockIdx.x * bgk::TILE;
    if (first >= ns) return;
    const uint32_t m = min(bgk::TILE, ns - first);
    uint64_t *gkey = a.surv_key + size_t(blockIdx.y) * a.surv_stride + first;
    uint32_t *gdoc = a.surv_doc + size_t(blockIdx.y) * a.surv_stride + first;
    const uint32_t sn = rrk::sort_entries(m);
    for (uint32_t i = tid; i < sn; i += SORT_THREADS) {
        s_key[i] = i < m ? gkey[i] : bgk::WORST_KEY;
        s_doc[i] = i < m ? gdoc[i] : bgk::WORST_DOC;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= sn; size <<= 1)
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t t = tid; t < sn / 2; t += SORT_THREADS) {
                uint32_t i, j;
                rrk::bitonic_pair(t, stride, i, j);
                rrk::exchange(s_key[i], s_doc[i], s_key[j], s_doc[j], rrk::bitonic_best_first(i, size));  // (better: key descending, doc ascending)
            }
            __syncthreads();
        }
    for (uint32_t i = tid; i < m; i += SORT_THREADS) {
        gkey[i] = s_key[i];
        gdoc[i] = s_doc[i];
    }
}

// grid (k in 256s, queries of the chunk)
__global__ void __launch_bounds__(EMIT_THREADS) bigk_rank_emit_kernel(DevIndex ix, Args a, uint32_t s0) {
    const uint32_t s = s0 + blockIdx.y;
    const uint32_t q = a.qd[s].q;
    const uint32_t ns = min(a.surv_cnt[s], a.k);
    const uint32_t i = blockIdx.x * EMIT_THREADS + threadIdx.x;
    if (i == 0) a.n_hits[q] = ns;
    if (i >= ns) return;
    const uint64_t *keys = a.surv_key + size_t(blockIdx.y) * a.surv_stride;
    const uint32_t *docs = a.surv_doc + size_t(blockIdx.y) * a.surv_stride;
    const uint64_t key = keys[i];
    const uint32_t d = docs[i];
    const uint32_t mine = i / bgk::TILE, n_tiles = (ns + bgk::TILE - 1u) / bgk::TILE;
    uint32_t rank = i % bgk::TILE;
    for (uint32_t u = 0; u < n_tiles; ++u)
        if (u != mine) rank += bgk::count_beating(keys + u * bgk::TILE, docs + u * bgk::TILE, min(bgk::TILE, ns - u * bgk::TILE), key, d);
    if (rank >= ns) {  // (the order is strict: cannot be)
        atomicOr(a.error_flag, 32u);
        return;
    }
    const uint16_t *pl = ix.doc_payload + 3ull * d;
    ull *out = reinterpret_cast<ull *>(a.hits + size_t(q) * a.k + rank);
    out[0] = key;
    out[1] = (ull)d | (ull)pl[0] << 32 | (ull)pl[1] << 48;
    out[2] = (ull)pl[2];
}

}  // namespace

// The scratch of the sparse path, sized once when the batch is made.  bigk_chunk_cand entries of candidates a chunk (12 bytes each;
// no more than max_queries queries of bigk_cand_max entries, or of all the index's postings, can ask for), and k rounded up to tiles
// for each of the chunk's queries in the survivor buffers.
int bigk_create(vbm25_batch *bt) {
    BigkState &g = bt->bg;
    g.on = bt->tune.bigk_sparse != 0;
    if (!g.on) return VBM25_OK;
    const vbm25_index *ix = bt->index;
    uint64_t postings = 0;
    for (uint32_t df : ix->term_df_host) postings += df;
    const uint64_t chunk = std::max<uint64_t>(1, bt->tune.bigk_chunk_cand);
    g.cand_max = std::min<uint64_t>(std::min<uint64_t>(bt->tune.bigk_cand_max, chunk), std::max<uint64_t>(postings, 1));
    g.chunk_cand = std::min<uint64_t>(chunk, std::max<uint64_t>(1, uint64_t(bt->max_queries) * g.cand_max));
    g.surv_stride = (bt->k + bgk::TILE - 1u) / bgk::TILE * bgk::TILE;
    g.chunk_q = (uint32_t)std::min<uint64_t>(bt->max_queries, std::max<uint64_t>(1, BIGK_SURV_ENTRIES / g.surv_stride));
    g.max_items = std::max<uint64_t>(4096, 4ull * bt->max_queries);
    // the dense half's gate.  A dense query's segment: bigk_dense_seg entries, no more than its postings can fill, never below k
    // rounded up to tiles (the emit scan brings at least k whenever there are k), and the chunk's scratch holds at least one
    g.dense_on = bt->tune.bigk_dense != 0 && ix->n_docs >= bt->tune.bigk_dense_min_docs;
    if (g.dense_on) {
        const uint64_t room = std::max<uint64_t>(chunk, g.surv_stride);
        g.dense_seg = (uint32_t)std::min<uint64_t>(room, std::max<uint64_t>(g.surv_stride, std::min<uint64_t>(bt->tune.bigk_dense_seg, postings)));
        g.chunk_cand = std::min<uint64_t>(room, std::max<uint64_t>(1, uint64_t(bt->max_queries) * std::max<uint64_t>(g.cand_max, g.dense_seg)));
        g.dense_chunk_q = (uint32_t)std::min<uint64_t>(g.chunk_q, std::max<uint64_t>(1, g.chunk_cand / g.surv_stride));
    }
    int rc = 0;
    if (g.dense_on && ((rc = g.dstate.alloc(sizeof(bgd::State) * size_t(bt->max_queries))) ||
                       (rc = g.dhist.alloc(4ull * bgd::BINS * g.dense_chunk_q))))
        return rc;
    if ((rc = g.cand_key.alloc(8 * g.chunk_cand)) || (rc = g.cand_doc.alloc(4 * g.chunk_cand)) ||
        (rc = g.surv_key.alloc(8ull * g.chunk_q * g.surv_stride)) || (rc = g.surv_doc.alloc(4ull * g.chunk_q * g.surv_stride)) ||
        (rc = g.cursor.alloc(4ull * (BIGK_STAT_WORDS + bt->max_queries))) || (rc = g.surv_cnt.alloc(4ull * bt->max_queries)) ||
        (rc = g.sel.alloc(4ull * bt->max_queries)) || (rc = g.qd.alloc(sizeof(BigkQuery) * size_t(bt->max_queries))) ||
        (rc = g.terms.alloc(4ull * std::max(bt->max_terms, 1u))) || (rc = g.items.alloc(sizeof(BigkItem) * g.max_items * (g.dense_on ? 2u : 1u))))  // (the dense queries' items: max_items of their own)
        return rc;
    g.sparse.assign(bt->max_queries, 0);
    // the window scan's gate: the switch, the index's size, and the planes the kernel reads
    g.win_on = bt->tune.bigk_win != 0 && ix->n_docs >= bt->tune.bigk_win_min_docs && ix->dev.post_id16 && ix->dev.win_off &&
               ix->dev.term_win && ix->dev.post_tfn && !ix->term_win_host.empty();
    g.win_tile = bwin::tile_windows(bt->tune.bigk_win_tile ? bt->tune.bigk_win_tile : bwin::MAX_G, bwin::MAX_G);
    g.h_win.reserve(bt->max_queries);
    g.h_qd.reserve(bt->max_queries);
    g.h_terms.reserve(bt->max_terms);
    return VBM25_OK;
}

// set_queries: which queries are sparse, their chunks and their work items, and the descriptors to the device.  (bt->h_terms / h_off hold
// the queries.)  The descriptors go up with synchronous copies, as the queries of every batch that is not staged do: a k > 1024 batch
// never is (stream.hip submits it with fast = false and runs it on the null stream), so the ring's k > 1024 step, which was
// synchronous before, stays so.
int bigk_plan(vbm25_batch *bt) {
    BigkState &g = bt->bg;
    g.n_sparse = g.n_dense = 0;
    g.chunks.clear();
    if (!g.on) return VBM25_OK;
    const vbm25_index *ix = bt->index;
    const uint32_t nq = uint32_t(bt->h_off.size()) - 1u;
    g.h_qd.clear();
    g.h_terms.clear();
    g.h_items.clear();
    std::fill(g.sparse.begin(), g.sparse.end(), uint8_t(0));
    g.h_win.clear();
    g.items_win = g.items_blk = 0;
    uint32_t n_scanned = 0, n_scanned_win = 0;  // sparse queries with a posting, by scan kernel: the others make no item
    // the descriptor of query q with its indexed terms that have postings, in query order; whether every one has a window table
    auto describe = [&](uint32_t q, bool &tables) {
        BigkQuery d{};
        d.q = q;
        d.term_lo = uint32_t(g.h_terms.size());
        for (uint32_t p = bt->h_off[q]; p < bt->h_off[q + 1]; ++p)
            if (bt->h_terms[p] < ix->n_terms && ix->term_df_host[bt->h_terms[p]]) {  // search.rs:59-61
                g.h_terms.push_back(bt->h_terms[p]);
                tables = tables && g.win_on && ix->term_win_host[bt->h_terms[p]] != UINT32_MAX;
            }
        d.term_hi = uint32_t(g.h_terms.size());
        return d;
    };
    for (uint32_t q = 0; q < nq; ++q) {
        if (bt->h_postings[q] > g.cand_max) continue;
        g.sparse[q] = 1;
        bool tables = true;
        BigkQuery d = describe(q, tables);
        d.cand_cap = uint32_t(bt->h_postings[q]);
        // the window scan's queries: 1 .. 16 indexed terms, every one with a window table
        const bool win = g.win_on && tables && d.term_hi > d.term_lo && d.term_hi - d.term_lo <= sbig::MAX_T;
        (win ? n_scanned_win : n_scanned) += d.cand_cap != 0;
        g.h_win.push_back(win ? 1 : 0);
        g.h_qd.push_back(d);
    }
    g.n_sparse = uint32_t(g.h_qd.size());
    // the dense queries behind them: batched too (g.sparse says "not the per-query path"), their descriptors behind the sparse ones
    for (uint32_t q = 0; g.dense_on && q < nq; ++q) {
        if (g.sparse[q]) continue;
        g.sparse[q] = 1;
        bool tables = true;
        BigkQuery d = describe(q, tables);
        d.cand_cap = (uint32_t)std::min<uint64_t>(g.dense_seg, std::max<uint64_t>(g.surv_stride, bt->h_postings[q]));
        g.h_qd.push_back(d);
    }
    g.n_dense = uint32_t(g.h_qd.size()) - g.n_sparse;
    if (g.h_qd.empty()) return VBM25_OK;
    // the item cuts, per scan kernel over its own windows; with both kinds in the batch each gets half the item buffer
    const uint64_t cap = n_scanned && n_scanned_win ? g.max_items / 2 : g.max_items;
    const uint32_t n_win = (ix->n_docs + bgk::WINDOW - 1u) / bgk::WINDOW, n_win16 = ix->dev.n_win;
    const uint32_t wpi = bgk::item_windows(n_win, n_scanned, bt->tune.bigk_item_win, ITEM_TARGET, cap);
    const uint32_t wpi16 = bgk::item_windows(n_win16, n_scanned_win, bt->tune.bigk_item_win, ITEM_TARGET, cap);
    g.wpi = wpi;
    // chunks: queries in order while their candidate segments fit the scratch and their survivors the survivor buffers; a chunk's
    // items the window scan's first, then the block scan's: one launch of each
    for (uint32_t s = 0; s < g.n_sparse;) {
        BigkChunk c{};
        c.s0 = s;
        c.item0 = uint32_t(g.h_items.size());
        uint64_t used = 0;
        while (s < g.n_sparse && s - c.s0 < g.chunk_q && used + g.h_qd[s].cand_cap <= g.chunk_cand) {
            g.h_qd[s].cand_base = uint32_t(used);
            used += g.h_qd[s].cand_cap;
            ++s;
        }
        if (s == c.s0) return set_error(VBM25_ERR_INVALID, "internal error: a sparse query exceeds the candidate scratch");
        c.s1 = s;
        for (uint32_t i = c.s0; i < c.s1; ++i)
            if (g.h_win[i] && g.h_qd[i].cand_cap)
                for (uint32_t w = 0; w < n_win16; w += wpi16) g.h_items.push_back(BigkItem{i, w, std::min(w + wpi16, n_win16)});
        c.item_mid = uint32_t(g.h_items.size());
        for (uint32_t i = c.s0; i < c.s1; ++i)
            if (!g.h_win[i] && g.h_qd[i].cand_cap)
                for (uint32_t w = 0; w < n_win; w += wpi) g.h_items.push_back(BigkItem{i, w, std::min(w + wpi, n_win)});
        c.item1 = uint32_t(g.h_items.size());
        g.items_win += c.item_mid - c.item0;
        g.items_blk += c.item1 - c.item_mid;
        g.chunks.push_back(c);
    }
    if (g.h_items.size() > g.max_items) return set_error(VBM25_ERR_INVALID, "internal error: %zu work items exceed the buffer", g.h_items.size());
    // the dense chunks: queries in order while their segments fit the scratch, their survivors the survivor buffers and their
    // histograms the rows; then the items -- cut for ITEM_TARGET items a chunk (a chunk is a launch), all of them within max_items
    const size_t first_dense_chunk = g.chunks.size(), sparse_items = g.h_items.size();
    uint32_t most = 0;
    for (uint32_t s = g.n_sparse, end = g.n_sparse + g.n_dense; s < end;) {
        BigkChunk c{};
        c.dense = true;
        c.s0 = s;
        uint64_t used = 0;
        while (s < end && s - c.s0 < g.dense_chunk_q && used + g.h_qd[s].cand_cap <= g.chunk_cand) {
            g.h_qd[s].cand_base = uint32_t(used);
            used += g.h_qd[s].cand_cap;
            ++s;
        }
        if (s == c.s0) return set_error(VBM25_ERR_INVALID, "internal error: a dense query exceeds the candidate scratch");
        c.s1 = s;
        most = std::max(most, c.s1 - c.s0);
        g.chunks.push_back(c);
    }
    if (g.n_dense) {
        const uint32_t wpd = bgk::item_windows(n_win, most, bt->tune.bigk_item_win, ITEM_TARGET, uint64_t(most) * (g.max_items / g.n_dense));
        for (size_t ci = first_dense_chunk; ci < g.chunks.size(); ++ci) {
            BigkChunk &c = g.chunks[ci];
            c.item0 = c.item_mid = uint32_t(g.h_items.size());
            for (uint32_t i = c.s0; i < c.s1; ++i)
                for (uint32_t w = 0; w < n_win; w += wpd) g.h_items.push_back(BigkItem{i, w, std::min(w + wpd, n_win)});
            c.item1 = uint32_t(g.h_items.size());
        }
        if (g.h_items.size() - sparse_items > g.max_items)
            return set_error(VBM25_ERR_INVALID, "internal error: %zu work items of dense queries exceed the buffer", g.h_items.size() - sparse_items);
    }
    HIP_TRY(hipMemcpy(g.qd.p, g.h_qd.data(), sizeof(BigkQuery) * g.h_qd.size(), hipMemcpyHostToDevice));
    if (!g.h_terms.empty()) HIP_TRY(hipMemcpy(g.terms.p, g.h_terms.data(), 4ull * g.h_terms.size(), hipMemcpyHostToDevice));
    if (!g.h_items.empty()) HIP_TRY(hipMemcpy(g.items.p, g.h_items.data(), sizeof(BigkItem) * g.h_items.size(), hipMemcpyHostToDevice));
    return VBM25_OK;
}

// the batched queries of the current set, on st: one clear, then four launches a sparse chunk; a dense chunk: its histograms cleared,
// every level's scan and walk whether a query still needs it or not (the host does not wait to know: a level nobody needs is two
// grids that return at once), the emit scan and the same three launches
int bigk_run(vbm25_batch *bt, hipStream_t st) {
    BigkState &g = bt->bg;
    g.ran = false;
    g.ran_dense = 0;
    const uint32_t n_batched = g.n_sparse + g.n_dense;
    if (!n_batched) return VBM25_OK;
    const DevIndex &dix = bt->index->dev;
    Args a{};
    a.qd = g.qd.as<BigkQuery>();
    a.items = g.items.as<BigkItem>();
    a.terms = g.terms.as<uint32_t>();
    uint32_t *stats = g.cursor.as<uint32_t>();  // (the window scan's counters, then the cursors)
    a.cursor = stats + BIGK_STAT_WORDS;
    a.surv_cnt = g.surv_cnt.as<uint32_t>();
    a.cand_key = g.cand_key.as<uint64_t>();
    a.cand_doc = g.cand_doc.as<uint32_t>();
    a.surv_key = g.surv_key.as<uint64_t>();
    a.surv_doc = g.surv_doc.as<uint32_t>();
    a.k = bt->k;
    a.surv_stride = g.surv_stride;
    a.hits = bt->hits.as<vbm25_hit>();
    a.n_hits = bt->n_hits.as<uint32_t>();
    a.error_flag = bt->error_flag.as<uint32_t>();
    if (bt->filt_on) {  // (the selectors may have been set since set_queries: they go up with every run)
        HIP_TRY(hipMemcpyAsync(g.sel.p, bt->h_filt_sel.data(), 4ull * bt->nq, hipMemcpyHostToDevice, st));
        a.filt_words = bt->filter->bits.as<ull>();
        a.filt_sel = g.sel.as<uint32_t>();
        a.filt_stride = bt->filter->words;
    }
    bigk_clear_kernel<<<(BIGK_STAT_WORDS + n_batched + 255) / 256, 256, 0, st>>>(stats, BIGK_STAT_WORDS + n_batched);
    BigkDenseArgs da{};
    if (g.n_dense) {
        da.qd = a.qd, da.items = a.items, da.terms = a.terms, da.cursor = a.cursor, da.cand_key = a.cand_key, da.cand_doc = a.cand_doc;
        da.filt_words = a.filt_words, da.filt_sel = a.filt_sel, da.filt_stride = a.filt_stride;
        da.k = a.k;
        da.d0 = g.n_sparse;
        da.state = g.dstate.as<bgd::State>();
        da.hist = g.dhist.as<uint32_t>();
        da.stats = stats + 2;
        da.error_flag = a.error_flag;
        bigk_dense_init_kernel<<<(g.n_dense + 255) / 256, 256, 0, st>>>(dix, da, g.n_dense);
    }
    const uint32_t k_tiles = g.surv_stride / bgk::TILE;
    for (const BigkChunk &c : g.chunks) {
        const uint32_t cq = c.s1 - c.s0;
        if (c.dense) {
            const uint32_t items = c.item1 - c.item0;
            bigk_clear_kernel<<<std::min<uint32_t>((cq * bgd::BINS + 255) / 256, 1024u), 256, 0, st>>>(da.hist, cq * bgd::BINS);
            for (uint32_t level = 0; level < bgd::MAX_LEVELS; ++level) {
                bigk_dense_scan_kernel<false><<<items, bgk::SCAN_THREADS, 0, st>>>(dix, da, c.item0, c.s0);
                bigk_dense_walk_kernel<<<cq, bgd::WALK_THREADS, 0, st>>>(da, c.s0);
            }
            bigk_dense_scan_kernel<true><<<items, bgk::SCAN_THREADS, 0, st>>>(dix, da, c.item0, c.s0);
        }
        if (!c.dense && c.item_mid > c.item0) bigk_scan_win_kernel<<<c.item_mid - c.item0, bgk::SCAN_THREADS, 0, st>>>(dix, a, c.item0, g.win_tile, stats);
        if (!c.dense && c.item1 > c.item_mid) bigk_scan_kernel<<<c.item1 - c.item_mid, bgk::SCAN_THREADS, 0, st>>>(dix, a, c.item_mid);
        bigk_select_kernel<<<cq, SELECT_THREADS, 0, st>>>(a, c.s0);
        bigk_sort_kernel<<<dim3(k_tiles, cq), SORT_THREADS, 0, st>>>(a, c.s0);
        bigk_rank_emit_kernel<<<dim3((bt->k + EMIT_THREADS - 1) / EMIT_THREADS, cq), EMIT_THREADS, 0, st>>>(dix, a, c.s0);
    }
    HIP_TRY(hipGetLastError());
    g.ran_items_win = g.items_win;
    g.ran_items_blk = g.items_blk;
    g.ran_d0 = g.n_sparse;
    g.ran_dense = g.n_dense;
    g.ran = true;
    return VBM25_OK;
}

// vbm25_batch_debug_bigk_win: the last run's items by scan kernel (the host's cut) and the window scan's two device counters
int bigk_debug_win(vbm25_batch *bt, uint32_t *out4) {
    BigkState &g = bt->bg;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!g.on || !g.ran || !g.n_sparse) return VBM25_OK;
    out4[0] = g.ran_items_win;
    out4[1] = g.ran_items_blk;
    HIP_TRY(hipMemcpy(out4 + 2, g.cursor.p, 8, hipMemcpyDeviceToHost));
    return VBM25_OK;
}

// vbm25_batch_debug_bigk_dense: the dense queries batched in the last run, the highest level any of them needed plus one, the queries
// whose level-0 boundary was the clip bin, and the candidates their emit scans listed (the sum of their cursors)
int bigk_debug_dense(vbm25_batch *bt, uint32_t *out4) {
    BigkState &g = bt->bg;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!g.on || !g.ran || !g.ran_dense) return VBM25_OK;
    out4[0] = g.ran_dense;
    HIP_TRY(hipMemcpy(out4 + 1, g.cursor.as<uint32_t>() + 2, 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> cur(g.ran_dense);
    HIP_TRY(hipMemcpy(cur.data(), g.cursor.as<uint32_t>() + BIGK_STAT_WORDS + g.ran_d0, 4ull * g.ran_dense, hipMemcpyDeviceToHost));
    uint64_t sum = 0;
    for (uint32_t c : cur) sum += c;
    out4[3] = (uint32_t)std::min<uint64_t>(sum, UINT32_MAX);
    return VBM25_OK;
}

// ---------------------------------------------------------------------------
// The growing segment's part of a k > 1024 run, batched (growing_bigk.h; switch bigk_grow).  It serves every query of the batch,
// whichever sealed path the query took, and does not depend on bigk_sparse: the scratch below is its own.
// ---------------------------------------------------------------------------
// The scratch for a segment of n_grow documents: candidate entries for a chunk (bigk_chunk_cand, no more than max_queries queries of
// n_grow candidates can ask for, never less than one query's n_grow), survivor rows within BIGK_SURV_ENTRIES, cursors, descriptors.
// No run of the batch may be in flight.
int growing_bigk_scratch(vbm25_batch *bt, uint32_t n_grow) {
    GrowBigkState &g = bt->gb;
    const uint64_t n = std::max<uint64_t>(std::max(n_grow, bt->gr_n), 1), mq = std::max(bt->max_queries, 1u);
    g.surv_stride = (bt->k + bgk::TILE - 1u) / bgk::TILE * bgk::TILE;
    g.chunk_q = (uint32_t)std::min<uint64_t>(mq, std::max<uint64_t>(1, BIGK_SURV_ENTRIES / g.surv_stride));
    g.chunk_cand = std::max<uint64_t>(n, std::min<uint64_t>(std::max<uint64_t>(1, bt->tune.bigk_chunk_cand), mq * n));
    int rc = 0;
    if ((rc = batch_grow_buffer(g.cand_key, 8 * g.chunk_cand)) || (rc = batch_grow_buffer(g.cand_doc, 4 * g.chunk_cand)) ||
        (rc = batch_grow_buffer(g.surv_key, 8ull * g.chunk_q * g.surv_stride)) || (rc = batch_grow_buffer(g.surv_doc, 4ull * g.chunk_q * g.surv_stride)) ||
        (rc = batch_grow_buffer(g.cursor, 4ull * (BIGK_STAT_WORDS + mq))) || (rc = batch_grow_buffer(g.surv_cnt, 4ull * mq)) ||
        (rc = batch_grow_buffer(g.sel, 4ull * mq)) || (rc = batch_grow_buffer(g.qd, sizeof(BigkQuery) * size_t(mq))) ||
        (rc = batch_grow_buffer(g.terms, 4ull * std::max(bt->max_terms, 1u))))
        return rc;
    g.h_qd.reserve(mq);
    g.h_terms.reserve(bt->max_terms);
    g.h_cap.reserve(mq);
    g.h_base.reserve(mq);
    g.h_chunk.reserve(mq + 1);
    bt->gr_n = uint32_t(n);
    return VBM25_OK;
}

// on st behind the sealed scan and the copy of its records: the descriptors, one clear, four launches a chunk
int growing_bigk_run(vbm25_batch *bt, const vbm25_hit *sealed, const uint32_t *sealed_cnt, hipStream_t st) {
    GrowBigkState &g = bt->gb;
    const vbm25_device_growing *gs = bt->growing;
    const uint32_t nq = bt->nq, n_terms = bt->index->n_terms;
    g.ran = false;
    if (!nq) return VBM25_OK;
    // a query's terms and capacity from the segment's postings of the moment (it may have been appended to since set_queries; the
    // batch's queries are on the host only), then the chunks
    g.h_qd.resize(nq);
    g.h_cap.resize(nq);
    g.h_base.resize(nq);
    g.h_chunk.clear();
    g.h_terms.clear();
    for (uint32_t q = 0; q < nq; ++q) {
        uint64_t postings = 0;
        g.h_qd[q].term_lo = uint32_t(g.h_terms.size());
        for (uint32_t p = bt->h_off[q]; p < bt->h_off[q + 1]; ++p) {
            const uint32_t t = bt->h_terms[p];
            const uint32_t df = t < n_terms ? gs->term_start_host[t + 1] - gs->term_start_host[t] : 0u;
            if (df) g.h_terms.push_back(t);
            postings += df;
        }
        g.h_qd[q].term_hi = uint32_t(g.h_terms.size());
        g.h_cap[q] = gbk::query_cap(gs->n_grow, postings);
    }
    for (uint32_t q = 0; q < nq;) {
        const uint32_t q1 = gbk::chunk_end(g.h_cap.data(), nq, q, g.chunk_q, g.chunk_cand, g.h_base.data());
        if (q1 == q) return set_error(VBM25_ERR_INVALID, "internal error: a query's growing candidates exceed the scratch");
        g.h_chunk.push_back(q);
        q = q1;
    }
    g.h_chunk.push_back(nq);
    for (uint32_t q = 0; q < nq; ++q) g.h_qd[q] = BigkQuery{q, g.h_qd[q].term_lo, g.h_qd[q].term_hi, g.h_base[q], g.h_cap[q]};
    HIP_TRY(hipMemcpyAsync(g.qd.p, g.h_qd.data(), sizeof(BigkQuery) * size_t(nq), hipMemcpyHostToDevice, st));
    if (!g.h_terms.empty()) HIP_TRY(hipMemcpyAsync(g.terms.p, g.h_terms.data(), 4ull * g.h_terms.size(), hipMemcpyHostToDevice, st));
    const DevGrowing G = gs->dev();
    uint32_t *stats = g.cursor.as<uint32_t>();  // (the two counters, then the cursors: one clear covers both)
    GrowBigkArgs ga{};
    ga.qd = g.qd.as<BigkQuery>();
    ga.terms = g.terms.as<uint32_t>();
    ga.cursor = stats + BIGK_STAT_WORDS;
    ga.stats = stats;
    ga.cand_key = g.cand_key.as<uint64_t>();
    ga.cand_doc = g.cand_doc.as<uint32_t>();
    if (bt->filt_on) {  // (batch_run_growing_impl checked that the growing bitmaps are this segment's)
        HIP_TRY(hipMemcpyAsync(g.sel.p, bt->h_filt_sel.data(), 4ull * nq, hipMemcpyHostToDevice, st));
        ga.filt_words = bt->filter->grow_bits.as<uint32_t>();
        ga.filt_sel = g.sel.as<uint32_t>();
        ga.filt_stride = 2u * bt->filter->grow_stride;
    }
    ga.sealed = sealed;
    ga.sealed_cnt = sealed_cnt;
    ga.surv_cnt = g.surv_cnt.as<uint32_t>();
    ga.surv_key = g.surv_key.as<uint64_t>();
    ga.surv_doc = g.surv_doc.as<uint32_t>();
    ga.k = bt->k;
    ga.surv_stride = g.surv_stride;
    ga.hits = bt->hits.as<vbm25_hit>();
    ga.n_hits = bt->n_hits.as<uint32_t>();
    ga.error_flag = bt->error_flag.as<uint32_t>();
    Args a{};  // the select's and the sort's view of the same scratch
    a.qd = ga.qd;
    a.cursor = ga.cursor;
    a.surv_cnt = g.surv_cnt.as<uint32_t>();
    a.cand_key = ga.cand_key;
    a.cand_doc = ga.cand_doc;
    a.surv_key = g.surv_key.as<uint64_t>();
    a.surv_doc = g.surv_doc.as<uint32_t>();
    a.k = bt->k;
    a.surv_stride = g.surv_stride;
    a.error_flag = ga.error_flag;
    bigk_clear_kernel<<<(BIGK_STAT_WORDS + nq + 255) / 256, 256, 0, st>>>(stats, BIGK_STAT_WORDS + nq);
    const uint32_t k_tiles = g.surv_stride / bgk::TILE;
    uint32_t items = 0;
    for (size_t c = 0; c + 1 < g.h_chunk.size(); ++c) {
        const uint32_t q0 = g.h_chunk[c], cq = g.h_chunk[c + 1] - q0;
        const uint32_t ipq = gbk::items_per_query(G.n_tiles, cq, gbk::ITEM_TARGET);
        growing_bigk_scan_kernel<<<cq * ipq, GWG, 0, st>>>(G, ga, q0, ipq);
        bigk_select_kernel<<<cq, SELECT_THREADS, 0, st>>>(a, q0);
        bigk_sort_kernel<<<dim3(k_tiles, cq), SORT_THREADS, 0, st>>>(a, q0);
        growing_bigk_merge_kernel<<<dim3((bt->k + 255) / 256, cq), 256, 0, st>>>(G, ga, q0);
        items += cq * ipq;
    }
    HIP_TRY(hipGetLastError());
    g.ran_items = items;
    g.ran_chunks = uint32_t(g.h_chunk.size()) - 1u;
    g.ran = true;
    return VBM25_OK;
}

// vbm25_batch_debug_bigk_grow: the last run's work items of the growing scan, its two device counters and the chunks
int growing_bigk_debug(vbm25_batch *bt, uint32_t *out4) {
    GrowBigkState &g = bt->gb;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!g.ran) return VBM25_OK;
    out4[0] = g.ran_items;
    HIP_TRY(hipMemcpy(out4 + 1, g.cursor.p, 8, hipMemcpyDeviceToHost));
    out4[3] = g.ran_chunks;
    return VBM25_OK;
}

}  // namespace vbm25
