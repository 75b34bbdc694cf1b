// scan_sparse_big.h -- scan_sparse_big_kernel: SPARSE queries (postings < 0.1 N) of 1 .. 16 indexed terms at 256 < k <= 1024, every
// term with a window table.  The rank-addressed window scan; compiled in its own unit (scan_sparse_big.hip), launched by search.hip's
// general route between plan_kernel and scan_many_kernel.  sparse_big_lane.h has the per-lane functions.
//
// One workgroup of dlist::WAVES = 8 waves per work item (the items plan_kernel marks ITEM_SPARSE_BIG), persistent, items drawn longest
// first through item_order from bt.work_ctr[0] (scan_range_kernel's counter: that kernel does not run at k > 256).  The item's
// documents [doc_lo, doc_hi) are taken window by window (2^16 documents); every posting in them is scored exactly -- nothing is
// skipped, there is no upper bound anywhere -- but nothing of what scan_many_kernel spends on such an item is done:
//   no block decode   ids come from post_id16 (a term's postings of a window are one contiguous run of 16-bit ids, addressed by
//                     win_off), tf and fieldnorm from post_tfn
//   no hash, no CAS   a document's accumulator slot is its RANK in the window's bitmap
//   no serial top-k   every wave appends survivors to one list, all eight waves cut it (dense_list_lane.h: scan_dense_kernel<1024>'s)
//
// A TILE is a window, or a power-of-two aligned part of one, whose slices hold at most CAP = 4096 postings in at most 512 chunks of 8.
// Wave 0 plans it, lane t = term t.  FAST PATH: the tile is the whole window -- the slices are the runs, read from win_off.  SLOW
// PATH (the item's edge windows, and any window with more postings or chunks than a tile holds): the lane bisects its run for the
// tile's bounds, and the width halves while the tile does not fit; width 1 always does.  Empty tiles are passed over by wave 0 alone.
//   load   thread c owns chunk c: one 16-byte load of 8 ids and one of 8 (tf, tf, fieldnorm, fieldnorm) bytes, both issued here.  The
//          ids stay in the thread's registers to the end of the tile; the tf words are first looked at in the add phase.
//   mark   every posting sets its document's bit in the window's bitmap (LDS atomic or, no return).  Barrier.
//   rank   every thread counts the bits of four bitmap words; a workgroup exclusive scan (wave scan + one LDS hop) gives every word
//          the number of bits before it and the tile its number of documents n_slots <= CAP.  A posting's slot is that prefix + the
//          bits below its own in its word.  Two barriers.
//   add    term after term in ascending query order: the threads of term t add (tf s0) / (tf + s1[fieldnorm]) -- f64, no contraction
//          -- to acc[slot].  A term has one posting per document: no atomics.  A barrier closes the phase, so every sum is formed in
//          key order (0.0 + x is exact): the scores are bit for bit the other kernels'.  A term without a posting in the tile is
//          passed over by the whole workgroup, barrier included.  A zero tf byte means "wider than a byte": the ITEM is given up
//          (item_failed: scan_many_kernel redoes it).
//   sweep  one thread per slot in rounds of ROUND = 1024 slots: a sum the threshold does not strictly beat, of a document the query's
//          filter keeps, is appended to the survivor list (one LDS atomic per wave, ballot ranks); the accumulator is cleared on the
//          way, the bitmap after the last round.  Behind every round with the cursor past k: the CUT -- eight-wave bitonic sort, the
//          first k stay, the k-th key is the workgroup's threshold and goes to bt.theta[q].
// THE LIST CANNOT OVERFLOW: a cut leaves at most k <= 1024 entries, a round without a cut was entered with at most k, a round
// appends at most ROUND = 1024, and 1024 + 1024 = dlist::CAP.  There is no give-up for that reason (the store is guarded all the same).
// The query's shared threshold is polled once per tile.  Item end: a last cut (the sort), then res_score / res_doc / res_cnt with
// lpi = 1 as scan_dense_kernel<1024> writes them; merge_kernel merges.
#ifndef VBM25_SCAN_SPARSE_BIG_H
#define VBM25_SCAN_SPARSE_BIG_H

#include "device_types.h"
#include "block_fetch.h"
#include "topk_reg.h"
#include "sparse_big_lane.h"

namespace vbm25 {

constexpr int SBWG = (int)sbig::THREADS;
constexpr uint32_t SB_GRID = 512;      // persistent workgroups: 256 CUs x 2 (80 KB of LDS each)
constexpr uint32_t SB_FAILED = 0x181u;  // item_failed of an item given up for a term frequency wider than a byte

struct SparseBigLds {
    double acc[sbig::CAP];                  // 32 KB: a slot's score, zero between tiles
    unsigned long long key[dlist::CAP];     // 16 KB + 8 KB: the survivor list
    uint32_t doc[dlist::CAP];
    uint32_t bm[sbig::BM_WORDS];            // 8 KB: the window's bitmap, zero between tiles
    uint16_t pre[sbig::BM_WORDS];           // 4 KB: bits set before every word
    uint16_t sid[sbig::CAP];                // 8 KB: a slot's 16-bit id
    double s1[256];
    double t_s0[sbig::MAX_T];
    uint32_t t_tw[sbig::MAX_T], t_fb[sbig::MAX_T];  // the term's table in win_off, its first block (post_id16 / post_tfn: 64 words a block)
    uint32_t p_a[sbig::MAX_T], p_b[sbig::MAX_T], p_cb[sbig::MAX_T + 1];  // the tile's plan: slices and chunk prefix
    uint32_t wsum[dlist::WAVES];
    uint32_t scratch[64];
    unsigned long long theta;               // bits of a lower bound of the query's k-th best score
    uint32_t cur;                           // entries of the survivor list
    uint32_t item, m, fail, p_win, p_done;
};

// stats (vbm25_batch_debug_sparse_big): [0] items taken, [1] items given up for a wide tf, [2] tiles on the slow path, [3] cuts
__global__ void __launch_bounds__(SBWG, 4) scan_sparse_big_kernel(DevIndex ix, DevBatch bt, uint32_t *stats) {
    __shared__ SparseBigLds S;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);
    const uint32_t k = bt.k;
    const uint32_t n_items = *cold_args()->bt.n_items;
    for (uint32_t i = tid; i < 256u; i += SBWG) S.s1[i] = ix.s1[i];
    for (uint32_t i = tid; i < sbig::CAP; i += SBWG) S.acc[i] = 0.0;
    for (uint32_t i = tid; i < sbig::BM_WORDS; i += SBWG) S.bm[i] = 0u;
    uint32_t st_items = 0, st_given = 0, st_slow = 0, st_cuts = 0;  // (thread 0's)
    const uint16_t *id16 = reinterpret_cast<const uint16_t *>(ix.post_id16);
    uint32_t q = 0;  // the item's query

    // ---- the cut of the survivor list (scan_dense_kernel<1024>'s loop over dense_list_lane.h): called by all eight waves behind a
    // barrier with no append in flight; ends with a barrier
    auto list_cut = [&]() {
        const uint32_t live = min(uni(S.cur), dlist::CAP);
        const uint32_t n = dlist::sort_entries(live), ppw = dlist::wave_pairs(n);
        for (uint32_t i = live + tid; i < n; i += SBWG) {
            S.key[i] = dlist::PAD_KEY;
            S.doc[i] = dlist::PAD_DOC;
        }
        bool wide_before = true;  // (the padding is other waves')
        for (uint32_t size = 2; size <= n; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                const bool local = dlist::stage_local(stride, n);
                if (!local || wide_before) lds_barrier();
                else __builtin_amdgcn_wave_barrier();  // (the wave's own entries: its LDS operations complete in order)
                wide_before = !local;
                for (uint32_t p = lane; p < ppw; p += 64) {
                    uint32_t i, j;
                    bool best_first;
                    dlist::wave_pair(wave, p, n, size, stride, i, j, best_first);
                    const unsigned long long ka0 = S.key[i], kb0 = S.key[j];
                    const uint32_t da0 = S.doc[i], db0 = S.doc[j];
                    uint64_t ka = ka0, kb = kb0;
                    uint32_t da = da0, db = db0;
                    rrk::exchange(ka, da, kb, db, best_first);
                    if (ka != ka0 || da != da0) {  // swapped (two entries never hold the same document)
                        S.key[i] = ka;
                        S.doc[i] = da;
                        S.key[j] = kb;
                        S.doc[j] = db;
                    }
                }
            }
        lds_barrier();
        if (tid == 0) {
            S.cur = dlist::cut_count(live, k);
            if (live >= k) {
                const unsigned long long kb = S.key[k - 1u];
                atomicMax(&S.theta, kb);
                atomicMax(&bt.theta[q], kb);
            }
            ++st_cuts;
        }
        lds_barrier();
    };

    for (;;) {
        __syncthreads();  // previous item fully done with LDS
        if (tid == 0) {
            const uint32_t drawn = atomicAdd(&cold_args()->bt.work_ctr[0], 1u);
            S.item = drawn < n_items ? cold_args()->bt.item_order[drawn] : NONE32;
            S.cur = 0;
            S.fail = 0;
            S.theta = 0;
            S.m = 0;
        }
        __syncthreads();
        const uint32_t item = uni(S.item);
        if (item >= n_items) break;
        const Item it = cold_args()->bt.items[item];
        if (!(it.m & ITEM_SPARSE_BIG)) continue;  // the other kernels'
        q = uni(it.q);
        const uint32_t lo = uni(it.doc_lo), hi = uni(it.doc_hi);
        const unsigned long long *fw = query_filter(q);

        // ---- item setup (wave 0, lane t = term t): the indexed terms in query order, their tables, first blocks and s0
        uint32_t tw = 0, fb = 0;  // (wave 0's plan registers)
        bool act = false;
        if (wave == 0) {
            const KernArgsP ca = cold_args();
            uint32_t m = 0, term = NONE32;
            const uint32_t qb = uni(ca->bt.q_off[q]), qe = uni(ca->bt.q_off[q + 1]);
            for (uint32_t base = qb; base < qe; base += 64) {  // compaction of the indexed terms (search.rs:59-61)
                const uint32_t tt = base + lane < qe ? ca->bt.term_ids[base + lane] : NONE32;
                const bool ok = tt < ix.n_terms;
                const unsigned long long okm = __ballot(ok);
                const uint32_t pos = m + __builtin_amdgcn_mbcnt_hi((uint32_t)(okm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)okm, 0u));
                if (ok && pos < 64u) S.scratch[pos] = tt;
                m += (uint32_t)__popcll(okm);
            }
            __builtin_amdgcn_wave_barrier();
            m = min(uni(m), sbig::MAX_T);  // (the host marks queries of at most MAX_T indexed terms only)
            act = lane < m;
            if (act) {
                term = S.scratch[lane];
                tw = ix.term_win[term];
                fb = ca->ix.term_first_block[term];
                S.t_tw[lane] = tw;
                S.t_fb[lane] = fb;
                S.t_s0[lane] = ca->ix.term_s0[term];
            }
            const bool no_table = __ballot(act && tw == NONE32) != 0ull;  // (never: the host marks queries whose terms all have a table)
            if (lane == 0) {
                S.m = m;
                if (no_table) S.fail = 1u;
            }
        }
        __syncthreads();
        const uint32_t m = uni(S.m);

        // wave 0's cursor over the item: document `cur`, the tile width to try, the window whose runs the lanes hold ([wo0, wo1) in
        // the term's posting numbers), and the lane's slice start at cur
        uint32_t cur = lo, W = sbig::WIN, wl = NONE32, wo0 = 0, wo1 = 0, sa = 0;
        auto id_at = [&](uint32_t i) { return id16[128ull * fb + i]; };
        bool failed = uni(S.fail) != 0u;
        while (!failed) {
            // ---- plan (wave 0): the next tile with a posting in it
            if (wave == 0) {
                const unsigned long long pg = __hip_atomic_load(&bt.theta[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bool found = false, unfit = false;
                uint32_t tend = cur, sb = sa, ch = 0, incl = 0;
                while (cur < hi) {
                    const uint32_t w = cur >> 16;
                    if (w != wl) {  // a new window: the runs from the tables; an item's first window may start inside one
                        wo0 = act ? ix.win_off[tw + w] : 0u;
                        wo1 = act ? ix.win_off[tw + w + 1u] : 0u;
                        wl = w;
                        W = sbig::WIN;
                        sa = (cur & (sbig::WIN - 1u)) && act ? sbig::run_lower_bound(id_at, wo0, wo1, cur & (sbig::WIN - 1u)) : wo0;
                    }
                    const uint32_t part_hi = sbig::part_end(w, hi);
                    uint32_t posts = 0;
                    for (;;) {
                        tend = sbig::tile_end(cur, W, part_hi);
                        const bool to_end = (tend & (sbig::WIN - 1u)) == 0u || tend == ix.n_docs;  // (the window's last document: the run's end)
                        sb = to_end || !act ? wo1 : sbig::run_lower_bound(id_at, sa, wo1, tend & (sbig::WIN - 1u));
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
                        break;
                    }
                    cur = tend;  // an empty tile
                    sa = sb;
                    W = sbig::widen(W);
                }
                if (found) {
                    if (act) {
                        S.p_a[lane] = sa;
                        S.p_b[lane] = sb;
                        S.p_cb[lane] = incl - ch;
                    }
                    const uint32_t all_ch = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                    if (lane == 0) {
                        S.p_cb[m] = all_ch;
                        S.p_win = cur >> 16;
                        if (!sbig::whole_window(cur, tend, ix.n_docs)) ++st_slow;
                    }
                    cur = tend;
                    sa = sb;
                    W = sbig::widen(W);
                }
                if (lane == 0) {
                    S.p_done = found ? 0u : 1u;
                    if (unfit) S.fail = 1u;
                    atomicMax(&S.theta, pg);
                }
            }
            lds_barrier();  // the plan, and the bitmap clean
            if (uni(S.p_done)) {
                failed = uni(S.fail) != 0u;
                break;
            }
            const uint32_t nch = uni(S.p_cb[m]), win = uni(S.p_win);

            // ---- load: the thread's chunk.  Both loads issued here; the tf words are used behind the mark and the rank
            const bool own = tid < nch;
            uint32_t t = 0, mask = 0;
            uint32_t idw[4] = {0, 0, 0, 0}, tfw[4] = {0, 0, 0, 0};
            if (own) {
                t = sbig::chunk_term(S.p_cb, m, tid);
                const uint32_t a = S.p_a[t], b = S.p_b[t];
                const uint32_t start = sbig::chunk_start(a, S.p_cb[t], tid);
                mask = sbig::chunk_mask(start, a, b);
                const size_t v = 16ull * S.t_fb[t] + (start >> 3);  // (16 chunks a block; the planes are 256 bytes a block)
                const uint4 i4 = reinterpret_cast<const uint4 *>(ix.post_id16)[v];
                const uint4 f4 = reinterpret_cast<const uint4 *>(ix.post_tfn)[v];
                idw[0] = i4.x, idw[1] = i4.y, idw[2] = i4.z, idw[3] = i4.w;
                tfw[0] = f4.x, tfw[1] = f4.y, tfw[2] = f4.z, tfw[3] = f4.w;
            }
            // ---- mark
#pragma unroll
            for (uint32_t e = 0; e < sbig::CHUNK; ++e)
                if ((mask >> e) & 1u) {
                    const uint32_t id = sbig::chunk_id(idw, e);
                    atomicOr(&S.bm[id >> 5], 1u << (id & 31u));
                }
            lds_barrier();
            // ---- rank: bits before every word, documents of the tile
            uint32_t n_slots;
            {
                const uint4 bw = *reinterpret_cast<const uint4 *>(&S.bm[4u * tid]);
                const uint32_t c0 = sbig::popc(bw.x), c1 = sbig::popc(bw.y), c2 = sbig::popc(bw.z), c3 = sbig::popc(bw.w);
                const uint32_t own_c = c0 + c1 + c2 + c3;
                const uint32_t incl = wave_incl_scan_u32(own_c);
                if (lane == 63u) S.wsum[wave] = incl;
                lds_barrier();
                uint32_t before = 0, all = 0;
#pragma unroll
                for (uint32_t w2 = 0; w2 < dlist::WAVES; ++w2) {
                    const uint32_t x = S.wsum[w2];
                    before += w2 < wave ? x : 0u;
                    all += x;
                }
                n_slots = uni(all);
                const uint32_t ex = before + incl - own_c;  // (<= CAP: 16 bits hold it)
                *reinterpret_cast<uint2 *>(&S.pre[4u * tid]) = make_uint2(ex | (ex + c0) << 16, (ex + c0 + c1) | (ex + c0 + c1 + c2) << 16);
            }
            lds_barrier();
            uint32_t slot[sbig::CHUNK];
#pragma unroll
            for (uint32_t e = 0; e < sbig::CHUNK; ++e) {
                slot[e] = 0;
                if ((mask >> e) & 1u) {
                    const uint32_t id = sbig::chunk_id(idw, e);
                    slot[e] = sbig::slot_of(S.pre[id >> 5], S.bm[id >> 5], id & 31u);
                }
            }
            // ---- add: term after term in ascending query order, a barrier behind every term that has a posting in the tile
            for (uint32_t tt = 0; tt < m; ++tt) {
                if (uni(S.p_cb[tt + 1u]) == uni(S.p_cb[tt])) continue;
                if (own && t == tt) {
                    const double s0 = S.t_s0[tt];
#pragma unroll
                    for (uint32_t e = 0; e < sbig::CHUNK; ++e)
                        if ((mask >> e) & 1u) {
                            const uint32_t tfv = sbig::chunk_tf(tfw, e);
                            if (tfv == 0u) {
                                S.fail = 1u;  // wider than a byte: the item is scan_many_kernel's
                            } else {
                                const double tf = (double)tfv;
                                const double p = (tf * s0) / (tf + S.s1[sbig::chunk_fn(tfw, e)]);  // Cache::evaluate, bm25.rs:355-358
                                S.acc[slot[e]] = S.acc[slot[e]] + p;
                                S.sid[slot[e]] = (uint16_t)sbig::chunk_id(idw, e);
                            }
                        }
                }
                lds_barrier();
            }
            if (uni(S.fail)) {  // given up: leave the LDS clean
                for (uint32_t i = tid; i < n_slots; i += SBWG) S.acc[i] = 0.0;
                *reinterpret_cast<uint4 *>(&S.bm[4u * tid]) = make_uint4(0, 0, 0, 0);
                failed = true;
                break;
            }
            // ---- sweep: rounds of ROUND slots, a cut behind every round that left the cursor past k
            for (uint32_t r0 = 0; r0 < n_slots; r0 += sbig::ROUND) {
                const unsigned long long th = S.theta;
#pragma unroll
                for (uint32_t h = 0; h < sbig::ROUND / sbig::THREADS; ++h) {
                    const uint32_t s = r0 + h * sbig::THREADS + tid;
                    bool has = s < n_slots;
                    unsigned long long key = 0;
                    uint32_t d = 0;
                    if (has) {
                        key = (unsigned long long)__double_as_longlong(S.acc[s]);
                        S.acc[s] = 0.0;
                        d = (win << 16) + S.sid[s];
                        has = dlist::keeps(key, th) && (!fw || filter_keeps(fw, d));
                    }
                    const unsigned long long hm = __ballot(has);
                    if (hm) {
                        uint32_t base = 0;
                        if (lane == 0) base = atomicAdd(&S.cur, (uint32_t)__popcll(hm));
                        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                        const uint32_t at = rrk::offer_slot(base, __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0u)));
                        if (has && dlist::fits(at)) {  // (always fits: the arithmetic at the top of the file)
                            S.key[at] = key;
                            S.doc[at] = d;
                        }
                    }
                }
                lds_barrier();  // the round's appends are in; nobody appends before the next barrier: every wave reads the same cursor
                if (uni(S.cur) > k) list_cut();
                else lds_barrier();
            }
            *reinterpret_cast<uint4 *>(&S.bm[4u * tid]) = make_uint4(0, 0, 0, 0);
        }

        // ---- item end: the last cut sorts what is left; one list per item (lpi = 1), as scan_many_kernel writes its own
        __syncthreads();
        if (!failed) list_cut();
        {
            const uint32_t n = failed ? 0u : min(uni(S.cur), k);
            const KernArgsP ce = cold_args();
            for (uint32_t i = tid; i < n; i += SBWG) {
                ce->bt.res_score[(size_t)item * k + i] = __longlong_as_double((long long)S.key[i]);
                ce->bt.res_doc[(size_t)item * k + i] = S.doc[i];
            }
            if (tid == 0) {
                ce->bt.res_cnt[item] = n;
                ce->bt.item_failed[item] = failed ? SB_FAILED : 0u;
                if (failed) *ce->bt.fail_any = 1u;
                ++st_items;
                st_given += failed ? 1u : 0u;
            }
        }
    }
    if (tid == 0 && stats) {
        if (st_items) atomicAdd(&stats[0], st_items);
        if (st_given) atomicAdd(&stats[1], st_given);
        if (st_slow) atomicAdd(&stats[2], st_slow);
        if (st_cuts) atomicAdd(&stats[3], st_cuts);
    }
}

}  // namespace vbm25

#endif
