// bigk.hip -- the sparse half of the k > 1024 route (run_exhaustive, search.hip): batched over queries, its cost grows with the
// postings the queries touch, not with the index.  A query whose document frequencies sum to at most bigk_cand_max takes it; the
// others of the batch keep the per-query path of search.hip (an accumulator per document, one launch per term, a radix sort of every
// document).  Records are byte for byte that path's.  Per chunk of queries (their candidate segments fit the batch's scratch) four
// launches, whatever the queries:
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
// Host: bigk_create sizes the scratch when the batch is made, bigk_plan cuts queries into chunks and items at set_queries (no device
// planning pass), bigk_run enqueues.  Nothing is allocated in a run.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "vbm25_internal.h"
#include "host_objects.h"
#include "decode.h"
#include "rerank_lane.h"
#include "bigk_lane.h"

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

// first j in [lo, hi) with v[j] >= x, hi when none; v ascending.  The whole wave calls it with the same arguments: 64 samples a step.
__device__ __forceinline__ uint32_t wave_lower_bound(const uint32_t *__restrict__ v, uint32_t lo, uint32_t hi, uint32_t x, uint32_t lane) {
    while (lo < hi) {
        const uint32_t n = hi - lo, step = (n + 63u) / 64u;
        const uint32_t idx = min(lo + (lane + 1u) * step - 1u, hi - 1u);
        const ull m = __ballot(v[idx] >= x);
        if (!m) return hi;  // (the last lane sampled hi - 1)
        const uint32_t f = (uint32_t)__ffsll((long long)m) - 1u;
        if (step == 1u) return lo + f;
        const uint32_t top = min(lo + (f + 1u) * step - 1u, hi - 1u);  // v[top] >= x, v[lo + f step - 1] < x
        lo += f * step;
        hi = top + 1u;
        if (hi - lo == 1u) return lo;
    }
    return hi;
}

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
    int rc = 0;
    if ((rc = g.cand_key.alloc(8 * g.chunk_cand)) || (rc = g.cand_doc.alloc(4 * g.chunk_cand)) ||
        (rc = g.surv_key.alloc(8ull * g.chunk_q * g.surv_stride)) || (rc = g.surv_doc.alloc(4ull * g.chunk_q * g.surv_stride)) ||
        (rc = g.cursor.alloc(4ull * bt->max_queries)) || (rc = g.surv_cnt.alloc(4ull * bt->max_queries)) ||
        (rc = g.sel.alloc(4ull * bt->max_queries)) || (rc = g.qd.alloc(sizeof(BigkQuery) * size_t(bt->max_queries))) ||
        (rc = g.terms.alloc(4ull * std::max(bt->max_terms, 1u))) || (rc = g.items.alloc(sizeof(BigkItem) * g.max_items)))
        return rc;
    g.sparse.assign(bt->max_queries, 0);
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
    g.n_sparse = 0;
    g.chunks.clear();
    if (!g.on) return VBM25_OK;
    const vbm25_index *ix = bt->index;
    const uint32_t nq = uint32_t(bt->h_off.size()) - 1u;
    g.h_qd.clear();
    g.h_terms.clear();
    g.h_items.clear();
    std::fill(g.sparse.begin(), g.sparse.end(), uint8_t(0));
    uint32_t n_scanned = 0;  // sparse queries with a posting: the others make no item
    for (uint32_t q = 0; q < nq; ++q) {
        if (bt->h_postings[q] > g.cand_max) continue;
        g.sparse[q] = 1;
        BigkQuery d{};
        d.q = q;
        d.term_lo = uint32_t(g.h_terms.size());
        for (uint32_t p = bt->h_off[q]; p < bt->h_off[q + 1]; ++p)
            if (bt->h_terms[p] < ix->n_terms && ix->term_df_host[bt->h_terms[p]]) g.h_terms.push_back(bt->h_terms[p]);  // search.rs:59-61
        d.term_hi = uint32_t(g.h_terms.size());
        d.cand_cap = uint32_t(bt->h_postings[q]);
        n_scanned += d.cand_cap != 0;
        g.h_qd.push_back(d);
    }
    g.n_sparse = uint32_t(g.h_qd.size());
    if (!g.n_sparse) return VBM25_OK;
    const uint32_t n_win = (ix->n_docs + bgk::WINDOW - 1u) / bgk::WINDOW;
    const uint32_t wpi = bgk::item_windows(n_win, n_scanned, bt->tune.bigk_item_win, ITEM_TARGET, g.max_items);
    g.wpi = wpi;
    // chunks: queries in order while their candidate segments fit the scratch and their survivors the survivor buffers
    for (uint32_t s = 0; s < g.n_sparse;) {
        BigkChunk c{};
        c.s0 = s;
        c.item0 = uint32_t(g.h_items.size());
        uint64_t used = 0;
        while (s < g.n_sparse && s - c.s0 < g.chunk_q && used + g.h_qd[s].cand_cap <= g.chunk_cand) {
            g.h_qd[s].cand_base = uint32_t(used);
            used += g.h_qd[s].cand_cap;
            if (g.h_qd[s].cand_cap)
                for (uint32_t w = 0; w < n_win; w += wpi) g.h_items.push_back(BigkItem{s, w, std::min(w + wpi, n_win)});
            ++s;
        }
        if (s == c.s0) return set_error(VBM25_ERR_INVALID, "internal error: a sparse query exceeds the candidate scratch");
        c.s1 = s;
        c.item1 = uint32_t(g.h_items.size());
        g.chunks.push_back(c);
    }
    if (g.h_items.size() > g.max_items) return set_error(VBM25_ERR_INVALID, "internal error: %zu work items exceed the buffer", g.h_items.size());
    HIP_TRY(hipMemcpy(g.qd.p, g.h_qd.data(), sizeof(BigkQuery) * g.h_qd.size(), hipMemcpyHostToDevice));
    if (!g.h_terms.empty()) HIP_TRY(hipMemcpy(g.terms.p, g.h_terms.data(), 4ull * g.h_terms.size(), hipMemcpyHostToDevice));
    if (!g.h_items.empty()) HIP_TRY(hipMemcpy(g.items.p, g.h_items.data(), sizeof(BigkItem) * g.h_items.size(), hipMemcpyHostToDevice));
    return VBM25_OK;
}

// the sparse queries of the current set, on st: one clear, then four launches a chunk
int bigk_run(vbm25_batch *bt, hipStream_t st) {
    BigkState &g = bt->bg;
    if (!g.n_sparse) return VBM25_OK;
    const DevIndex &dix = bt->index->dev;
    Args a{};
    a.qd = g.qd.as<BigkQuery>();
    a.items = g.items.as<BigkItem>();
    a.terms = g.terms.as<uint32_t>();
    a.cursor = g.cursor.as<uint32_t>();
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
    bigk_clear_kernel<<<(g.n_sparse + 255) / 256, 256, 0, st>>>(a.cursor, g.n_sparse);
    const uint32_t k_tiles = g.surv_stride / bgk::TILE;
    for (const BigkChunk &c : g.chunks) {
        const uint32_t cq = c.s1 - c.s0;
        if (c.item1 > c.item0) bigk_scan_kernel<<<c.item1 - c.item0, bgk::SCAN_THREADS, 0, st>>>(dix, a, c.item0);
        bigk_select_kernel<<<cq, SELECT_THREADS, 0, st>>>(a, c.s0);
        bigk_sort_kernel<<<dim3(k_tiles, cq), SORT_THREADS, 0, st>>>(a, c.s0);
        bigk_rank_emit_kernel<<<dim3((bt->k + EMIT_THREADS - 1) / EMIT_THREADS, cq), EMIT_THREADS, 0, st>>>(dix, a, c.s0);
    }
    HIP_TRY(hipGetLastError());
    return VBM25_OK;
}

}  // namespace vbm25
