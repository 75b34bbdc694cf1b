// rerank.hip -- the rerank step on the device: a scorer handle over bound documents (vbm25_scorer) that keeps its stream, events,
// pinned staging and device buffers between calls, and the `<&>` operator's scores cut to each query's k best on the device.
// rerank_lane.h holds the per-entry functions of the selection; evaluate_shared.h the checks and the scoring kernel this file shares
// with evaluate.hip.
//
//   vbm25_scorer_evaluate   vbm25_evaluate_documents with the handle's buffers: the same checks (check_score_call), the same kernel
//                           (launch_eval_score), one staged upload, the scores back through the pinned block.
//   vbm25_scorer_topk       score and select fused; the nq x n_cand scores never reach HBM.  A unit is (query, part of at most
//                           rerank_part candidates); every query has at least one unit, so every row of the result has a writer.
//     rerank_part_kernel    one workgroup a unit, the workgroups stride the units.  A round: each of the four waves scores 64
//                           candidates (one whose document is dead in the handle's deletion bitmap is left out as a NO_DOC entry
//                           is: no score, no rank, its pos still counts) as eval_score_kernel does (the query's (id, idf) pairs 64 at a time through v_readlane,
//                           score_step per term in query order -- the same operations in the same order, so the same bits), then
//                           every lane offers (score key, pos) to the selection buffer in LDS if it beats the workgroup's threshold.
//                           A full buffer is sorted (bitonic, in place) and cut to k; the k-th entry is the new threshold.  A lane
//                           whose slot lies beyond the buffer keeps its entry and offers again after the cut.  At the end the
//                           buffer is sorted: a query of one unit gets its row written, a query of several its part list.
//     rerank_merge_kernel   one workgroup a query of several units: the part lists offered to the same buffer, 256 entries a round,
//                           then the row.  A kernel of its own behind the first on the stream: no flags, no fences, and the queries
//                           of one unit (the common rerank shape) never see it.
//   The selection is exact whatever the order of arrival: entries compare by (score, pos) as a whole and positions are distinct, so
//   an entry is only ever dropped against k better ones.  LDS: 12 bytes an entry + 16: 24 592 bytes at k = 1024 (2048 entries), the
//   sort is in place and the query's ids stay in registers -- six workgroups a CU by LDS.  No kernel here has scratch memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "resolve_lane.h"
#include "evaluate_lane.h"
#include "evaluate_shared.h"
#include "rerank_lane.h"
#include "rerank_shared.h"

struct vbm25_scorer {
    const vbm25_doc_terms *t = nullptr;
    int device = 0;
    std::mutex mu;  // one call at a time
    vbm25::HbmArray d_in, d_out, d_scr;  // the staged inputs, the results, the part lists
    vbm25::PinnedHost pin;               // the inputs' staging, then the results
    size_t pin_bytes = 0;
    vbm25::Event ev_start, ev_done;
    vbm25::Stream st;  // (declared last: destroyed first, after vbm25_scorer_free has waited for it)
};

namespace {

using namespace vbm25;
using namespace vbm25::rsv;
using namespace vbm25::evl;
using namespace vbm25::rrk;
using ull = unsigned long long;

constexpr uint32_t WG = ROUND, MAX_GRID = 2048;
constexpr uint32_t PART_DEFAULT = 1024, PART_MIN = 64, PART_MAX = 1u << 20;
static_assert(sizeof(vbm25_rank) == 16, "vbm25_rank is 16 bytes");

// rerank_part / rerank_buf of vbm25_tuning_set; read at the start of each scorer call
std::atomic<uint32_t> g_part{PART_DEFAULT}, g_buf{MIN_MULTIPLE};
// the calling thread's last scorer calls: the kernels by HIP events
thread_local double g_evaluate_ms = -1.0, g_topk_ms = -1.0;

// the selection buffer of a workgroup, the whole of its LDS: key[buf], thr_key, pos[buf], cnt, thr_pos
extern __shared__ ull rerank_lds[];
struct Sel {
    uint32_t buf, k;
    __device__ __forceinline__ ull *key() const { return rerank_lds; }
    __device__ __forceinline__ ull *thr_key() const { return rerank_lds + buf; }
    __device__ __forceinline__ uint32_t *pos() const { return reinterpret_cast<uint32_t *>(rerank_lds + buf + 1); }
    __device__ __forceinline__ uint32_t *cnt() const { return pos() + buf; }
    __device__ __forceinline__ uint32_t *thr_pos() const { return pos() + buf + 1; }
};
size_t sel_lds_bytes(uint32_t buf) { return 12ull * buf + 16; }

// A value every lane of the wave holds alike, into a scalar register.  Every loop and branch here that has a barrier inside is
// steered by such values only: a count read from LDS or HBM sits in a vector register, and a loop steered by it is a divergent loop
// to the compiler, which may then run the loop's barriers once per group of lanes (a wave with some lanes without a candidate ran the
// offer's barriers twice: its count came out one short).
__device__ __forceinline__ uint32_t uni(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
__device__ __forceinline__ ull uni(ull v) { return ull(uni(uint32_t(v >> 32))) << 32 | uni(uint32_t(v)); }

// the caller's barrier stands between the last use of the buffer and this
__device__ __forceinline__ void sel_reset(const Sel &s) {
    if (threadIdx.x == 0) {
        *s.cnt() = 0;
        *s.thr_key() = WORST_KEY;
        *s.thr_pos() = WORST_POS;
    }
    __syncthreads();
}

// entries 0 .. n (a power of two <= buf) best first.  In: the entries are visible to the workgroup.  Out: so is the order.
__device__ __forceinline__ void sel_sort(const Sel &s, uint32_t n) {
    for (uint32_t size = 2; size <= n; size <<= 1)
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < (n >> 1); t += WG) {
                uint32_t i, j;
                bitonic_pair(t, stride, i, j);
                uint64_t ak = s.key()[i], bk = s.key()[j];
                uint32_t ap = s.pos()[i], bp = s.pos()[j];
                exchange(ak, ap, bk, bp, bitonic_best_first(i, size));
                s.key()[i] = ak;
                s.pos()[i] = ap;
                s.key()[j] = bk;
                s.pos()[j] = bp;
            }
            __syncthreads();
        }
}

// Every thread of the workgroup calls this, with or without an entry.  An entry that loses to the threshold is dropped; the others
// take slots; when the buffer is full it is cut to its k best and the lanes left over offer again (the cut leaves buf - k >= k free
// slots, so every turn places an entry).
__device__ __forceinline__ void sel_offer(const Sel &s, bool have, ull key, uint32_t pos) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool beats = better(key, pos, *s.thr_key(), *s.thr_pos());  // (read by every lane: no branch in front of the loop)
    bool pending = have & beats;
    for (;;) {
        const ull offers = __ballot(pending);
        if (offers) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(s.cnt(), uint32_t(__popcll(offers)));
            base = uni(base);
            const uint32_t slot = offer_slot(base, uint32_t(__popcll(offers & ((1ull << lane) - 1ull))));
            if (pending && slot < s.buf) {
                s.key()[slot] = key;
                s.pos()[slot] = pos;
                pending = false;
            }
        }
        __syncthreads();
        const uint32_t n = uni(*s.cnt());
        __syncthreads();  // (everyone has read the count before the next offer or the cut changes it)
        if (n < s.buf) return;  // (every offer had a slot: nobody is pending)
        sel_sort(s, s.buf);     // full: slots 0 .. buf are all written
        if (threadIdx.x == 0) {
            *s.cnt() = s.k;
            *s.thr_key() = s.key()[s.k - 1];
            *s.thr_pos() = s.pos()[s.k - 1];
        }
        __syncthreads();
        pending = pending & better(key, pos, *s.thr_key(), *s.thr_pos());
    }
}

// the buffer's live entries sorted; returns how many of them the result takes
__device__ __forceinline__ uint32_t sel_finish(const Sel &s) {
    const uint32_t n = uni(*s.cnt());  // (below buf: sel_offer's last turn saw to it)
    const uint32_t span = sort_entries(n);
    for (uint32_t i = n + threadIdx.x; i < span; i += WG) {
        s.key()[i] = WORST_KEY;
        s.pos()[i] = WORST_POS;
    }
    __syncthreads();
    sel_sort(s, span);
    return n < s.k ? n : s.k;
}

// the last query with unit_start[q] <= u (every query has a unit: the starts ascend strictly)
__device__ __forceinline__ uint32_t unit_query(const uint32_t *unit_start, uint32_t nq, uint32_t u) {
    uint32_t ql = 0, qh = nq;
    while (qh - ql > 1) {
        const uint32_t mid = ql + ((qh - ql) >> 1);
        if (unit_start[mid] <= u) ql = mid; else qh = mid;
    }
    return uni(ql);
}

__device__ __forceinline__ void write_row(const TopkArgs &a, const TopkOut &o, const Sel &s, uint32_t q, ull cand0, uint32_t n) {
    vbm25_rank *row = o.ranks + size_t(q) * a.k;
    for (uint32_t i = threadIdx.x; i < a.k; i += WG) {
        vbm25_rank r;
        r.score = 0.0;
        r.pos = r.doc = 0;
        if (i < n) {
            r.score = __longlong_as_double((long long)key_score(s.key()[i]));
            r.pos = s.pos()[i];
            r.doc = a.s.cand_doc ? a.s.cand_doc[cand0 + r.pos] : r.pos;
        }
        row[i] = r;
    }
    if (threadIdx.x == 0) o.n_ranks[q] = n;
}

__global__ void __launch_bounds__(WG) rerank_part_kernel(TopkArgs a) {
    const Sel s{a.buf, a.k};
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
        __syncthreads();  // (the unit before is done with the buffer)
        const uint32_t *unit_start = a.out->unit_start, *q_off = a.out->q_off;
        const ull *q_cand = a.out->q_cand;
        const uint32_t q = unit_query(unit_start, a.s.nq, u);
        const uint32_t p = uni(u - unit_start[q]);
        const bool one_part = uni(unit_start[q + 1] - unit_start[q]) == 1u;
        const ull cand0 = uni(q_cand ? q_cand[q] : ull(q) * a.s.cross_docs);
        const uint32_t n_cand = uni(q_cand ? uint32_t(q_cand[q + 1] - cand0) : a.s.cross_docs);
        const uint32_t c_lo = p * a.part, c_hi = n_cand - c_lo < a.part ? n_cand : c_lo + a.part;
        const uint32_t qb = uni(q_off[q]), qn = uni(q_off[q + 1] - qb);
        sel_reset(s);
        for (uint32_t c0 = c_lo; c0 < c_hi; c0 += WG) {
            const uint32_t c = c0 + threadIdx.x;
            const uint32_t d = c >= c_hi ? NO_DOC : a.s.cand_doc ? a.s.cand_doc[cand0 + c] : c;
            bool mine = d != NO_DOC;  // (a list entry that names no document is not eligible; its pos still counts)
            // ... and neither is one whose document is dead.  The pointer is the same in every lane: a handle nobody deleted from
            // runs the line above and nothing more.
            if (a.dead && mine) mine = !((a.dead[d >> 6] >> (d & 63u)) & 1ull);
            // a lane without a candidate: the empty run 0 .. 0, which score_step never reads
            uint32_t cursor = 0, hi = 0;
            double s1 = 1.0;
            if (mine) {
                cursor = uint32_t(a.s.start[d]);
                hi = uint32_t(a.s.start[d + 1]);
                s1 = a.s.s1[a.s.fieldnorm[d]];
            }
            double result = 0.0;
            for (uint32_t t0 = 0; t0 < qn; t0 += 64) {
                const uint32_t chunk = qn - t0 < 64u ? qn - t0 : 64u;
                const uint32_t my_id = lane < chunk ? a.s.q_ids[qb + t0 + lane] : NOT_FOUND;
                const double my_idf = my_id < a.s.n_terms ? a.s.term_idf[my_id] : 0.0;
                for (uint32_t j = 0; j < chunk; ++j) {
                    const uint32_t id = uint32_t(__builtin_amdgcn_readlane(int(my_id), int(j)));
                    if (id >= a.s.n_terms) continue;
                    score_step(a.s.term, a.s.tf, cursor, hi, id, lane_double(my_idf, j), a.s.k1p1, s1, result);
                }
            }
            sel_offer(s, mine, score_key(ull(__double_as_longlong(result))), c);
        }
        const uint32_t n = sel_finish(s);
        const TopkOut o = *a.out;
        if (one_part) {
            write_row(a, o, s, q, cand0, n);
        } else {
            const uint32_t list = o.scr_start[q] + p;
            for (uint32_t i = threadIdx.x; i < n; i += WG) {
                o.scr_key[size_t(list) * a.k + i] = s.key()[i];
                o.scr_pos[size_t(list) * a.k + i] = s.pos()[i];
            }
            if (threadIdx.x == 0) o.scr_cnt[list] = n;
        }
    }
}

__global__ void __launch_bounds__(WG) rerank_merge_kernel(TopkArgs a) {
    const Sel s{a.buf, a.k};
    for (uint32_t m = blockIdx.x; m < a.n_multi; m += gridDim.x) {
        __syncthreads();
        const uint32_t q = uni(a.multi_q[m]);
        const TopkOut o = *a.out;
        const uint32_t n_parts = uni(o.unit_start[q + 1] - o.unit_start[q]), list0 = uni(o.scr_start[q]);
        const ull cand0 = uni(o.q_cand ? o.q_cand[q] : ull(q) * a.s.cross_docs);
        sel_reset(s);
        for (uint32_t p = 0; p < n_parts; ++p) {
            const uint32_t n = uni(o.scr_cnt[list0 + p]);
            for (uint32_t j0 = 0; j0 < n; j0 += WG) {
                const uint32_t j = j0 + threadIdx.x;
                const bool have = j < n;
                const size_t at = size_t(list0 + p) * a.k + (have ? j : 0u);
                sel_offer(s, have, o.scr_key[at], o.scr_pos[at]);
            }
        }
        write_row(a, o, s, q, cand0, sel_finish(s));
    }
}

// ---- the handle ----

// at least `need` bytes behind `a`, what it held lost; geometric, and the old block stays when the new one cannot be had
int grow(HbmArray &a, size_t need) {
    if (a.p && a.bytes >= need) return VBM25_OK;
    HbmArray next;
    HIP_TRY(next.alloc(std::max(need, 2 * a.bytes)));
    std::swap(a.p, next.p);
    std::swap(a.bytes, next.bytes);
    return VBM25_OK;
}
int grow_pinned(vbm25_scorer *sc, size_t need) {
    if (sc->pin.p && sc->pin_bytes >= need) return VBM25_OK;
    const size_t cap = std::max(need, 2 * sc->pin_bytes);
    PinnedHost next;
    HIP_TRY(next.alloc(cap));
    std::swap(sc->pin.p, next.p);  // (the old block goes with `next`, as in grow)
    sc->pin_bytes = cap;
    return VBM25_OK;
}

// one staged block: the 64-bit parts first, then the 32-bit arrays
struct Stage {
    size_t out = 0, cand = 0, off = 0, unit = 0, scr = 0, multi = 0, ids = 0, docs = 0, bytes = 0;
    Stage(uint32_t nq, bool lists, bool topk, uint32_t n_multi, uint32_t n_ids, uint64_t n_pairs) {
        size_t at = 0;
        auto take = [&](size_t n) { const size_t o = at; at += n; return o; };
        out = take(topk ? align_up(sizeof(TopkOut), 8) : 0);
        cand = take(lists ? 8ull * (nq + 1ull) : 0);
        off = take(4ull * (nq + 1ull));
        unit = take(4ull * (nq + 1ull));
        scr = take(topk ? 4ull * (nq + 1ull) : 0);
        multi = take(4ull * n_multi);
        ids = take(4ull * n_ids);
        docs = take(lists ? 4ull * n_pairs : 0);
        bytes = align_up(at, 16);
    }
};

void stage_common(const Stage &g, uint8_t *host, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                  const uint32_t *cand_doc, uint64_t n_pairs) {
    if (q_cand) {
        std::memcpy(host + g.cand, q_cand, 8ull * (nq + 1ull));
        if (n_pairs) std::memcpy(host + g.docs, cand_doc, 4ull * n_pairs);
    }
    std::memcpy(host + g.off, q_off, 4ull * (nq + 1ull));
    if (q_off[nq]) std::memcpy(host + g.ids, term_ids, 4ull * q_off[nq]);
}

void fill_call_arrays(const Stage &g, const uint8_t *dev, const vbm25_doc_terms *t, uint32_t nq, bool lists, ScoreArgs *a) {
    a->q_ids = reinterpret_cast<const uint32_t *>(dev + g.ids);
    a->q_off = reinterpret_cast<const uint32_t *>(dev + g.off);
    a->q_cand = lists ? reinterpret_cast<const ull *>(dev + g.cand) : nullptr;
    a->cand_doc = lists ? reinterpret_cast<const uint32_t *>(dev + g.docs) : nullptr;
    a->cross_docs = lists ? 0u : t->n_docs;
    a->nq = nq;
}

int scorer_evaluate(vbm25_scorer *sc, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                    const uint32_t *cand_doc, double *scores) {
    if (!sc) return set_error(VBM25_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> guard(sc->mu);
    const vbm25_doc_terms *t = sc->t;
    EvaluateTables ix;
    uint64_t n_pairs = 0;
    if (int rc = check_score_call(t, term_ids, q_off, nq, q_cand, cand_doc, scores, &ix, &n_pairs)) return rc;
    if (n_pairs == 0) return VBM25_OK;
    if (int rc = use_eval_device(sc->device)) return rc;
    g_evaluate_ms = -1.0;
    const Stage g(nq, q_cand != nullptr, false, 0, q_off[nq], n_pairs);
    const size_t out_bytes = 8ull * n_pairs;
    if (int rc = grow_pinned(sc, std::max(g.bytes, out_bytes))) return rc;
    if (int rc = grow(sc->d_in, g.bytes)) return rc;
    if (int rc = grow(sc->d_out, out_bytes)) return rc;
    uint8_t *host = sc->pin.as<uint8_t>();
    stage_common(g, host, term_ids, q_off, nq, q_cand, cand_doc, n_pairs);
    uint32_t *item_start = reinterpret_cast<uint32_t *>(host + g.unit);  // the items: a scan of the candidate counts, 64 candidates an item
    item_start[0] = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t n = q_cand ? q_cand[q + 1] - q_cand[q] : t->n_docs;
        item_start[q + 1] = item_start[q] + uint32_t((n + 63) / 64);
    }
    ScoreArgs a{};
    fill_score_tables(t, ix, &a);
    fill_call_arrays(g, sc->d_in.as<uint8_t>(), t, nq, q_cand != nullptr, &a);
    a.item_start = reinterpret_cast<const uint32_t *>(sc->d_in.as<uint8_t>() + g.unit);
    a.n_items = item_start[nq];
    a.scores = sc->d_out.as<double>();
    Quiesce quiesce(sc->st.s);  // (a failed step below leaves nothing in flight behind the call)
    HIP_TRY(hipMemcpyAsync(sc->d_in.p, host, g.bytes, hipMemcpyHostToDevice, sc->st.s));
    HIP_TRY(hipEventRecord(sc->ev_start.e, sc->st.s));
    HIP_TRY(launch_eval_score(a, sc->st.s));
    HIP_TRY(hipEventRecord(sc->ev_done.e, sc->st.s));
    // (the upload is behind the kernel on the stream: the staging is free to take the results)
    HIP_TRY(hipMemcpyAsync(host, sc->d_out.p, out_bytes, hipMemcpyDeviceToHost, sc->st.s));
    HIP_TRY(hipStreamSynchronize(sc->st.s));
    std::memcpy(scores, host, out_bytes);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, sc->ev_start.e, sc->ev_done.e));
    g_evaluate_ms = ms;
    return VBM25_OK;
}

int scorer_topk(vbm25_scorer *sc, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                const uint32_t *cand_doc, uint32_t k, vbm25_rank *ranks, uint32_t *n_ranks) {
    if (!sc) return set_error(VBM25_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> guard(sc->mu);
    const vbm25_doc_terms *t = sc->t;
    EvaluateTables ix;
    uint64_t n_pairs = 0;
    if (int rc = check_score_call(t, term_ids, q_off, nq, q_cand, cand_doc, ranks && n_ranks ? ranks : nullptr, &ix, &n_pairs)) return rc;
    if (k == 0) return set_error(VBM25_ERR_INVALID, "k is 0");
    if (k > MAX_K) return set_error(VBM25_ERR_UNSUPPORTED, "k is %u: a scorer returns at most %u candidates a query", k, MAX_K);
    if (nq == 0) return VBM25_OK;
    const size_t rank_bytes = size_t(nq) * k * sizeof(vbm25_rank), out_bytes = rank_bytes + 4ull * nq;
    if (n_pairs == 0) {  // no query has a candidate: every row is its zero tail
        std::memset(ranks, 0, rank_bytes);
        std::memset(n_ranks, 0, 4ull * nq);
        return VBM25_OK;
    }
    if (int rc = use_eval_device(sc->device)) return rc;
    g_topk_ms = -1.0;
    const uint32_t part = g_part.load(), buf = buffer_entries(k, g_buf.load());
    const UnitPlan plan = count_units(q_cand, t->n_docs, part, nq);
    const uint32_t n_units = plan.n_units, n_multi = plan.n_multi, n_lists = plan.n_lists;
    const Stage g(nq, q_cand != nullptr, true, n_multi, q_off[nq], n_pairs);
    const size_t list_entries = size_t(n_lists) * k, scr_bytes = part_list_bytes(n_lists, k);
    if (int rc = grow_pinned(sc, std::max(g.bytes, out_bytes))) return rc;
    if (int rc = grow(sc->d_in, g.bytes)) return rc;
    if (int rc = grow(sc->d_out, out_bytes)) return rc;
    if (int rc = grow(sc->d_scr, scr_bytes)) return rc;
    uint8_t *host = sc->pin.as<uint8_t>();
    stage_common(g, host, term_ids, q_off, nq, q_cand, cand_doc, n_pairs);
    fill_units(q_cand, t->n_docs, part, nq, reinterpret_cast<uint32_t *>(host + g.unit), reinterpret_cast<uint32_t *>(host + g.scr),
               reinterpret_cast<uint32_t *>(host + g.multi));
    TopkArgs a{};
    fill_score_tables(t, ix, &a.s);
    const uint8_t *dev = sc->d_in.as<uint8_t>();
    fill_call_arrays(g, dev, t, nq, q_cand != nullptr, &a.s);
    a.multi_q = reinterpret_cast<const uint32_t *>(dev + g.multi);
    a.n_units = n_units;
    a.n_multi = n_multi;
    a.k = k;
    a.buf = buf;
    a.part = part;
    a.dead = t->d_dead.as<ull>();
    a.out = reinterpret_cast<const TopkOut *>(dev + g.out);
    TopkOut o;
    o.unit_start = reinterpret_cast<const uint32_t *>(dev + g.unit);
    o.q_off = a.s.q_off;
    o.q_cand = a.s.q_cand;
    o.scr_start = reinterpret_cast<const uint32_t *>(dev + g.scr);
    o.scr_key = sc->d_scr.as<ull>();
    o.scr_pos = reinterpret_cast<uint32_t *>(sc->d_scr.as<uint8_t>() + 8ull * list_entries);
    o.scr_cnt = o.scr_pos + list_entries;
    o.ranks = sc->d_out.as<vbm25_rank>();
    o.n_ranks = reinterpret_cast<uint32_t *>(sc->d_out.as<uint8_t>() + rank_bytes);
    std::memcpy(host + g.out, &o, sizeof o);
    Quiesce quiesce(sc->st.s);
    HIP_TRY(hipMemcpyAsync(sc->d_in.p, host, g.bytes, hipMemcpyHostToDevice, sc->st.s));
    HIP_TRY(hipEventRecord(sc->ev_start.e, sc->st.s));
    HIP_TRY(launch_topk(a, sc->st.s));
    HIP_TRY(hipEventRecord(sc->ev_done.e, sc->st.s));
    HIP_TRY(hipMemcpyAsync(host, sc->d_out.p, out_bytes, hipMemcpyDeviceToHost, sc->st.s));
    HIP_TRY(hipStreamSynchronize(sc->st.s));
    std::memcpy(ranks, host, rank_bytes);
    std::memcpy(n_ranks, host + rank_bytes, 4ull * nq);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, sc->ev_start.e, sc->ev_done.e));
    g_topk_ms = ms;
    return VBM25_OK;
}

int scorer_create(const vbm25_doc_terms *t, vbm25_scorer **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!t) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = use_eval_device(t->device)) return rc;
    auto sc = std::make_unique<vbm25_scorer>();
    sc->t = t;
    sc->device = t->device;
    HIP_TRY(sc->st.create());
    HIP_TRY(sc->ev_start.create());
    HIP_TRY(sc->ev_done.create());
    *out = sc.release();
    return VBM25_OK;
}

}  // namespace

namespace vbm25 {
namespace rrk {
uint32_t rerank_part_now() { return g_part.load(); }
uint32_t rerank_buf_now() { return g_buf.load(); }
hipError_t launch_topk(const TopkArgs &a, hipStream_t stream) {
    const uint32_t cap = std::max(1u, eval_grid_cap());
    rerank_part_kernel<<<std::min(std::min(a.n_units, MAX_GRID), cap), WG, sel_lds_bytes(a.buf), stream>>>(a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (a.n_multi) {
        rerank_merge_kernel<<<std::min(std::min(a.n_multi, MAX_GRID), cap), WG, sel_lds_bytes(a.buf), stream>>>(a);
        return hipGetLastError();
    }
    return hipSuccess;
}
}  // namespace rrk
int rerank_tuning_set(const char *name, long long value) {
    if (std::string(name) == "rerank_part")
        g_part.store(uint32_t(std::min<long long>(std::max<long long>(value, PART_MIN), PART_MAX)) / 64u * 64u);
    else
        g_buf.store(uint32_t(std::min<long long>(std::max<long long>(value, MIN_MULTIPLE), MAX_MULTIPLE)));
    return VBM25_OK;
}
void rerank_tuning_reset() {
    g_part.store(PART_DEFAULT);
    g_buf.store(MIN_MULTIPLE);
}
}  // namespace vbm25

extern "C" {

int vbm25_scorer_create(const vbm25_doc_terms *t, vbm25_scorer **out) {
    return guarded([&] { return scorer_create(t, out); });
}

void vbm25_scorer_free(vbm25_scorer *sc) {
    if (!sc) return;
    (void)hipSetDevice(sc->device);
    if (sc->st.s) (void)hipStreamSynchronize(sc->st.s);
    delete sc;
}

uint64_t vbm25_scorer_device_bytes(const vbm25_scorer *sc) {
    uint64_t n = 0;
    if (sc)
        for (const HbmArray *a : {&sc->d_in, &sc->d_out, &sc->d_scr}) n += a->footprint();
    return n;
}

int vbm25_scorer_evaluate(vbm25_scorer *sc, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                          const uint32_t *cand_doc, double *scores) {
    return guarded([&] { return scorer_evaluate(sc, term_ids, q_off, nq, q_cand, cand_doc, scores); });
}

int vbm25_scorer_topk(vbm25_scorer *sc, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                      const uint32_t *cand_doc, uint32_t k, vbm25_rank *ranks, uint32_t *n_ranks) {
    return guarded([&] { return scorer_topk(sc, term_ids, q_off, nq, q_cand, cand_doc, k, ranks, n_ranks); });
}

// tools/rerank_cost.py: the device time of the calling thread's last vbm25_scorer_evaluate's and last vbm25_scorer_topk's kernels, by
// HIP events.  Not in the header.
int vbm25_debug_rerank_kernel_ms(double *evaluate_ms, double *topk_ms) {
    if (!evaluate_ms || !topk_ms) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *evaluate_ms = g_evaluate_ms;
    *topk_ms = g_topk_ms;
    return VBM25_OK;
}

}  // extern "C"
