// reranker.hip -- the rerank step as a ring (vbm25_reranker): lexeme queries (or term ids) and candidate lists (document indices,
// ctids, or none for the cross product) in, each query's k best (score, pos, doc) rows out, first in first out.  `depth` slots keep
// their stream, events, pinned blocks, resolve scratch and result arrays between batches; between submit and collect the host
// touches nothing.  The ring assembles what the library has: the intern / lookup / pack kernels of resolve.hip (resolve_shared.h),
// the fused score-and-select kernels of rerank.hip (rerank_shared.h), the two-stage sorted-key search of tid_lane.h.
//
//   per batch, all on the slot's own stream:
//     upload               the slot's pinned block (every array of the call, the units and the TopkOut) in ONE copy
//     intern -> pack       the lexemes to ascending term ids, the pack's last kernel writing q_off / term_ids into the slot's HBM
//                          arrays (the wave path for batches of queries <= 64 lexemes, the radix path otherwise); submit_ids has
//                          the ids in the staged block instead
//     cand_lookup_kernel   candidates given as ctids: one lane a candidate, tid_find in the payload directory (its directory staged
//                          in LDS once per workgroup, its sorted keys in HBM) -> the document index, or NO_DOC for a ctid no
//                          document carries.  On a handle with a deletion bitmap (vbm25_doc_terms_delete*) the position is walked
//                          forward over the ctid's entries to the lowest document that is not dead (tid_first_live), NO_DOC when
//                          all are.  Grid-stride under the eval_grid cap.
//     rerank_part_kernel (+ rerank_merge_kernel)   with the resolved ids; a NO_DOC entry is not eligible, its pos still counts
//     download             the rows and counts into the slot's pinned block, then the done event
//   The payload directory (built once at create, from the payloads of a vbm25_documents or, for vbm25_reranker_create_from_index,
//   from the doc_payload plane of the index the handle was bound from): (tid_key(payload[d]), d) sorted by the
//   48 key bits -- the sort is stable, equal keys keep ascending d, so a ctid of several documents resolves to the lowest -- and
//   tid_lane.h's directory of evenly spaced keys over them, under the tid_dir switch.
//   vbm25_reranker_sync (after vbm25_doc_terms_append*): the ctids of the documents the directory lacks, sorted (live_sort_kernel in
//   LDS up to live_sort_max rows, else payload_key_kernel + the radix sort), merged by rank with the old entries into spare arrays
//   (live_merge_kernel; live_shared.h) and the directory sampled again, on slot 0's stream; the spares are swapped in once every
//   slot has finished, so a batch submitted before the sync reads the old directory to its end.  cand_lookup_kernel's n_keys is the
//   count the directory covers (dir_n), not the handle's n_docs.
//   No stream waits for another: a slot is reused only after its collect, and the doc_terms, the vocabulary and the directory are
//   only read between syncs.  No kernel here has scratch memory.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "ring.h"
#include "resolve_shared.h"
#include "evaluate_shared.h"
#include "rerank_shared.h"
#include "tid_lane.h"
#include "live_shared.h"

namespace {

using namespace vbm25;
using namespace vbm25::rsv;
using namespace vbm25::evl;
using namespace vbm25::rrk;
using namespace vbm25::tid;
using vbm25::lexin::Seed;
using ull = unsigned long long;

constexpr uint32_t WG = 256, MAX_GRID = 2048;
enum CandKind : uint32_t { CAND_CROSS = 0, CAND_DOC = 1, CAND_TID = 2 };
enum PackPath : uint32_t { PATH_NONE = 0, PATH_WAVE = 1, PATH_RADIX = 2 };

// payload: the ctids of documents first .. first + n; keys / docs: where their entries go
__global__ void __launch_bounds__(WG) payload_key_kernel(const uint16_t *payload, uint32_t n, uint32_t first, ull *keys, uint32_t *docs) {
    for (uint32_t d = blockIdx.x * WG + threadIdx.x; d < n; d += gridDim.x * WG) {
        const uint16_t *p = payload + 3ull * d;
        const uint16_t p3[3] = {p[0], p[1], p[2]};
        keys[d] = tid_key(p3);
        docs[d] = first + d;
    }
}

__global__ void __launch_bounds__(WG) payload_dir_kernel(const ull *keys, uint32_t n_dir, uint32_t stride, ull *dir) {
    const uint32_t j = blockIdx.x * WG + threadIdx.x;
    if (j < n_dir) dir[j] = keys[dir_source(j, stride)];
}

struct LookupArgs {
    const uint16_t *tids;  // n x 3
    ull n;
    const ull *dir, *keys;  // the payload directory and the sorted keys under it
    const uint32_t *docs;   // the sorted keys' documents
    ull n_keys;
    uint32_t n_dir, stride;
    uint32_t *cand_doc;  // n
    const ull *dead;     // the handle's deletion bitmap as the submit found it (NULL: nobody deleted from the handle)
};
static_assert(NO_LIVE_DOC == NO_DOC, "a ctid whose documents are all dead is an entry that names no document");

__global__ void __launch_bounds__(WG) cand_lookup_kernel(LookupArgs a) {
    extern __shared__ ull s_dir[];
    for (uint32_t i = threadIdx.x; i < a.n_dir; i += WG) s_dir[i] = a.dir[i];
    __syncthreads();
    for (ull i = ull(blockIdx.x) * WG + threadIdx.x; i < a.n; i += ull(gridDim.x) * WG) {
        const uint16_t *p = a.tids + 3 * i;
        const uint16_t p3[3] = {p[0], p[1], p[2]};
        const uint64_t key = tid_key(p3);
        const uint64_t at = tid_find(key, (const uint64_t *)s_dir, a.n_dir, (const uint64_t *)a.keys, a.n_keys, a.stride);
        uint32_t doc = at == NOT_THERE ? NO_DOC : a.docs[at];
        // with a bitmap (the same pointer in every lane): the lowest LIVE document of the ctid -- a reused ctid names the new row
        if (a.dead && at != NOT_THERE) doc = tid_first_live(at, key, (const uint64_t *)a.keys, a.docs, a.n_keys, (const uint64_t *)a.dead);
        a.cand_doc[i] = doc;
    }
}

struct RerankSlot {
    Stream stream;
    Event start, done;
    PinnedHost pin_in, pin_out;                           // the staged block of one batch; its rows and counts
    HbmArray in;                                          // the staged block
    HbmArray ids, tmp, counts, q_off, sort_a, sort_b, cub;  // the resolve scratch (resolve_shared.h: PackScratch)
    HbmArray res_q_off, res_ids;                          // the resolved queries
    HbmArray cand_doc;                                    // the documents of a ctid list (a reranker with payloads only)
    HbmArray out, scr;                                    // the rows and counts; the part lists
    uint32_t nq = 0, k = 0;
    bool enqueued = false;  // false: a batch without a candidate, which collects as zero rows
};

// one staged block, every part rounded up to 16 bytes
struct Layout {
    size_t out = 0, cand = 0, lex_off = 0, unit = 0, scr = 0, multi = 0, q32 = 0, docs = 0, ids = 0, pool = 0, bytes = 0;
    // n_lex: the lexemes of a lexeme batch (lex_off has n_lex + 1 entries), ~0 for an id batch; n_ids: the ids of an id batch
    Layout(uint64_t nq, bool lists, uint64_t n_multi, uint64_t n_lex, uint64_t n_ids, uint64_t n_pairs, uint32_t cand_kind, uint64_t n_bytes) {
        size_t at = 0;
        auto take = [&](size_t n) { const size_t o = at; at += align_up(n, 16); return o; };
        out = take(sizeof(TopkOut));
        cand = take(lists ? 8 * (nq + 1) : 0);
        lex_off = take(n_lex != ~0ull ? 8 * (n_lex + 1) : 0);
        unit = take(4 * (nq + 1));
        scr = take(4 * (nq + 1));
        multi = take(4 * n_multi);
        q32 = take(4 * (nq + 1));  // q_lex, or q_off
        docs = take(cand_kind == CAND_TID ? 6 * n_pairs : cand_kind == CAND_DOC ? 4 * n_pairs : 0);
        ids = take(4 * n_ids);
        pool = take(align_up(n_bytes, 4));
        bytes = at;
    }
};

}  // namespace

// vbm25_reranker_free waits for every slot's stream before it deletes: the order of the members below does not matter to their destructors.
struct vbm25_reranker {
    const vbm25_doc_terms *t = nullptr;
    int device = 0;
    uint32_t max_queries = 0, max_lexemes = 0, max_k = 0, n_terms = 0;
    uint64_t max_bytes = 0, max_candidates = 0, max_lists = 0;
    const Key *vocab = nullptr;  // the resolver's, in HBM
    bool has_seed = false;
    Seed seed{};
    bool has_payloads = false;
    uint32_t n_dir = 0, stride = 1;
    uint32_t dir_n = 0;  // the documents the directory covers: the handle's n_docs at create or at the last vbm25_reranker_sync
    HbmArray dir_keys, dir_docs, dir;  // the payload directory: dir_n sorted keys, their documents, n_dir evenly spaced keys
    // vbm25_reranker_sync: the spare arrays a merge writes and the sync swaps in (dir_keys / dir_docs and their spares hold room to
    // spare, in entries: dir_cap; the spare directory has MAX_DIR_LOG2's 4096 entries), and the delta's scratch -- its sorted keys
    // and documents, the radix sort's input and temporary storage -- for delta_cap rows.  All empty until the first sync that grows.
    HbmArray dir_keys2, dir_docs2, dir2, delta_keys, delta_docs, delta_keys_in, delta_docs_in, delta_cub;
    uint64_t dir_cap = 0, delta_cap = 0;
    size_t delta_cub_bytes = 0;
    Event sync_start, sync_done;  // around a sync's kernels (made by the first sync)
    double directory_ms = -1.0, sync_ms = -1.0;
    size_t in_capacity = 0, cub_bytes = 0;
    std::vector<uint32_t> zero_off;  // max_queries + 1 zeros: the q_off of a lexeme batch before it is resolved
    ResourceTally tally;  // every allocation and creation of the handle goes through it
    RerankSlot slots[16];
    RingCursor ring;
    int last_collected = -1;
    uint32_t last_path = PATH_NONE;
};

namespace {

// the payload directory over `n` payloads in HBM (a vbm25_documents' or an index's) and, behind them, the `n_tail` payloads of the
// documents the handle was appended (n_tail == 0: a handle that has not grown), on slot 0's stream; synchronous
int build_directory(vbm25_reranker *r, const uint16_t *payload, uint32_t n_base, const uint16_t *tail, uint32_t n_tail) {
    const uint32_t n = n_base + n_tail;
    r->dir_n = n;
    r->dir_cap = n;
    const DirShape shape = dir_shape(n, tid_dir_now());
    r->n_dir = shape.n_dir;
    r->stride = shape.stride;
    hipStream_t st = r->slots[0].stream.s;
    ResourceTally &ta = r->tally;
    HbmArray keys_in, docs_in, cub;
    Event ev_start, ev_done;
    HIP_TRY(ta.event_create(ev_start));
    HIP_TRY(ta.event_create(ev_done));
    Quiesce quiesce(st);  // (behind the temporaries: waited for before they are freed)
    HIP_TRY(ta.device_alloc(r->dir_keys, 8ull * n));
    HIP_TRY(ta.device_alloc(r->dir_docs, 4ull * n));
    HIP_TRY(ta.device_alloc(r->dir, 8ull * r->n_dir));
    HIP_TRY(hipEventRecord(ev_start.e, st));
    if (n) {
        HIP_TRY(ta.device_alloc(keys_in, 8ull * n, false));
        HIP_TRY(ta.device_alloc(docs_in, 4ull * n, false));
        size_t cub_bytes = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, (const ull *)nullptr, (ull *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                  int(n), 0, 48, st));
        HIP_TRY(ta.device_alloc(cub, cub_bytes, false));
        if (n_base) payload_key_kernel<<<grid_for(n_base, WG, MAX_GRID), WG, 0, st>>>(payload, n_base, 0u, keys_in.as<ull>(), docs_in.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        if (n_tail)
            payload_key_kernel<<<grid_for(n_tail, WG, MAX_GRID), WG, 0, st>>>(tail, n_tail, n_base, keys_in.as<ull>() + n_base, docs_in.as<uint32_t>() + n_base);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub.p, cub_bytes, keys_in.as<ull>(), r->dir_keys.as<ull>(), docs_in.as<uint32_t>(),
                                                  r->dir_docs.as<uint32_t>(), int(n), 0, 48, st));
        payload_dir_kernel<<<(r->n_dir + WG - 1) / WG, WG, 0, st>>>(r->dir_keys.as<ull>(), r->n_dir, r->stride, r->dir.as<ull>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev_done.e, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(elapsed_ms(ev_start, ev_done, &r->directory_ms));
    return VBM25_OK;
}

// from_index: the ctids are the index's own (vbm25_reranker_create_from_index; `payloads` is NULL then)
int reranker_create(const vbm25_doc_terms *t, const vbm25_resolver *rs, const vbm25_documents *payloads, bool from_index, uint32_t depth,
                    uint32_t max_queries, uint32_t max_lexemes, uint64_t max_bytes, uint64_t max_candidates, uint32_t max_k, vbm25_reranker **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!t || !rs) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (from_index && !t->from_index)
        return set_error(VBM25_ERR_INVALID, "the bound documents were not made by vbm25_index_bind: their ctids are not the index's");
    if (depth < 1 || depth > 16) return set_error(VBM25_ERR_INVALID, "depth %u is outside 1 .. 16", depth);
    if (!max_queries || !max_lexemes || !max_candidates || !max_k)
        return set_error(VBM25_ERR_INVALID, "max_queries, max_lexemes, max_candidates or max_k is 0");
    if (max_queries >= (1u << 31) || max_lexemes >= (1u << 31)) return set_error(VBM25_ERR_INVALID, "max_queries or max_lexemes is 2^31 or more");
    if (max_k > MAX_K) return set_error(VBM25_ERR_UNSUPPORTED, "k is %u: a scorer returns at most %u candidates a query", max_k, MAX_K);
    ResolverVocabulary v;
    if (int rc = resolver_vocabulary(rs, &v)) return rc;
    ResolverSeed sd;
    if (int rc = resolver_seed(rs, &sd)) return rc;
    if (v.device != t->device)
        return set_error(VBM25_ERR_INVALID, "the bound documents are on device %d, the resolver's index is on device %d", t->device, v.device);
    if (v.index != t->index) return set_error(VBM25_ERR_INVALID, "the documents are bound to another index than the resolver's");
    if (payloads) {
        if (!payloads->has_payload) return set_error(VBM25_ERR_INVALID, "the documents given for the ctid lookup carry no payloads");
        if (payloads->n_docs != t->base_docs)  // (a handle that has grown: the appended documents' ctids are in its tail)
            return set_error(VBM25_ERR_INVALID, "the documents given for the ctid lookup are %u, the bound documents %u", payloads->n_docs, t->base_docs);
        if (payloads->device != t->device)
            return set_error(VBM25_ERR_INVALID, "the documents given for the ctid lookup are on device %d, the bound documents on device %d",
                             payloads->device, t->device);
    }
    const uint32_t n_tail = t->n_docs - t->base_docs;
    if ((payloads || from_index) && n_tail && !t->tail_payload)
        return set_error(VBM25_ERR_INVALID, "the %u documents appended to the bound documents carry no payloads: no ctid names them", n_tail);
    EvaluateTables ix;
    if (int rc = index_evaluate_tables(t->index, &ix)) return rc;
    if (ix.n_docs == 0) return set_error(VBM25_ERR_INVALID, "evaluate on an index without sealed documents");
    if (int rc = use_eval_device(t->device)) return rc;
    std::unique_ptr<vbm25_reranker, void (*)(vbm25_reranker *)> guard(new vbm25_reranker, vbm25_reranker_free);
    vbm25_reranker *r = guard.get();
    ResourceTally &ta = r->tally;
    r->t = t;
    r->device = t->device;
    r->ring.depth = depth;
    r->max_queries = max_queries;
    r->max_lexemes = max_lexemes;
    r->max_bytes = max_bytes;
    r->max_candidates = max_candidates;
    r->max_k = max_k;
    r->n_terms = v.n_terms;
    r->vocab = static_cast<const Key *>(v.keys);
    r->has_seed = sd.has_seed;
    r->seed = sd.seed;
    const bool has_payloads = payloads != nullptr || from_index;
    r->has_payloads = has_payloads;
    r->zero_off.assign(size_t(max_queries) + 1, 0u);
    // a query of several parts has more than `part` candidates, so its ceil(n / part) lists are fewer than 2 n / part; and every
    // query adds at most one list to the quotient of the whole
    const uint64_t part = rerank_part_now();
    r->max_lists = std::min(2 * (max_candidates / part) + 1, max_candidates / part + max_queries);
    const uint64_t nq1 = uint64_t(max_queries) + 1, nl1 = uint64_t(max_lexemes) + 1;
    r->in_capacity = Layout(max_queries, true, max_queries, max_lexemes, max_lexemes, max_candidates, has_payloads ? CAND_TID : CAND_DOC, max_bytes).bytes;
    const size_t out_bytes = size_t(max_queries) * max_k * sizeof(vbm25_rank) + 4ull * max_queries;
    for (uint32_t i = 0; i < depth; ++i) {
        RerankSlot &s = r->slots[i];
        HIP_TRY(ta.stream_create(s.stream));
        HIP_TRY(ta.event_create(s.start));
        HIP_TRY(ta.event_create(s.done));
        if (i == 0)
            if (int rc = pack_cub_bytes(max_queries, max_lexemes, s.stream.s, &r->cub_bytes)) return rc;
        HIP_TRY(ta.pinned_alloc(s.pin_in, r->in_capacity));
        HIP_TRY(ta.pinned_alloc(s.pin_out, out_bytes));
        HIP_TRY(ta.device_alloc(s.in, r->in_capacity));
        HIP_TRY(ta.device_alloc(s.ids, 4 * nl1));
        HIP_TRY(ta.device_alloc(s.tmp, 4 * nl1));
        HIP_TRY(ta.device_alloc(s.counts, 4 * nq1));
        HIP_TRY(ta.device_alloc(s.q_off, 4 * nq1));
        HIP_TRY(ta.device_alloc(s.sort_a, 8ull * max_lexemes));
        HIP_TRY(ta.device_alloc(s.sort_b, 8ull * max_lexemes + 4 * nl1));
        HIP_TRY(ta.device_alloc(s.cub, r->cub_bytes));
        HIP_TRY(ta.device_alloc(s.res_q_off, 4 * nq1));
        HIP_TRY(ta.device_alloc(s.res_ids, 4ull * max_lexemes));
        if (has_payloads) HIP_TRY(ta.device_alloc(s.cand_doc, 4 * max_candidates));
        HIP_TRY(ta.device_alloc(s.out, out_bytes));
        HIP_TRY(ta.device_alloc(s.scr, part_list_bytes(r->max_lists, max_k)));
    }
    if (payloads) {
        if (int rc = build_directory(r, payloads->d_payload.as<uint16_t>(), payloads->n_docs, t->d_tail_payload.as<uint16_t>(), n_tail)) return rc;
    } else if (from_index) {  // (an index-bound handle has the index's n_docs documents, in its order)
        const uint16_t *plane = nullptr;
        uint32_t n = 0;
        if (int rc = index_payloads(t->index, &plane, &n)) return rc;
        if (n != t->base_docs) return set_error(VBM25_ERR_INVALID, "the index has %u documents, the handle was bound with %u", n, t->base_docs);
        if (int rc = build_directory(r, plane, n, t->d_tail_payload.as<uint16_t>(), n_tail)) return rc;
    }
    *out = guard.release();
    return VBM25_OK;
}

// a batch's queries: lexemes (q32 = q_lex) or term ids (q32 = q_off)
struct Queries {
    bool lexemes;
    const uint8_t *bytes;
    const uint64_t *lex_off;
    const uint32_t *term_ids, *q32;
    uint32_t nq;
};

int reranker_submit(vbm25_reranker *r, const Queries &in, const uint64_t *q_cand, const uint32_t *cand_doc, const uint16_t *cand_tid, uint32_t k) {
    if (!r) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (cand_doc && cand_tid) return set_error(VBM25_ERR_INVALID, "cand_doc and cand_tid are both given: a batch's candidates come one way");
    if ((cand_doc || cand_tid) && !q_cand) return set_error(VBM25_ERR_INVALID, "%s is given without q_cand", cand_doc ? "cand_doc" : "cand_tid");
    if (cand_tid && !r->has_payloads) return set_error(VBM25_ERR_INVALID, "cand_tid on a reranker created without payloads");
    const uint32_t nq = in.nq;
    LexShape sh;
    if (in.lexemes)
        if (int rc = check_lexemes(r->has_seed, in.bytes, in.lex_off, in.q32, nq, &sh)) return rc;
    if (r->ring.full()) return set_error(VBM25_ERR_INVALID, "the reranker's %u slots are all in flight: collect first", r->ring.depth);
    if (nq > r->max_queries) return set_error(VBM25_ERR_INVALID, "%u queries exceed the reranker's max_queries %u", nq, r->max_queries);
    if (sh.n_lex > r->max_lexemes) return set_error(VBM25_ERR_INVALID, "%u lexemes exceed the reranker's max_lexemes %u", sh.n_lex, r->max_lexemes);
    if (sh.n_bytes > r->max_bytes)
        return set_error(VBM25_ERR_INVALID, "%llu bytes exceed the reranker's max_bytes %llu", (ull)sh.n_bytes, (ull)r->max_bytes);
    // the scorer's checks of the ids and the candidates.  A lexeme batch has no ids yet: its queries are checked as empty ones.
    const vbm25_doc_terms *t = r->t;
    EvaluateTables ix{};
    uint64_t n_pairs = 0;
    const uint32_t no_ids = 0;
    if (int rc = check_score_call(t, in.lexemes ? &no_ids : in.term_ids, in.lexemes ? r->zero_off.data() : in.q32, nq, q_cand, cand_doc, r, &ix,
                                  &n_pairs, cand_tid != nullptr))
        return rc;
    const uint32_t n_ids = in.lexemes || !nq ? 0u : in.q32[nq];
    if (n_ids > r->max_lexemes) return set_error(VBM25_ERR_INVALID, "%u term ids exceed the reranker's max_lexemes %u", n_ids, r->max_lexemes);
    if (k == 0) return set_error(VBM25_ERR_INVALID, "k is 0");
    if (k > r->max_k) return set_error(VBM25_ERR_INVALID, "k %u exceeds the reranker's max_k %u", k, r->max_k);
    if (n_pairs > r->max_candidates)
        return set_error(VBM25_ERR_INVALID, "%llu candidates exceed the reranker's max_candidates %llu", (ull)n_pairs, (ull)r->max_candidates);
    RerankSlot &s = r->slots[r->ring.tail()];
    if (n_pairs == 0) {  // no query has a candidate: nothing to enqueue, the batch keeps its place in the ring
        s.nq = nq;
        s.k = k;
        s.enqueued = false;
        r->last_path = PATH_NONE;
        r->ring.push();
        return VBM25_OK;
    }
    const uint32_t part = rerank_part_now(), buf = buffer_entries(k, rerank_buf_now());
    const UnitPlan plan = count_units(q_cand, t->n_docs, part, nq);
    if (plan.n_lists > r->max_lists)
        return set_error(VBM25_ERR_INVALID, "the batch needs %u part lists, a slot of the reranker holds %llu: rerank_part was lowered after create",
                         plan.n_lists, (ull)r->max_lists);
    if (int rc = use_eval_device(r->device)) return rc;
    const uint32_t kind = cand_tid ? CAND_TID : q_cand ? CAND_DOC : CAND_CROSS;
    const Layout g(nq, q_cand != nullptr, plan.n_multi, in.lexemes ? sh.n_lex : ~0ull, n_ids, n_pairs, kind, sh.n_bytes);
    uint8_t *host = s.pin_in.as<uint8_t>();
    const uint8_t *dev = s.in.as<uint8_t>();
    if (q_cand) std::memcpy(host + g.cand, q_cand, 8ull * (nq + 1ull));
    if (kind == CAND_DOC) std::memcpy(host + g.docs, cand_doc, 4ull * n_pairs);
    if (kind == CAND_TID) std::memcpy(host + g.docs, cand_tid, 6ull * n_pairs);
    std::memcpy(host + g.q32, in.q32, 4ull * (nq + 1ull));
    if (in.lexemes) {
        std::memcpy(host + g.lex_off, in.lex_off, 8ull * (sh.n_lex + 1ull));
        if (sh.n_bytes) std::memcpy(host + g.pool, in.bytes, sh.n_bytes);
    } else if (n_ids) {
        std::memcpy(host + g.ids, in.term_ids, 4ull * n_ids);
    }
    fill_units(q_cand, t->n_docs, part, nq, reinterpret_cast<uint32_t *>(host + g.unit), reinterpret_cast<uint32_t *>(host + g.scr),
               reinterpret_cast<uint32_t *>(host + g.multi));
    const size_t rank_bytes = size_t(nq) * k * sizeof(vbm25_rank), out_bytes = rank_bytes + 4ull * nq;
    const size_t list_entries = size_t(plan.n_lists) * k;
    TopkArgs a{};
    fill_score_tables(t, ix, &a.s);
    a.s.q_ids = in.lexemes ? s.res_ids.as<uint32_t>() : reinterpret_cast<const uint32_t *>(dev + g.ids);
    a.s.q_off = in.lexemes ? s.res_q_off.as<uint32_t>() : reinterpret_cast<const uint32_t *>(dev + g.q32);
    a.s.q_cand = q_cand ? reinterpret_cast<const ull *>(dev + g.cand) : nullptr;
    a.s.cand_doc = kind == CAND_TID ? s.cand_doc.as<uint32_t>() : kind == CAND_DOC ? reinterpret_cast<const uint32_t *>(dev + g.docs) : nullptr;
    a.s.cross_docs = q_cand ? 0u : t->n_docs;
    a.s.nq = nq;
    a.multi_q = reinterpret_cast<const uint32_t *>(dev + g.multi);
    a.out = reinterpret_cast<const TopkOut *>(dev + g.out);
    a.n_units = plan.n_units;
    a.n_multi = plan.n_multi;
    a.k = k;
    a.buf = buf;
    a.part = part;
    a.dead = t->d_dead.as<ull>();
    TopkOut o;
    o.unit_start = reinterpret_cast<const uint32_t *>(dev + g.unit);
    o.q_off = a.s.q_off;
    o.q_cand = a.s.q_cand;
    o.scr_start = reinterpret_cast<const uint32_t *>(dev + g.scr);
    o.scr_key = s.scr.as<ull>();
    o.scr_pos = reinterpret_cast<uint32_t *>(s.scr.as<uint8_t>() + 8ull * list_entries);
    o.scr_cnt = o.scr_pos + list_entries;
    o.ranks = s.out.as<vbm25_rank>();
    o.n_ranks = reinterpret_cast<uint32_t *>(s.out.as<uint8_t>() + rank_bytes);
    std::memcpy(host + g.out, &o, sizeof o);
    hipStream_t st = s.stream.s;
    Quiesce quiesce(st);  // (a failed step below leaves nothing in flight on the slot; let go of on success)
    HIP_TRY(hipMemcpyAsync(s.in.p, host, g.bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s.start.e, st));
    uint32_t path = PATH_NONE;
    if (in.lexemes) {
        if (int rc = launch_intern(st, r->seed, reinterpret_cast<const uint32_t *>(dev + g.pool), reinterpret_cast<const uint64_t *>(dev + g.lex_off),
                                   sh.n_lex, sh.longest_lexeme, r->vocab, r->n_terms, nullptr, s.ids.as<uint32_t>()))
            return rc;
        const PackScratch scratch{s.ids.as<uint32_t>(), s.tmp.as<uint32_t>(), s.counts.as<uint32_t>(), s.q_off.as<uint32_t>(),
                                  s.sort_a.as<ull>(), s.sort_b.as<ull>(), s.cub.p, r->cub_bytes, r->max_lexemes};
        if (int rc = enqueue_pack(st, scratch, reinterpret_cast<const uint32_t *>(dev + g.q32), nq, sh.n_lex, sh.longest_query,
                                  s.res_ids.as<uint32_t>(), s.res_q_off.as<uint32_t>()))
            return rc;
        path = sh.longest_query <= WAVE_QUERY ? PATH_WAVE : PATH_RADIX;
    }
    if (kind == CAND_TID) {
        const LookupArgs la{reinterpret_cast<const uint16_t *>(dev + g.docs), n_pairs, r->dir.as<ull>(), r->dir_keys.as<ull>(),
                            r->dir_docs.as<uint32_t>(), r->dir_n, r->n_dir, r->stride, s.cand_doc.as<uint32_t>(), t->d_dead.as<ull>()};
        const uint32_t cap = std::min(MAX_GRID, std::max(1u, eval_grid_cap()));
        cand_lookup_kernel<<<grid_for(n_pairs, WG, cap), WG, 8ull * std::max(1u, r->n_dir), st>>>(la);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(launch_topk(a, st));
    HIP_TRY(hipMemcpyAsync(s.pin_out.p, s.out.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(s.done.e, st));
    s.nq = nq;
    s.k = k;
    s.enqueued = true;
    r->last_path = path;
    r->ring.push();
    quiesce.s = nullptr;
    return VBM25_OK;
}

int reranker_collect(vbm25_reranker *r, vbm25_rank *ranks, uint32_t *n_ranks, uint32_t *nq_out, uint32_t *k_out) {
    if (!r || !nq_out || !k_out) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (r->ring.empty()) return set_error(VBM25_ERR_INVALID, "nothing is in flight on the reranker");
    RerankSlot &s = r->slots[r->ring.head];
    if (s.nq && (!ranks || !n_ranks)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    const size_t rank_bytes = size_t(s.nq) * s.k * sizeof(vbm25_rank);
    if (s.enqueued) {
        if (int rc = use_eval_device(r->device)) return rc;
        HIP_TRY(hipEventSynchronize(s.done.e));
        std::memcpy(ranks, s.pin_out.p, rank_bytes);
        std::memcpy(n_ranks, s.pin_out.as<uint8_t>() + rank_bytes, 4ull * s.nq);
    } else if (s.nq) {
        std::memset(ranks, 0, rank_bytes);
        std::memset(n_ranks, 0, 4ull * s.nq);
    }
    *nq_out = s.nq;
    *k_out = s.k;
    const int released = int(r->ring.pop());
    r->last_collected = s.enqueued ? released : -1;
    return VBM25_OK;
}

// vbm25_reranker_sync: the ctids of documents dir_n .. t->n_docs (the handle's tail) sorted, merged by rank into the spare arrays and the
// directory sampled again, all on slot 0's stream; the spares swapped in once every slot has finished
int reranker_sync(vbm25_reranker *r) {
    if (!r) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (!r->has_payloads) return set_error(VBM25_ERR_INVALID, "sync on a reranker created without payloads: it has no ctid directory");
    const vbm25_doc_terms *t = r->t;
    const uint32_t n_old = r->dir_n, n_new = t->n_docs, m = n_new - n_old;
    if (!m) return VBM25_OK;
    if (!t->tail_payload)
        return set_error(VBM25_ERR_INVALID, "the %u documents appended to the bound documents carry no payloads: no ctid names them", m);
    if (int rc = use_eval_device(r->device)) return rc;
    hipStream_t st = r->slots[0].stream.s;
    ResourceTally &ta = r->tally;
    const uint32_t sort_max = live::live_sort_max_now();
    const bool radix = m > sort_max;
    // Everything the sync needs, before anything is enqueued.  Capacities at least double (vbm25_documents_extend's factor).  What a
    // growth step replaces is only ever written by a sync (the spares, the scratch): nothing is copied.
    auto regrow = [&](HbmArray &a, size_t bytes) -> hipError_t {
        ta.device_bytes -= a.footprint();
        a.release();
        return ta.device_alloc(a, bytes);
    };
    constexpr size_t DIR_BYTES = 8ull << MAX_DIR_LOG2;  // (a directory of any shape)
    const uint64_t cap = n_new > r->dir_cap ? std::max<uint64_t>(n_new, 2 * r->dir_cap) : r->dir_cap;
    if (!r->dir_keys2.p || 8 * cap > r->dir_keys2.bytes) {
        HIP_TRY(regrow(r->dir_keys2, 8 * cap));
        HIP_TRY(regrow(r->dir_docs2, 4 * cap));
    }
    if (r->dir2.bytes < DIR_BYTES) HIP_TRY(regrow(r->dir2, DIR_BYTES));
    if (!r->sync_start.e) {
        HIP_TRY(ta.event_create(r->sync_start));
        HIP_TRY(ta.event_create(r->sync_done));
    }
    if (m > r->delta_cap) {  // the delta's scratch, the radix sort's included whichever sort this delta takes: a later sync that fits allocates nothing
        const uint64_t dcap = std::max<uint64_t>({m, 2 * r->delta_cap, live::LIVE_SORT_CAP});
        // hipcub's temporary storage is asked for dcap items and used for every m <= dcap: the requirement of a radix sort does not shrink
        // with its input (SortPairs refuses storage smaller than it needs, it does not write past it)
        size_t cub_bytes = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, (const ull *)nullptr, (ull *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                  int(dcap), 0, 48, st));
        HIP_TRY(regrow(r->delta_keys, 8 * dcap));
        HIP_TRY(regrow(r->delta_docs, 4 * dcap));
        HIP_TRY(regrow(r->delta_keys_in, 8 * dcap));
        HIP_TRY(regrow(r->delta_docs_in, 4 * dcap));
        HIP_TRY(regrow(r->delta_cub, cub_bytes));
        r->delta_cub_bytes = cub_bytes;
        r->delta_cap = dcap;
    }
    const DirShape shape = dir_shape(n_new, tid_dir_now());
    const uint16_t *tail = t->d_tail_payload.as<uint16_t>() + 3ull * (n_old - t->base_docs);
    Quiesce quiesce(st);  // (a failed step below leaves nothing in flight that reads the scratch)
    HIP_TRY(hipEventRecord(r->sync_start.e, st));
    if (radix) {
        payload_key_kernel<<<grid_for(m, WG, MAX_GRID), WG, 0, st>>>(tail, m, n_old, r->delta_keys_in.as<ull>(), r->delta_docs_in.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        size_t cub_bytes = r->delta_cub_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(r->delta_cub.p, cub_bytes, r->delta_keys_in.as<ull>(), r->delta_keys.as<ull>(),
                                                  r->delta_docs_in.as<uint32_t>(), r->delta_docs.as<uint32_t>(), int(m), 0, 48, st));
    } else {
        HIP_TRY(live::launch_live_sort(tail, m, n_old, r->delta_keys.as<ull>(), r->delta_docs.as<uint32_t>(), st));
    }
    const live::MergeArgs ma{r->dir_keys.as<ull>(), r->dir_docs.as<uint32_t>(), n_old, r->dir.as<ull>(), r->n_dir, r->stride, r->delta_keys.as<ull>(),
                             r->delta_docs.as<uint32_t>(), m, r->dir_keys2.as<ull>(), r->dir_docs2.as<uint32_t>()};
    HIP_TRY(live::launch_live_merge(ma, st));
    payload_dir_kernel<<<(shape.n_dir + WG - 1) / WG, WG, 0, st>>>(r->dir_keys2.as<ull>(), shape.n_dir, shape.stride, r->dir2.as<ull>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->sync_done.e, st));
    // a batch submitted before the sync reads the old arrays to its end: every slot has finished before the spares become the directory
    for (RerankSlot &s : r->slots)
        if (s.stream.s) HIP_TRY(hipStreamSynchronize(s.stream.s));
    HIP_TRY(elapsed_ms(r->sync_start, r->sync_done, &r->sync_ms));
    for (auto pr : {std::make_pair(&r->dir_keys, &r->dir_keys2), std::make_pair(&r->dir_docs, &r->dir_docs2), std::make_pair(&r->dir, &r->dir2)}) {
        std::swap(pr.first->p, pr.second->p);
        std::swap(pr.first->bytes, pr.second->bytes);
    }
    r->dir_n = n_new;
    r->dir_cap = cap;
    r->n_dir = shape.n_dir;
    r->stride = shape.stride;
    // the old arrays, now the spares, may be smaller than their partners: made again in this sync, so that the next one that fits
    // allocates nothing.  The sync has taken effect: an allocation that fails here leaves a spare empty, which the next sync makes
    // again (and reports, if it fails again) -- this one returns VBM25_OK.
    if (8 * cap > r->dir_keys2.bytes && (regrow(r->dir_keys2, 8 * cap) != hipSuccess || regrow(r->dir_docs2, 4 * cap) != hipSuccess))
        for (HbmArray *a : {&r->dir_keys2, &r->dir_docs2}) {
            ta.device_bytes -= a->p ? a->footprint() : 0;
            a->release();
        }
    if (r->dir2.bytes < DIR_BYTES && regrow(r->dir2, DIR_BYTES) != hipSuccess) r->dir2.release();
    (void)hipGetLastError();  // (a failed allocation above is not the next call's error)
    return VBM25_OK;
}

}  // namespace

extern "C" {

int vbm25_reranker_sync(vbm25_reranker *r) {
    return guarded([&] { return reranker_sync(r); });
}

uint32_t vbm25_reranker_directory_docs(const vbm25_reranker *r) { return r ? r->dir_n : 0; }

// tools/live_rerank_cost.py: the device time of the last sync's kernels between its events (-1: no sync has enqueued anything).  Not in
// the header.
int vbm25_debug_reranker_sync_ms(const vbm25_reranker *r, double *ms) {
    if (!r || !ms) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *ms = r->sync_ms;
    return VBM25_OK;
}

int vbm25_reranker_create(const vbm25_doc_terms *t, const vbm25_resolver *rs, const vbm25_documents *payloads, uint32_t depth, uint32_t max_queries,
                          uint32_t max_lexemes, uint64_t max_bytes, uint64_t max_candidates, uint32_t max_k, vbm25_reranker **out) {
    return guarded([&] { return reranker_create(t, rs, payloads, false, depth, max_queries, max_lexemes, max_bytes, max_candidates, max_k, out); });
}

int vbm25_reranker_create_from_index(const vbm25_doc_terms *t, const vbm25_resolver *rs, uint32_t depth, uint32_t max_queries, uint32_t max_lexemes,
                                     uint64_t max_bytes, uint64_t max_candidates, uint32_t max_k, vbm25_reranker **out) {
    return guarded([&] { return reranker_create(t, rs, nullptr, true, depth, max_queries, max_lexemes, max_bytes, max_candidates, max_k, out); });
}

void vbm25_reranker_free(vbm25_reranker *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    for (RerankSlot &s : r->slots)
        if (s.stream.s) (void)hipStreamSynchronize(s.stream.s);  // nothing is freed under a kernel or a copy in flight
    delete r;
}

uint64_t vbm25_reranker_device_bytes(const vbm25_reranker *r) { return r ? r->tally.device_bytes : 0; }

int vbm25_reranker_info(const vbm25_reranker *r, uint32_t *depth, uint32_t *n_docs, uint32_t *has_payloads, uint64_t *allocations) {
    if (!r) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (depth) *depth = r->ring.depth;
    if (n_docs) *n_docs = r->t->n_docs;
    if (has_payloads) *has_payloads = r->has_payloads ? 1u : 0u;
    if (allocations) *allocations = r->tally.allocations;
    return VBM25_OK;
}

int vbm25_reranker_submit_lexemes(vbm25_reranker *r, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex, uint32_t nq,
                                  const uint64_t *q_cand, const uint32_t *cand_doc, const uint16_t *cand_tid, uint32_t k) {
    return guarded([&] { return reranker_submit(r, Queries{true, bytes, lex_off, nullptr, q_lex, nq}, q_cand, cand_doc, cand_tid, k); });
}

int vbm25_reranker_submit_ids(vbm25_reranker *r, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, const uint64_t *q_cand,
                              const uint32_t *cand_doc, const uint16_t *cand_tid, uint32_t k) {
    return guarded([&] { return reranker_submit(r, Queries{false, nullptr, nullptr, term_ids, q_off, nq}, q_cand, cand_doc, cand_tid, k); });
}

int vbm25_reranker_collect(vbm25_reranker *r, vbm25_rank *ranks, uint32_t *n_ranks, uint32_t *nq_out, uint32_t *k_out) {
    return guarded([&] { return reranker_collect(r, ranks, n_ranks, nq_out, k_out); });
}

int vbm25_reranker_in_flight(const vbm25_reranker *r) { return r ? int(r->ring.count) : 0; }

// tools/reranker_cost.py and the tests of the pack paths: the device time of the last collected batch between its slot's events (the
// upload excluded, the rows' download included; -1 when that batch enqueued nothing), the pack path of the last accepted submit (0 none,
// 1 one wave a query, 2 the radix sort), and the device time of the payload directory's build (-1 without payloads).  Not in the header.
int vbm25_debug_reranker(const vbm25_reranker *r, double *batch_ms, uint32_t *pack_path, double *directory_ms) {
    if (!r) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (batch_ms) {
        *batch_ms = -1.0;
        if (r->last_collected >= 0) {
            const RerankSlot &s = r->slots[r->last_collected];
            HIP_TRY(elapsed_ms(s.start, s.done, batch_ms));
        }
    }
    if (pack_path) *pack_path = r->last_path;
    if (directory_ms) *directory_ms = r->directory_ms;
    return VBM25_OK;
}

}  // extern "C"
