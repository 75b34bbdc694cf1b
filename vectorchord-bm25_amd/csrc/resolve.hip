// resolve.hip -- the query resolver: cast_tsvector_to_query (src/datatype/tsvector.rs:96-105: intern every lexeme, sort, dedup) and
// the key lookup of bm25::search (address_tokens::read, search.rs:59-61: keys the index lacks are dropped) on the device, batched.
// Lexemes or 16-byte keys in, ascending term ids out, as a CSR term_ids / q_off in pinned host memory -- the form every search entry
// point takes.  resolve_lane.h holds the per-lexeme and per-key functions; the kernels here are loops over them.
//
// Why sorting ids is the reference's sort: the vocabulary is ascending by key (memcmp order) and term id = position in it.  Two keys
// that the index holds therefore compare as their ids do, equal keys have equal ids, and a key the index lacks has no id.  Sorting the
// FOUND ids ascending and dropping repeats and misses gives exactly the ids of (sort keys, dedup keys, drop unknown keys), in the same
// order -- without ever sorting 16-byte keys.
//
//   per batch, all on the resolver's own stream (nothing synchronises the device or touches the index's batches):
//     upload            the slot's pinned block (q_lex | lex_off | bytes, or q_key | keys) in ONE copy into the device staging
//     intern_kernel     one lane a lexeme: intern_lane -> key -> lookup_lane -> id            (lexeme entry)
//     lookup_kernel     one lane a key: lookup_lane -> id                                     (keys entry)
//     step (c), every query of the batch <= 64 lexemes  -- the wave path:
//       pack_wave_kernel   one wave a query, one lane a lexeme: duplicates (an equal id in a lower lane) and misses leave by ballot, a
//                          lane's rank is the number of surviving lower ids (cross-lane compares, no LDS, no sort); the survivors go
//                          to tmp[q_lex[q] + rank] and the query's count to counts[q]
//       (scan)             exclusive sum of the counts -> q_off (hipcub)
//       gather_kernel      one wave a query: tmp -> term_ids[q_off[q] ..) and q_off, both in pinned host memory
//     step (c), otherwise -- the general path, any query length up to the capacity:
//       sortkey_kernel     one lane a lexeme: (query << 32 | id), the query by bisection of q_lex
//       (radix sort)       hipcub, the bits of the id and of the query number only; a query keeps its range q_lex[q] .. q_lex[q + 1]
//       flag_kernel        first of its run and found -> 1
//       (scan)             exclusive sum of the flags -> position
//       emit_kernel        term_ids[position] and q_off[q] = position[q_lex[q]], both in pinned host memory
//   Both paths write identical bytes; the switch is the longest query of the batch, which submit knows from validating q_lex.
//   The chaining-value stack of lexemes over 1024 bytes lives in LDS, sized per launch from the batch's longest lexeme (0 bytes when
//   every lexeme fits a chunk): no kernel here has scratch memory.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "vbm25_internal.h"
#include "hip_host.h"
#include "ring.h"
#include "resolve_lane.h"
#include "lexeme_input.h"
#include "resolve_shared.h"

namespace {

using namespace vbm25;
using namespace vbm25::rsv;
using vbm25::lexin::MAX_LEVELS;
using vbm25::lexin::NEEDS_SEED;
using vbm25::lexin::Seed;
using vbm25::lexin::seed_words;

constexpr uint32_t INTERN_THREADS = 64;   // one wave a block: the LDS stack is 32 bytes a level a lane
constexpr uint32_t INTERN_GRID = 1024;    // one wave a SIMD of the 256 CUs; more lexemes than 65536 stride the grid
constexpr uint32_t WG_THREADS = 256, MAX_GRID = 2048;

// keys_out and ids may each be NULL.  The pool is 4-byte aligned and ends on a multiple of 4 (WordLoad).
__global__ void __launch_bounds__(INTERN_THREADS) intern_kernel(Seed seed, const uint32_t *pool, const uint64_t *lex_off, uint32_t n_lex,
                                                                const Key *vocab, uint32_t n_terms, Key *keys_out, uint32_t *ids) {
    extern __shared__ uint32_t cv_stack[];
    const WordLoad ld{pool};
    for (uint32_t i = blockIdx.x * INTERN_THREADS + threadIdx.x; i < n_lex; i += gridDim.x * INTERN_THREADS) {
        const uint64_t begin = lex_off[i];
        const Key key = intern_lane(seed.w, ld, begin, lex_off[i + 1] - begin, cv_stack + threadIdx.x, INTERN_THREADS);
        if (keys_out) keys_out[i] = key;
        if (ids) ids[i] = lookup_lane(vocab, n_terms, key);
    }
}

__global__ void __launch_bounds__(WG_THREADS) lookup_kernel(const Key *keys, uint32_t n, const Key *vocab, uint32_t n_terms, uint32_t *ids) {
    for (uint32_t i = blockIdx.x * WG_THREADS + threadIdx.x; i < n; i += gridDim.x * WG_THREADS) ids[i] = lookup_lane(vocab, n_terms, keys[i]);
}

// the wave path; every query has at most 64 lexemes.  counts has nq + 1 entries, the last one 0 (the scan's total lands there).
__global__ void __launch_bounds__(WG_THREADS) pack_wave_kernel(const uint32_t *ids, const uint32_t *q_lex, uint32_t nq, uint32_t *tmp,
                                                               uint32_t *counts) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[nq] = 0;
    for (uint32_t q = wave; q < nq; q += n_waves) {
        const uint32_t b = q_lex[q], n = q_lex[q + 1] - b;
        const uint32_t id = lane < n ? ids[b + lane] : NOT_FOUND;
        bool dup = false;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t v = __shfl(id, j);
            dup |= v == id && j < lane;
        }
        const bool keep = id != NOT_FOUND && !dup;
        const unsigned long long kept = __ballot(keep);
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t v = __shfl(id, j);
            rank += ((kept >> j) & 1ull) && v < id;
        }
        if (keep) tmp[b + rank] = id;
        if (lane == 0) counts[q] = __popcll(kept);
    }
}

__global__ void __launch_bounds__(WG_THREADS) gather_kernel(const uint32_t *tmp, const uint32_t *q_lex, const uint32_t *q_off, uint32_t nq,
                                                            uint32_t *out_ids, uint32_t *out_q_off) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) out_q_off[nq] = q_off[nq];
    for (uint32_t q = wave; q < nq; q += n_waves) {
        const uint32_t o = q_off[q], c = q_off[q + 1] - o;
        if (lane < c) out_ids[o + lane] = tmp[q_lex[q] + lane];
        if (lane == 0) out_q_off[q] = o;
    }
}

// the general path
__global__ void __launch_bounds__(WG_THREADS) sortkey_kernel(const uint32_t *ids, const uint32_t *q_lex, uint32_t nq, uint32_t n_lex,
                                                             unsigned long long *keys) {
    for (uint32_t i = blockIdx.x * WG_THREADS + threadIdx.x; i < n_lex; i += gridDim.x * WG_THREADS) {
        uint32_t lo = 0, hi = nq;  // the last q with q_lex[q] <= i (empty queries in front of it share its start)
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (q_lex[mid] <= i) lo = mid; else hi = mid;
        }
        keys[i] = (unsigned long long)lo << 32 | ids[i];
    }
}

__global__ void __launch_bounds__(WG_THREADS) flag_kernel(const unsigned long long *sorted, uint32_t n_lex, uint32_t *flags) {
    if (blockIdx.x == 0 && threadIdx.x == 0) flags[n_lex] = 0;
    for (uint32_t i = blockIdx.x * WG_THREADS + threadIdx.x; i < n_lex; i += gridDim.x * WG_THREADS) {
        const unsigned long long k = sorted[i];
        flags[i] = uint32_t(k) != NOT_FOUND && (i == 0 || sorted[i - 1] != k);
    }
}

__global__ void __launch_bounds__(WG_THREADS) emit_kernel(const unsigned long long *sorted, const uint32_t *flags, const uint32_t *pos,
                                                          const uint32_t *q_lex, uint32_t nq, uint32_t n_lex, uint32_t *out_ids,
                                                          uint32_t *out_q_off) {
    const uint32_t units = n_lex > nq + 1 ? n_lex : nq + 1;
    for (uint32_t i = blockIdx.x * WG_THREADS + threadIdx.x; i < units; i += gridDim.x * WG_THREADS) {
        if (i < n_lex && flags[i]) out_ids[pos[i]] = uint32_t(sorted[i]);
        if (i <= nq) out_q_off[i] = pos[q_lex[i]];
    }
}

}  // namespace

namespace vbm25 {
namespace rsv {

int check_offsets32(const uint32_t *q, uint32_t nq, const char *what, LexShape *s) {
    if (q[0] != 0) return set_error(VBM25_ERR_INVALID, "%s[0] is %u, not 0", what, q[0]);
    for (uint32_t i = 0; i < nq; ++i) {
        if (q[i + 1] < q[i]) return set_error(VBM25_ERR_INVALID, "%s is not monotone at query %u", what, i);
        s->longest_query = std::max(s->longest_query, q[i + 1] - q[i]);
    }
    s->n_lex = q[nq];
    return VBM25_OK;
}
int check_lexemes(bool has_seed, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex, uint32_t nq, LexShape *s) {
    if (!q_lex || !lex_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = check_offsets32(q_lex, nq, "q_lex", s)) return rc;
    return lexin::check_pool(has_seed, bytes, lex_off, s->n_lex, "resolver", &s->n_bytes, &s->longest_lexeme);
}

int pack_cub_bytes(uint32_t max_queries, uint32_t max_lexemes, hipStream_t st, size_t *bytes) {
    size_t scan_q = 0, scan_l = 0, sort_l = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_q, (uint32_t *)nullptr, (uint32_t *)nullptr, int(max_queries + 1), st));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_l, (uint32_t *)nullptr, (uint32_t *)nullptr, int(size_t(max_lexemes) + 1), st));
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_l, (unsigned long long *)nullptr, (unsigned long long *)nullptr, int(max_lexemes), 0, 64, st));
    *bytes = std::max(scan_q, std::max(scan_l, sort_l));
    return VBM25_OK;
}

int launch_intern(hipStream_t st, const Seed &seed, const uint32_t *pool, const uint64_t *lex_off, uint32_t n_lex, uint64_t longest,
                  const Key *vocab, uint32_t n_terms, Key *keys_out, uint32_t *ids) {
    if (!n_lex) return VBM25_OK;
    const size_t lds = size_t(stack_levels(longest)) * 8 * sizeof(uint32_t) * INTERN_THREADS;
    intern_kernel<<<std::min(INTERN_GRID, grid_for(n_lex, INTERN_THREADS, MAX_GRID)), INTERN_THREADS, lds, st>>>(seed, pool, lex_off, n_lex, vocab, n_terms, keys_out, ids);
    HIP_TRY(hipGetLastError());
    return VBM25_OK;
}

int enqueue_pack(hipStream_t st, const PackScratch &s, const uint32_t *q_lex_dev, uint32_t nq, uint32_t n_lex, uint32_t longest_query,
                 uint32_t *out_ids, uint32_t *out_q_off) {
    if (longest_query <= WAVE_QUERY) {
        pack_wave_kernel<<<grid_for(nq, WG_THREADS / 64, MAX_GRID), WG_THREADS, 0, st>>>(s.ids, q_lex_dev, nq, s.tmp, s.counts);
        HIP_TRY(hipGetLastError());
        size_t tb = s.cub_bytes;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.cub, tb, s.counts, s.q_off, int(nq + 1), st));
        gather_kernel<<<grid_for(nq, WG_THREADS / 64, MAX_GRID), WG_THREADS, 0, st>>>(s.tmp, q_lex_dev, s.q_off, nq, out_ids, out_q_off);
        HIP_TRY(hipGetLastError());
    } else {
        unsigned long long *ka = s.sort_a, *kb = s.sort_b;
        uint32_t *flags = reinterpret_cast<uint32_t *>(kb + s.max_lexemes), *pos = s.tmp;
        sortkey_kernel<<<grid_for(n_lex, WG_THREADS, MAX_GRID), WG_THREADS, 0, st>>>(s.ids, q_lex_dev, nq, n_lex, ka);
        HIP_TRY(hipGetLastError());
        int q_bits = 0;
        while (q_bits < 32 && (uint64_t(nq) >> q_bits)) ++q_bits;
        size_t tb = s.cub_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortKeys(s.cub, tb, ka, kb, int(n_lex), 0, 32 + q_bits, st));
        flag_kernel<<<grid_for(n_lex, WG_THREADS, MAX_GRID), WG_THREADS, 0, st>>>(kb, n_lex, flags);
        HIP_TRY(hipGetLastError());
        tb = s.cub_bytes;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.cub, tb, flags, pos, int(n_lex + 1), st));
        emit_kernel<<<grid_for(std::max(n_lex, nq + 1), WG_THREADS, MAX_GRID), WG_THREADS, 0, st>>>(kb, flags, pos, q_lex_dev, nq, n_lex, out_ids, out_q_off);
        HIP_TRY(hipGetLastError());
    }
    return VBM25_OK;
}

}  // namespace rsv
}  // namespace vbm25

namespace {

struct Slot {
    PinnedHost in;   // the staged block of one batch
    PinnedHost out;  // q_off (max_queries + 1) then term_ids (max_lexemes), as uint32_t
    Event start, done;
    uint32_t nq = 0;
};

}  // namespace

// vbm25_resolver_destroy waits for the stream before it deletes: the order of the members below does not matter to their destructors.
struct vbm25_resolver {
    const vbm25_index *index = nullptr;
    int device = 0;
    uint32_t max_queries = 0, max_lexemes = 0, n_terms = 0;
    uint64_t max_bytes = 0;
    bool has_seed = false;
    Seed seed{};
    Stream stream;  // the one stream of every slot
    size_t in_capacity = 0, cub_bytes = 0;
    ResourceTally tally;
    HbmArray vocab, in_dev, ids, tmp, counts, q_off, sort_a, sort_b, cub;
    Slot slots[16];
    RingCursor ring;
    int last_collected = -1;
};

namespace {

int resolver_create(vbm25_index *ix, const uint8_t *seed32, uint32_t depth, uint32_t max_queries, uint32_t max_lexemes, uint64_t max_bytes,
                    vbm25_resolver **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ix) return set_error(VBM25_ERR_INVALID, "index is NULL");
    if (depth < 1 || depth > 16) return set_error(VBM25_ERR_INVALID, "depth %u is outside 1 .. 16", depth);
    if (!max_queries || !max_lexemes) return set_error(VBM25_ERR_INVALID, "max_queries or max_lexemes is 0");
    if (max_queries >= (1u << 31) || max_lexemes >= (1u << 31)) return set_error(VBM25_ERR_INVALID, "max_queries or max_lexemes is 2^31 or more");
    int device = 0;
    uint32_t n_terms = 0;
    const uint8_t *term_key = nullptr;
    if (int rc = index_vocabulary(ix, &device, &n_terms, &term_key)) return rc;
    if (int rc = use_device(device)) return rc;
    std::unique_ptr<vbm25_resolver, void (*)(vbm25_resolver *)> guard(new vbm25_resolver, vbm25_resolver_destroy);
    vbm25_resolver *r = guard.get();
    r->index = ix;
    r->device = device;
    r->ring.depth = depth;
    r->max_queries = max_queries;
    r->max_lexemes = max_lexemes;
    r->max_bytes = max_bytes;
    r->n_terms = n_terms;
    r->has_seed = seed32 != nullptr;
    seed_words(seed32, &r->seed);
    ResourceTally &ta = r->tally;
    HIP_TRY(ta.stream_create(r->stream));
    // the staged block: q_lex | lex_off | bytes (rounded up to 4), or q_key | keys
    const size_t head_bytes = align_up(align_up(4ull * (max_queries + 1), 8) + 8ull * (max_lexemes + 1), 16);
    r->in_capacity = head_bytes + std::max<size_t>(align_up(max_bytes, 4), 16ull * max_lexemes);
    const size_t n1 = size_t(max_lexemes) + 1;
    if (int rc = pack_cub_bytes(max_queries, max_lexemes, r->stream.s, &r->cub_bytes)) return rc;
    HIP_TRY(ta.device_alloc(r->vocab, 16ull * n_terms));  // (a footprint of 16 for the vocabulary of an index without terms)
    HIP_TRY(ta.device_alloc(r->in_dev, r->in_capacity));
    HIP_TRY(ta.device_alloc(r->ids, 4 * n1));       // ids; the general path's flags
    HIP_TRY(ta.device_alloc(r->tmp, 4 * n1));       // the wave path's packed ids; the general path's positions
    HIP_TRY(ta.device_alloc(r->counts, 4ull * (max_queries + 1)));
    HIP_TRY(ta.device_alloc(r->q_off, 4ull * (max_queries + 1)));
    HIP_TRY(ta.device_alloc(r->sort_a, 8ull * max_lexemes));
    HIP_TRY(ta.device_alloc(r->sort_b, 8ull * max_lexemes + 4 * n1));  // the sorted keys, then the general path's flags
    HIP_TRY(ta.device_alloc(r->cub, r->cub_bytes));
    if (n_terms) HIP_TRY(hipMemcpyAsync(r->vocab.p, term_key, 16ull * n_terms, hipMemcpyHostToDevice, r->stream.s));
    for (uint32_t i = 0; i < depth; ++i) {
        Slot &s = r->slots[i];
        HIP_TRY(ta.pinned_alloc(s.in, r->in_capacity));
        HIP_TRY(ta.pinned_alloc(s.out, 4ull * (max_queries + 1) + 4ull * max_lexemes));
        HIP_TRY(ta.event_create(s.start));
        HIP_TRY(ta.event_create(s.done));
    }
    HIP_TRY(hipStreamSynchronize(r->stream.s));  // (the index's host keys are not read after create)
    *out = guard.release();
    return VBM25_OK;
}

// step (c) and the slot's completion, after the ids are in r->ids
int enqueue_pack(vbm25_resolver *r, Slot &s, const uint32_t *q_lex_dev, uint32_t nq, uint32_t n_lex, uint32_t longest_query) {
    const PackScratch scratch{r->ids.as<uint32_t>(), r->tmp.as<uint32_t>(), r->counts.as<uint32_t>(), r->q_off.as<uint32_t>(),
                              r->sort_a.as<unsigned long long>(), r->sort_b.as<unsigned long long>(), r->cub.p, r->cub_bytes, r->max_lexemes};
    uint32_t *out = s.out.as<uint32_t>();
    if (int rc = rsv::enqueue_pack(r->stream.s, scratch, q_lex_dev, nq, n_lex, longest_query, out + (r->max_queries + 1), out)) return rc;
    HIP_TRY(hipEventRecord(s.done.e, r->stream.s));
    return VBM25_OK;
}

int submit_common(vbm25_resolver *r, uint32_t nq) {
    if (r->ring.full()) return set_error(VBM25_ERR_INVALID, "the resolver's %u slots are all in flight: collect first", r->ring.depth);
    if (nq > r->max_queries) return set_error(VBM25_ERR_INVALID, "%u queries exceed the resolver's max_queries %u", nq, r->max_queries);
    return VBM25_OK;
}

int resolver_submit_lexemes(vbm25_resolver *r, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex, uint32_t nq) {
    if (!r) return set_error(VBM25_ERR_INVALID, "NULL argument");
    LexShape sh;
    if (int rc = check_lexemes(r->has_seed, bytes, lex_off, q_lex, nq, &sh)) return rc;
    if (int rc = submit_common(r, nq)) return rc;
    if (sh.n_lex > r->max_lexemes) return set_error(VBM25_ERR_INVALID, "%u lexemes exceed the resolver's max_lexemes %u", sh.n_lex, r->max_lexemes);
    if (sh.n_bytes > r->max_bytes) return set_error(VBM25_ERR_INVALID, "%llu bytes exceed the resolver's max_bytes %llu", (unsigned long long)sh.n_bytes, (unsigned long long)r->max_bytes);
    if (int rc = use_device(r->device)) return rc;
    Slot &s = r->slots[r->ring.tail()];
    const size_t o_lex = align_up(4ull * (nq + 1), 8), o_bytes = align_up(o_lex + 8ull * (sh.n_lex + 1), 16), total = o_bytes + align_up(sh.n_bytes, 4);
    uint8_t *in = s.in.as<uint8_t>();
    std::memcpy(in, q_lex, 4ull * (nq + 1));
    std::memcpy(in + o_lex, lex_off, 8ull * (sh.n_lex + 1));
    if (sh.n_bytes) std::memcpy(in + o_bytes, bytes, sh.n_bytes);
    uint8_t *d = r->in_dev.as<uint8_t>();
    Quiesce quiesce(r->stream.s);  // (a failed step below leaves nothing in flight on the slot; let go of on success)
    HIP_TRY(hipMemcpyAsync(d, in, total, hipMemcpyHostToDevice, r->stream.s));
    HIP_TRY(hipEventRecord(s.start.e, r->stream.s));
    const uint32_t *q_lex_dev = reinterpret_cast<const uint32_t *>(d);
    if (int rc = launch_intern(r->stream.s, r->seed, reinterpret_cast<const uint32_t *>(d + o_bytes), reinterpret_cast<const uint64_t *>(d + o_lex),
                               sh.n_lex, sh.longest_lexeme, r->vocab.as<Key>(), r->n_terms, nullptr, r->ids.as<uint32_t>()))
        return rc;
    if (int rc = enqueue_pack(r, s, q_lex_dev, nq, sh.n_lex, sh.longest_query)) return rc;
    s.nq = nq;
    r->ring.push();
    quiesce.s = nullptr;
    return VBM25_OK;
}

int resolver_submit_keys(vbm25_resolver *r, const uint8_t *keys16, const uint32_t *q_key, uint32_t nq) {
    if (!r || !q_key) return set_error(VBM25_ERR_INVALID, "NULL argument");
    LexShape sh;
    if (int rc = check_offsets32(q_key, nq, "q_key", &sh)) return rc;
    if (sh.n_lex && !keys16) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = submit_common(r, nq)) return rc;
    if (sh.n_lex > r->max_lexemes) return set_error(VBM25_ERR_INVALID, "%u keys exceed the resolver's max_lexemes %u", sh.n_lex, r->max_lexemes);
    if (int rc = use_device(r->device)) return rc;
    Slot &s = r->slots[r->ring.tail()];
    const size_t o_keys = align_up(4ull * (nq + 1), 16), total = o_keys + 16ull * sh.n_lex;
    uint8_t *in = s.in.as<uint8_t>();
    std::memcpy(in, q_key, 4ull * (nq + 1));
    if (sh.n_lex) std::memcpy(in + o_keys, keys16, 16ull * sh.n_lex);
    uint8_t *d = r->in_dev.as<uint8_t>();
    Quiesce quiesce(r->stream.s);  // (as in resolver_submit_lexemes)
    HIP_TRY(hipMemcpyAsync(d, in, total, hipMemcpyHostToDevice, r->stream.s));
    HIP_TRY(hipEventRecord(s.start.e, r->stream.s));
    if (sh.n_lex) {
        lookup_kernel<<<grid_for(sh.n_lex, WG_THREADS, MAX_GRID), WG_THREADS, 0, r->stream.s>>>(reinterpret_cast<const Key *>(d + o_keys), sh.n_lex, r->vocab.as<Key>(),
                                                                                     r->n_terms, r->ids.as<uint32_t>());
        HIP_TRY(hipGetLastError());
    }
    if (int rc = enqueue_pack(r, s, reinterpret_cast<const uint32_t *>(d), nq, sh.n_lex, sh.longest_query)) return rc;
    s.nq = nq;
    r->ring.push();
    quiesce.s = nullptr;
    return VBM25_OK;
}

int resolver_collect(vbm25_resolver *r, uint32_t *term_ids, uint32_t *q_off, uint32_t *nq_out) {
    if (!r || !q_off || !nq_out) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (r->ring.empty()) return set_error(VBM25_ERR_INVALID, "nothing is in flight on the resolver");
    if (int rc = use_device(r->device)) return rc;
    Slot &s = r->slots[r->ring.head];
    HIP_TRY(hipEventSynchronize(s.done.e));
    const uint32_t *out = s.out.as<uint32_t>(), n_ids = out[s.nq];
    if (n_ids && !term_ids) return set_error(VBM25_ERR_INVALID, "NULL argument");
    std::memcpy(q_off, out, 4ull * (s.nq + 1));
    if (n_ids) std::memcpy(term_ids, out + (r->max_queries + 1), 4ull * n_ids);
    *nq_out = s.nq;
    r->last_collected = int(r->ring.pop());
    return VBM25_OK;
}

int intern_batch_device(int device, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off, uint32_t n_lex, uint8_t *keys16) {
    if (!lex_off || (n_lex && !keys16)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    LexShape sh;
    const uint32_t one_query[2] = {0, n_lex};
    if (int rc = check_lexemes(seed32 != nullptr, bytes, lex_off, one_query, 1, &sh)) return rc;
    if (int rc = use_device(device)) return rc;
    if (!n_lex) return VBM25_OK;
    Seed seed;
    seed_words(seed32, &seed);
    const size_t o_bytes = align_up(8ull * (n_lex + 1), 16), total = o_bytes + align_up(sh.n_bytes, 4);
    std::vector<uint8_t> stage(total, 0);
    std::memcpy(stage.data(), lex_off, 8ull * (n_lex + 1));
    if (sh.n_bytes) std::memcpy(stage.data() + o_bytes, bytes, sh.n_bytes);
    HbmArray in, keys;
    Stream st;  // (a stream of its own: a launch on the null stream would wait for every other stream of the device)
    HIP_TRY(st.create());
    Quiesce quiesce(st.s);  // (behind the buffers and the stream: waited for before the one is destroyed and the others are freed)
    HIP_TRY(in.alloc(total));
    HIP_TRY(keys.alloc(16ull * n_lex));
    HIP_TRY(hipMemcpyAsync(in.p, stage.data(), total, hipMemcpyHostToDevice, st.s));
    if (int rc = launch_intern(st.s, seed, reinterpret_cast<const uint32_t *>(in.as<uint8_t>() + o_bytes), in.as<uint64_t>(), n_lex, sh.longest_lexeme,
                               nullptr, 0, keys.as<Key>(), nullptr))
        return rc;
    HIP_TRY(hipMemcpyAsync(keys16, keys.p, 16ull * n_lex, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    return VBM25_OK;
}

int search_batch_lexemes(vbm25_index *ix, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex, uint32_t nq,
                         uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    if (!ix) return set_error(VBM25_ERR_INVALID, "index is NULL");
    LexShape sh;
    if (int rc = check_lexemes(seed32 != nullptr, bytes, lex_off, q_lex, nq, &sh)) return rc;
    vbm25_resolver *r = nullptr;
    if (int rc = resolver_create(ix, seed32, 1, std::max(nq, 1u), std::max(sh.n_lex, 1u), sh.n_bytes, &r)) return rc;
    std::unique_ptr<vbm25_resolver, void (*)(vbm25_resolver *)> free_it(r, vbm25_resolver_destroy);
    std::vector<uint32_t> term_ids(std::max(sh.n_lex, 1u)), q_off(size_t(nq) + 1);
    uint32_t got = 0;
    if (int rc = resolver_submit_lexemes(r, bytes, lex_off, q_lex, nq)) return rc;
    if (int rc = resolver_collect(r, term_ids.data(), q_off.data(), &got)) return rc;
    return vbm25_search_batch(ix, term_ids.data(), q_off.data(), nq, k, hits, n_hits);
}

}  // namespace

namespace vbm25 {
int resolver_vocabulary(const vbm25_resolver *r, ResolverVocabulary *out) {
    *out = ResolverVocabulary{r->index, r->device, r->n_terms, r->vocab.p};
    return VBM25_OK;
}
namespace rsv {
int resolver_seed(const vbm25_resolver *r, ResolverSeed *out) {
    *out = ResolverSeed{r->has_seed, r->seed};
    return VBM25_OK;
}
}  // namespace rsv
}  // namespace vbm25

extern "C" {

int vbm25_resolver_create(vbm25_index *ix, const uint8_t *seed32, uint32_t depth, uint32_t max_queries, uint32_t max_lexemes, uint64_t max_bytes,
                          vbm25_resolver **out) {
    return guarded([&] { return resolver_create(ix, seed32, depth, max_queries, max_lexemes, max_bytes, out); });
}

void vbm25_resolver_destroy(vbm25_resolver *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream.s) (void)hipStreamSynchronize(r->stream.s);  // nothing is freed under a kernel or a copy in flight
    delete r;
}

uint64_t vbm25_resolver_device_bytes(const vbm25_resolver *r) { return r ? r->tally.device_bytes : 0; }

int vbm25_resolver_submit_lexemes(vbm25_resolver *r, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex, uint32_t nq) {
    return guarded([&] { return resolver_submit_lexemes(r, bytes, lex_off, q_lex, nq); });
}

int vbm25_resolver_submit_keys(vbm25_resolver *r, const uint8_t *keys16, const uint32_t *q_key, uint32_t nq) {
    return guarded([&] { return resolver_submit_keys(r, keys16, q_key, nq); });
}

int vbm25_resolver_collect(vbm25_resolver *r, uint32_t *term_ids, uint32_t *q_off, uint32_t *nq_out) {
    return guarded([&] { return resolver_collect(r, term_ids, q_off, nq_out); });
}

int vbm25_resolver_in_flight(const vbm25_resolver *r) { return r ? int(r->ring.count) : 0; }

int vbm25_intern_batch_device(int device, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off, uint32_t n_lex, uint8_t *keys16) {
    return guarded([&] { return intern_batch_device(device, seed32, bytes, lex_off, n_lex, keys16); });
}

int vbm25_search_batch_lexemes(vbm25_index *ix, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *q_lex,
                               uint32_t nq, uint32_t k, vbm25_hit *hits, uint32_t *n_hits) {
    return guarded([&] { return search_batch_lexemes(ix, seed32, bytes, lex_off, q_lex, nq, k, hits, n_hits); });
}

// tools/resolve_cost.py: the device time of the last collected batch's kernels (upload excluded), by the slot's HIP events.  Not in the header.
int vbm25_debug_resolver_kernel_ms(vbm25_resolver *r, double *ms) {
    if (!r || !ms || r->last_collected < 0) return set_error(VBM25_ERR_INVALID, "no collected batch");
    const Slot &s = r->slots[r->last_collected];
    HIP_TRY(elapsed_ms(s.start, s.done, ms));
    return VBM25_OK;
}

}  // extern "C"
