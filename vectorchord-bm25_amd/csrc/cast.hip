// cast.hip -- the document cast: cast_tsvector_to_document (src/datatype/tsvector.rs:84-94: intern every lexeme, sort the elements by
// key, sum equal keys saturating -- dedup at :107-127) on the device, batched, the result kept in HBM (vbm25_documents), and the index
// ambuild + io.rs + flush.rs make of such documents (vbm25_device_segment_build_documents).  cast_lane.h holds the per-document
// functions; the kernels here are loops over them.
//
//   per cast, all on a stream of the call's own; no call here is a device-wide synchronisation and no index is touched.  The call
//   does allocate and free its staging and scratch (a pinned block, a dozen device buffers), and the runtime's hipFree / hipHostFree
//   wait for the device's other streams when the cast returns: a cast beside a serving stream stalls it for that moment.
//     upload              the pinned block (doc_lex | lex_off | lex_count | class lists | fieldnorm lengths | bytes) in ONE copy, the
//                         payloads in a second one straight into the handle's array
//     cast_intern_kernel  one lane a lexeme: intern_lane -> key; the chaining-value stack in LDS, sized from the longest lexeme
//     sort and dedup, per DOCUMENT one of three classes (doc_class; the host lists the documents of each while it validates doc_lex):
//       cast_wave_kernel    <= 64 lexemes: one wave a document, one lane a lexeme.  Equal keys in lower lanes and the rank among the
//                           distinct keys by cross-lane compares of the 128-bit key, the heads by ballot, no LDS
//       cast_group_kernel   <= CAST_GROUP_MAX lexemes: one workgroup a document.  Keys and counts sorted in LDS (bitonic; padding sorts
//                           behind every key), then head flags, the runs' saturating sums and the compaction by ballot
//       general             any length: the class's elements, tagged with their document's slot, through three stable radix passes
//                           (key bytes 8..15, key bytes 0..7, slot), head flags, an inclusive scan of the flags (the run numbers) and one
//                           of the counts in 64 bits (a run's sum is a difference of two prefixes, clamped to u32)
//     every class writes a document's survivors at its input offset (tmp_key / tmp_tf) and their number to counts[doc]
//     (scan)              exclusive sum of the counts in 64 bits -> start
//     cast_gather_kernel  one wave a document: tmp -> key / tf at start[doc], the length (saturating) and its fieldnorm code
//   The classes write identical bytes: the order is memcmp's in all three and the saturating sum does not depend on the order.
//   No kernel here has scratch memory.
//
//   the caster (vbm25_caster): the same cast as a ring of slots that keep stream, events, pinned block, scratch and result arrays.  A
//   submit validates, writes the class lists, the general class's offsets and the packing plan straight into the slot's pinned block,
//   copies the caller's arrays behind them and enqueues; nothing is allocated, created or freed, and nothing waits in the middle (key /
//   tf have room for every lexeme, start[n_docs] comes home in pinned memory).  collect waits for the oldest batch's event.
//     cast_pack_kernel    the wave class, several documents a wave (cast_pack 1, 2): one wave a run of the host's plan (<= 64 lexemes,
//                         <= 64 documents), one lane a lexeme, the rank-and-merge confined to the lane's own document, in as many
//                         steps as the run's longest document has lexemes.  <true>: the lanes intern their own lexemes (a batch
//                         without a group- or general-class document, cast_pack 2): no cast_intern_kernel, the keys never reach HBM
//     extend_start_kernel vbm25_documents_extend: src's start rebased behind dst's; the other arrays are device-to-device copies
//
//   the index from documents (document i = doc id i), on the handle's device:
//     (radix sort)        all elements by key, stable: two 64-bit passes with the element index as the value.  Elements are in document
//                         order, so every key's run comes out in ascending document order
//     build_flag_kernel   first of its key -> 1; (scan) inclusive -> rank + 1, the last one = n_terms
//     build_emit_kernel   post_doc (bisection of start), post_tf, term_key and term_start at the heads
//     term_key and term_start go to the host (build_device_core takes them there); the postings never do
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "ring.h"
#include "cast_lane.h"
#include "lexeme_input.h"

namespace {

using namespace vbm25;
using namespace vbm25::rsv;
using namespace vbm25::cst;
using vbm25::lexin::Seed;
using vbm25::lexin::seed_words;
using ull = unsigned long long;

constexpr uint32_t INTERN_THREADS = 64;  // one wave a block: the LDS stack is 32 bytes a level a lane
constexpr uint32_t INTERN_GRID = 1024;   // more lexemes than 65536 stride the grid
constexpr uint32_t WG = 256, MAX_GRID = 2048;

// cast_wave_max / cast_group_max of vbm25_tuning_set: read at the start of each cast
std::atomic<uint32_t> g_wave_max{CAST_WAVE_MAX}, g_group_max{CAST_GROUP_MAX};
// cast_pack / cast_grid: read at each vbm25_caster_submit.  cast_pack: the wave class of a caster's batch through cast_wave_kernel (0),
// cast_pack_kernel on keys from HBM (1), cast_pack_kernel interning in its lanes where the batch has no other class (2).  cast_grid: the most
// workgroups of a caster's kernels (0: no cap of its own).
constexpr uint32_t CAST_PACK_DEFAULT = 2;
std::atomic<uint32_t> g_cast_pack{CAST_PACK_DEFAULT}, g_cast_grid{0};
// the calling thread's last cast: its kernels by HIP events -- upload excluded, and so is the host's allocation of key / tf between
// the scan and the gather (two spans: upload's end .. the scan's end, the gather's start .. its end)
thread_local double g_kernel_ms = -1.0;

// The pool is 4-byte aligned and ends on a multiple of 4 (WordLoad).
__global__ void __launch_bounds__(INTERN_THREADS) cast_intern_kernel(Seed seed, const uint32_t *pool, const uint64_t *lex_off, uint32_t n_lex,
                                                                     Key *keys) {
    extern __shared__ uint32_t cv_stack[];
    const WordLoad ld{pool};
    for (uint32_t i = blockIdx.x * INTERN_THREADS + threadIdx.x; i < n_lex; i += gridDim.x * INTERN_THREADS) {
        const uint64_t begin = lex_off[i];
        keys[i] = intern_lane(seed.w, ld, begin, lex_off[i + 1] - begin, cv_stack + threadIdx.x, INTERN_THREADS);
    }
}

// what a sort kernel reads and writes: document d = lexemes doc_lex[d] .. doc_lex[d + 1]; its survivors go to tmp_*[doc_lex[d] ..)
struct SortArgs {
    const Key *keys;
    const uint32_t *lex_count, *doc_lex;
    Key *tmp_key;
    uint32_t *tmp_tf, *counts;
};

// element j of the wave's document: lane j's registers (every lane of the wave calls, cast_wave_kernel's with the same j)
struct LaneAt {
    Key k;
    uint32_t c;
    __device__ void operator()(uint32_t j, Key &kj, uint32_t &cj) const {
        kj.x = __shfl(ull(k.x), int(j));
        kj.y = __shfl(ull(k.y), int(j));
        cj = __shfl(c, int(j));
    }
};
struct MaskHead {
    ull mask;
    __device__ bool operator()(uint32_t j) const { return (mask >> j) & 1ull; }
};

// the wave class: every listed document has at most 64 lexemes
__global__ void __launch_bounds__(WG) cast_wave_kernel(SortArgs a, const uint32_t *list, uint32_t n_list) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG + threadIdx.x) >> 6, n_waves = (gridDim.x * WG) >> 6;
    for (uint32_t s = wave; s < n_list; s += n_waves) {
        const uint32_t d = list[s], b = a.doc_lex[d], n = a.doc_lex[d + 1] - b;
        const bool mine = lane < n;
        const LaneAt at{mine ? a.keys[b + lane] : Key{0, 0}, mine ? a.lex_count[b + lane] : 0u};
        uint32_t sum;
        const bool head = head_and_sum(at, n, lane, at.k, sum) && mine;
        const ull heads = __ballot(head);
        const uint32_t rank = rank_of(at, MaskHead{heads}, n, at.k);
        if (head) {
            a.tmp_key[b + rank] = at.k;
            a.tmp_tf[b + rank] = sum;
        }
        if (lane == 0) a.counts[d] = __popcll(heads);
    }
}

// the wave class, several documents a wave: entry s of the host's plan is a run of consecutive documents with at most 64 lexemes
// between them, one lane a lexeme.  A lane finds its document among the run's bounds of doc_lex; the rank-and-merge runs in the whole
// wave at once, every lane against the elements of its own document only (cast_lane.h), in as many steps as the run's longest document
// has lexemes.  FUSED: the lanes intern their own lexemes -- the batch
// has no document of another class, nobody else needs the keys, they never reach HBM -- with the chaining-value stack in LDS, one
// column a thread of the block (cast_intern_kernel's).  Otherwise a.keys is read.
struct BoundAt {
    uint32_t bound;  // lane j: where document j of the run begins, as a lane
    __device__ uint32_t operator()(uint32_t j) const { return __shfl(bound, int(j)); }
};
template <bool FUSED>
__global__ void __launch_bounds__(WG) cast_pack_kernel(SortArgs a, const PackEntry *plan, uint32_t n_plan, Seed seed, const uint32_t *pool,
                                                       const uint64_t *lex_off) {
    extern __shared__ uint32_t cv_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t s = wave; s < n_plan; s += n_waves) {
        const PackEntry e = plan[s];
        const uint32_t b = a.doc_lex[e.first], n = a.doc_lex[e.first + e.count] - b;  // n <= 64, e.count in 1 .. 64
        const BoundAt bound{lane < e.count ? a.doc_lex[e.first + lane] - b : n};
        const uint32_t doc = lane_document(bound, e.count, lane);  // (of the run; lanes at and beyond n get one they do not use)
        const uint32_t next = bound((lane + 1u) & 63u);
        const uint32_t sb = bound(doc), se_in = bound((doc + 1u) & 63u), se = doc + 1u < e.count ? se_in : n;
        uint32_t longest = lane < e.count ? (lane + 1u < e.count ? next : n) - bound.bound : 0u;  // lane j < count: document j's lexemes
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) longest = max(longest, uint32_t(__shfl_xor(longest, x)));
        const bool mine = lane < n;
        Key k{0, 0};
        if (mine) {
            if constexpr (FUSED) {
                const uint64_t begin = lex_off[b + lane];
                k = intern_lane(seed.w, WordLoad{pool}, begin, lex_off[b + lane + 1] - begin, cv_stack + threadIdx.x, blockDim.x);
            } else {
                k = a.keys[b + lane];
            }
        }
        const LaneAt at{k, mine ? a.lex_count[b + lane] : 0u};
        uint32_t sum;
        const bool head = seg_head_and_sum(at, longest, lane, at.k, sb, se, sum) && mine;
        const ull heads = __ballot(head);
        const uint32_t rank = seg_rank_of(at, MaskHead{heads}, longest, lane, at.k, sb, se);
        if (head) {
            a.tmp_key[b + sb + rank] = at.k;
            a.tmp_tf[b + sb + rank] = sum;
        }
        // lane j < count: document j of the run is lanes bound .. next (the last one ends at n)
        if (lane < e.count) a.counts[e.first + lane] = __popcll(heads & lane_span(bound.bound, lane + 1u < e.count ? next : n));
    }
}

// order of two LDS elements of the workgroup class: a count of 0 marks padding (a lexeme's count is never 0), which sorts last
__device__ __forceinline__ bool slot_less(const Key &ka, uint32_t ca, const Key &kb, uint32_t cb) {
    if ((ca == 0) != (cb == 0)) return cb == 0;
    return ca != 0 && key_less(ka, kb);
}

// the workgroup class: every listed document has at most CAST_GROUP_MAX lexemes
__global__ void __launch_bounds__(WG) cast_group_kernel(SortArgs a, const uint32_t *list, uint32_t n_list) {
    __shared__ Key s_key[CAST_GROUP_MAX];
    __shared__ uint32_t s_tf[CAST_GROUP_MAX];
    __shared__ uint32_t s_wave[WG / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    for (uint32_t s = blockIdx.x; s < n_list; s += gridDim.x) {
        const uint32_t d = list[s], b = a.doc_lex[d], n = a.doc_lex[d + 1] - b;
        uint32_t P = 1;
        while (P < n) P <<= 1;
        for (uint32_t i = t; i < P; i += WG) {
            s_key[i] = i < n ? a.keys[b + i] : Key{0, 0};
            s_tf[i] = i < n ? a.lex_count[b + i] : 0u;
        }
        __syncthreads();
        for (uint32_t k = 2; k <= P; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = t; i < P; i += WG) {
                    const uint32_t o = i ^ j;
                    if (o > i) {
                        const Key ki = s_key[i], ko = s_key[o];
                        const uint32_t ci = s_tf[i], co = s_tf[o];
                        const bool up = (i & k) == 0;
                        if (up ? slot_less(ko, co, ki, ci) : slot_less(ki, ci, ko, co)) {
                            s_key[i] = ko;
                            s_key[o] = ki;
                            s_tf[i] = co;
                            s_tf[o] = ci;
                        }
                    }
                }
                __syncthreads();
            }
        }
        // heads, their runs' sums and their positions among the heads
        uint32_t base = 0;
        for (uint32_t r = 0; r < n; r += WG) {
            const uint32_t i = r + t;
            const bool head = i < n && (i == 0 || !key_equal(s_key[i], s_key[i - 1]));
            const ull heads = __ballot(head);
            if (lane == 0) s_wave[w] = __popcll(heads);
            __syncthreads();
            uint32_t at = base, total = 0;
#pragma unroll
            for (uint32_t x = 0; x < WG / 64; ++x) {
                const uint32_t v = s_wave[x];
                at += x < w ? v : 0u;
                total += v;
            }
            if (head) {
                const Key k = s_key[i];
                uint32_t sum = s_tf[i];
                for (uint32_t e = i + 1; e < n && key_equal(s_key[e], k); ++e) sum = sat_add(sum, s_tf[e]);
                at += __popcll(heads & ((1ull << lane) - 1ull));
                a.tmp_key[b + at] = k;
                a.tmp_tf[b + at] = sum;
            }
            base += total;
            __syncthreads();
        }
        if (t == 0) a.counts[d] = base;
    }
}

// ---- the general class.  Slot s of the class is document list[s], its elements are e = off[s] .. off[s + 1] of the class ----
struct GenArgs {
    SortArgs a;
    const uint32_t *list, *off;  // n_gen documents, n_gen + 1 offsets
    uint32_t n_gen, n_el;
    uint32_t *src, *slot;        // per element: its lexeme, its slot (slot: the run numbers once the sorts are done)
    ull *ka, *kb;                // the sort's keys (ka: the counts in 64 bits once the sorts are done; kb: the slot per sorted position)
    uint32_t *va, *vb;           // the sort's values: element numbers (va: the head flags once the sorts are done)
    ull *prefix;                 // inclusive sums of the counts in sorted order
    uint32_t *head_pos;          // n_el + 1: run q starts at sorted position head_pos[q]
};

__global__ void __launch_bounds__(WG) gen_fill_kernel(GenArgs g) {
    for (uint32_t e = blockIdx.x * WG + threadIdx.x; e < g.n_el; e += gridDim.x * WG) {
        uint32_t lo = 0, hi = g.n_gen;  // the last slot with off[slot] <= e (empty documents in front of it share its start)
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (g.off[mid] <= e) lo = mid; else hi = mid;
        }
        const uint32_t src = g.a.doc_lex[g.list[lo]] + (e - g.off[lo]);
        g.src[e] = src;
        g.slot[e] = lo;
        g.ka[e] = __builtin_bswap64(g.a.keys[src].y);
        g.va[e] = e;
    }
}
__global__ void __launch_bounds__(WG) gen_key_high_kernel(GenArgs g) {  // after pass 1: (kb, vb)
    for (uint32_t p = blockIdx.x * WG + threadIdx.x; p < g.n_el; p += gridDim.x * WG) g.ka[p] = __builtin_bswap64(g.a.keys[g.src[g.vb[p]]].x);
}
__global__ void __launch_bounds__(WG) gen_key_slot_kernel(GenArgs g) {  // after pass 2: (kb, va)
    for (uint32_t p = blockIdx.x * WG + threadIdx.x; p < g.n_el; p += gridDim.x * WG) g.ka[p] = g.slot[g.va[p]];
}
// after pass 3: (kb = slot, vb = element) by (slot, key).  flags -> va, counts in 64 bits -> ka
__global__ void __launch_bounds__(WG) gen_flag_kernel(GenArgs g) {
    for (uint32_t p = blockIdx.x * WG + threadIdx.x; p < g.n_el; p += gridDim.x * WG) {
        const uint32_t src = g.src[g.vb[p]];
        const bool head = p == g.off[uint32_t(g.kb[p])] || !key_equal(g.a.keys[src], g.a.keys[g.src[g.vb[p - 1]]]);
        g.va[p] = head ? 1u : 0u;
        g.ka[p] = g.a.lex_count[src];
    }
}
// run numbers (inclusive sums of the flags) -> slot
__global__ void __launch_bounds__(WG) gen_head_pos_kernel(GenArgs g) {
    const uint32_t *run = g.slot;
    for (uint32_t p = blockIdx.x * WG + threadIdx.x; p < g.n_el; p += gridDim.x * WG) {
        if (g.va[p]) g.head_pos[run[p] - 1] = p;
        if (p == g.n_el - 1) g.head_pos[run[p]] = g.n_el;
    }
}
__global__ void __launch_bounds__(WG) gen_emit_kernel(GenArgs g) {
    const uint32_t *run = g.slot;
    for (uint32_t p = blockIdx.x * WG + threadIdx.x; p < g.n_el; p += gridDim.x * WG) {
        const uint32_t s = uint32_t(g.kb[p]), first = g.off[s], d = g.list[s], in_doc = run[p] - run[first];
        if (g.va[p]) {
            const uint32_t end = g.head_pos[run[p]];
            const ull sum = g.prefix[end - 1] - (p ? g.prefix[p - 1] : 0ull);
            const uint32_t out = g.a.doc_lex[d] + in_doc;
            g.a.tmp_key[out] = g.a.keys[g.src[g.vb[p]]];
            g.a.tmp_tf[out] = clamp_u32(sum);
        }
        if (p == g.off[s + 1] - 1) g.a.counts[d] = in_doc + 1;
    }
}

// one wave a document: the survivors to their place, the length and the fieldnorm code
__global__ void __launch_bounds__(WG) cast_gather_kernel(const Key *tmp_key, const uint32_t *tmp_tf, const uint32_t *doc_lex, const ull *start,
                                                         uint32_t n_docs, const uint32_t *fn_len, Key *key, uint32_t *tf, uint32_t *length,
                                                         uint8_t *fieldnorm) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG + threadIdx.x) >> 6, n_waves = (gridDim.x * WG) >> 6;
    for (uint32_t d = wave; d < n_docs; d += n_waves) {
        const ull o = start[d];
        const uint32_t c = uint32_t(start[d + 1] - o), b = doc_lex[d];
        uint32_t len = 0;
        for (uint32_t j = lane; j < c; j += 64) {
            const uint32_t v = tmp_tf[b + j];
            key[o + j] = tmp_key[b + j];
            tf[o + j] = v;
            len = sat_add(len, v);
        }
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) len = sat_add(len, __shfl_xor(len, x));
        if (lane == 0) {
            length[d] = len;
            fieldnorm[d] = fieldnorm_of(fn_len, len);
        }
    }
}

// ---- the index from documents ----
__global__ void __launch_bounds__(WG) build_key_kernel(const Key *key, const uint32_t *idx, uint32_t n, int high, ull *out, uint32_t *iota) {
    for (uint32_t p = blockIdx.x * WG + threadIdx.x; p < n; p += gridDim.x * WG) {
        const Key k = key[idx ? idx[p] : p];
        out[p] = __builtin_bswap64(high ? k.x : k.y);
        if (iota) iota[p] = p;
    }
}
__global__ void __launch_bounds__(WG) build_flag_kernel(const Key *key, const uint32_t *order, uint32_t n, uint32_t *flags) {
    for (uint32_t p = blockIdx.x * WG + threadIdx.x; p < n; p += gridDim.x * WG)
        flags[p] = (p == 0 || !key_equal(key[order[p]], key[order[p - 1]])) ? 1u : 0u;
}
__global__ void __launch_bounds__(WG) build_emit_kernel(const Key *key, const uint32_t *tf, const ull *start, uint32_t n_docs, const uint32_t *order,
                                                        const uint32_t *flags, const uint32_t *rank1, uint32_t n, uint32_t *post_doc,
                                                        uint32_t *post_tf, Key *term_key, ull *term_start) {
    for (uint32_t p = blockIdx.x * WG + threadIdx.x; p < n; p += gridDim.x * WG) {
        const uint32_t e = order[p];
        uint32_t lo = 0, hi = n_docs;  // the last document with start[doc] <= e (empty documents in front of it share its start)
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (start[mid] <= e) lo = mid; else hi = mid;
        }
        post_doc[p] = lo;
        post_tf[p] = tf[e];
        if (flags[p]) {
            term_key[rank1[p] - 1] = key[e];
            term_start[rank1[p] - 1] = p;
        }
        if (p == n - 1) term_start[rank1[p]] = n;
    }
}

// the device of a cast: checked to be there, then made the calling thread's
int use_cast_device(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: the document cast has no host fallback");
    if (device < 0 || device >= n_dev) return set_error(VBM25_ERR_INVALID, "device %d out of range (%d devices)", device, n_dev);
    return use_device(device);
}

// what a batch of documents is, checked before anything is allocated or enqueued
struct Shape {
    uint32_t n_lex = 0;
    uint64_t n_bytes = 0, longest_lexeme = 0;
};
int check_documents(bool has_seed, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *lex_count, const uint32_t *doc_lex, uint32_t n_docs,
                    Shape *s) {
    if (!doc_lex || !lex_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_docs >= (1u << 31) - 1u) return set_error(VBM25_ERR_UNSUPPORTED, "%u documents: one cast takes fewer than 2^31 - 1", n_docs);
    if (doc_lex[0] != 0) return set_error(VBM25_ERR_INVALID, "doc_lex[0] is %u, not 0", doc_lex[0]);
    for (uint32_t i = 0; i < n_docs; ++i)
        if (doc_lex[i + 1] < doc_lex[i]) return set_error(VBM25_ERR_INVALID, "doc_lex is not monotone at document %u", i);
    s->n_lex = doc_lex[n_docs];
    if (s->n_lex >= (1u << 31)) return set_error(VBM25_ERR_UNSUPPORTED, "%u lexemes: one cast takes fewer than 2^31", s->n_lex);
    if (s->n_lex && !lex_count) return set_error(VBM25_ERR_INVALID, "NULL argument");
    // (the offsets and the pool first, as they were; the seed last, behind the counts)
    if (int rc = lexin::check_pool(true, bytes, lex_off, s->n_lex, "cast", &s->n_bytes, &s->longest_lexeme)) return rc;
    for (uint32_t d = 0; d < n_docs; ++d)  // (the reference panics on a lexeme without positions)
        for (uint32_t i = doc_lex[d]; i < doc_lex[d + 1]; ++i)
            if (lex_count[i] == 0) return set_error(VBM25_ERR_INVALID, "lexeme %u (document %u) has count 0", i, d);
    return has_seed ? VBM25_OK : lexin::check_pool(false, bytes, lex_off, s->n_lex, "cast", &s->n_bytes, &s->longest_lexeme);
}

// the most temporary storage hipcub asks for in one cast: the scan of n_docs + 1 counts and, with n_gen_el elements in the general
// class, its sorts and scans
int cast_cub_bytes(uint32_t n_docs, uint32_t n_gen_el, hipStream_t st, size_t *out) {
    size_t cub_bytes = 0, tb = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(nullptr, WidenU32()),
                                            (ull *)nullptr, int(n_docs + 1), st));
    cub_bytes = std::max(cub_bytes, tb);
    if (n_gen_el) {
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const ull *)nullptr, (ull *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                  int(n_gen_el), 0, 64, st));
        cub_bytes = std::max(cub_bytes, tb);
        HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb, (const uint32_t *)nullptr, (uint32_t *)nullptr, int(n_gen_el), st));
        cub_bytes = std::max(cub_bytes, tb);
        HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb, (const ull *)nullptr, (ull *)nullptr, int(n_gen_el), st));
        cub_bytes = std::max(cub_bytes, tb);
    }
    *out = cub_bytes;
    return VBM25_OK;
}

// the general class of one cast, enqueued: g.n_el > 0 elements, `grid` workgroups for its own kernels
int enqueue_general(hipStream_t st, const GenArgs &g, void *cub, size_t cub_bytes, uint32_t grid) {
    const uint32_t n_gen = g.n_gen, n_gen_el = g.n_el;
    int slot_bits = 1;
    while (slot_bits < 32 && (uint64_t(n_gen - 1) >> slot_bits)) ++slot_bits;
    size_t tb = cub_bytes;
    gen_fill_kernel<<<grid, WG, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub, tb, g.ka, g.kb, g.va, g.vb, int(n_gen_el), 0, 64, st));
    gen_key_high_kernel<<<grid, WG, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    tb = cub_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub, tb, g.ka, g.kb, g.vb, g.va, int(n_gen_el), 0, 64, st));
    gen_key_slot_kernel<<<grid, WG, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    tb = cub_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub, tb, g.ka, g.kb, g.va, g.vb, int(n_gen_el), 0, slot_bits, st));
    gen_flag_kernel<<<grid, WG, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    tb = cub_bytes;
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(cub, tb, g.va, g.slot, int(n_gen_el), st));
    tb = cub_bytes;
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(cub, tb, g.ka, g.prefix, int(n_gen_el), st));
    gen_head_pos_kernel<<<grid, WG, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    gen_emit_kernel<<<grid, WG, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    return VBM25_OK;
}

uint64_t handle_bytes(const vbm25_documents *h) {
    uint64_t n = 0;
    for (const HbmArray *a : {&h->d_start, &h->d_key, &h->d_tf, &h->d_length, &h->d_fieldnorm, &h->d_payload}) n += a->bytes;
    return n;
}

int documents_cast(int device, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *lex_count,
                   const uint32_t *doc_lex, uint32_t n_docs, const uint16_t *doc_payload, vbm25_documents **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    const uint32_t wave_max = g_wave_max.load(), group_max = g_group_max.load();
    Shape sh;
    if (int rc = check_documents(seed32 != nullptr, bytes, lex_off, lex_count, doc_lex, n_docs, &sh)) return rc;
    // the documents of each class, and the general class's element offsets
    std::vector<uint32_t> lists[3], gen_off{0};
    for (uint32_t d = 0; d < n_docs; ++d) {
        const uint32_t n = doc_lex[d + 1] - doc_lex[d];
        const DocClass c = doc_class(n, wave_max, group_max);
        lists[c].push_back(d);
        if (c == CLASS_GENERAL) gen_off.push_back(gen_off.back() + n);
    }
    const uint32_t n_lex = sh.n_lex, n_wave = uint32_t(lists[0].size()), n_group = uint32_t(lists[1].size()), n_gen = uint32_t(lists[2].size()),
                   n_gen_el = gen_off.back();
    if (int rc = use_cast_device(device)) return rc;
    g_kernel_ms = -1.0;

    auto h = std::make_unique<vbm25_documents>();
    h->device = device;
    h->n_docs = n_docs;
    h->has_payload = doc_payload != nullptr;
    Seed seed;
    seed_words(seed32, &seed);
    // the staged block
    size_t total = 0;
    auto take = [&](size_t n) {
        const size_t at = total;
        total = align_up(total + n, 16);
        return at;
    };
    const size_t o_doc = take(4ull * (n_docs + 1ull)), o_off = take(8ull * (n_lex + 1ull)), o_cnt = take(4ull * n_lex), o_list = take(4ull * n_docs),
                 o_goff = take(4ull * (n_gen + 1ull)), o_fn = take(4 * 256), o_pay = take(doc_payload ? 6ull * n_docs : 0), o_bytes = take(sh.n_bytes);
    PinnedHost stage;
    HbmArray in, keys, tmp_key, tmp_tf, counts, cub, g_src, g_slot, g_ka, g_kb, g_va, g_vb, g_prefix, g_head_pos;
    // a stream of the call's own (a launch on the null stream would wait for every other stream of the device), declared behind the
    // buffers and waited for by `quiesce` behind it: the stream is idle before it is destroyed, and both before anything is freed
    Event ev_start, ev_mid, ev_resume, ev_done;
    Stream st;
    HIP_TRY(st.create());
    Quiesce quiesce(st.s);
    HIP_TRY(ev_start.create());
    HIP_TRY(ev_done.create());
    HIP_TRY(ev_mid.create());
    HIP_TRY(ev_resume.create());
    HIP_TRY(stage.alloc(total));
    uint8_t *const staged = stage.as<uint8_t>();
    std::memcpy(staged + o_doc, doc_lex, 4ull * (n_docs + 1ull));
    std::memcpy(staged + o_off, lex_off, 8ull * (n_lex + 1ull));
    if (n_lex) std::memcpy(staged + o_cnt, lex_count, 4ull * n_lex);
    {
        size_t at = o_list;
        for (const auto &l : lists) {
            if (!l.empty()) std::memcpy(staged + at, l.data(), 4ull * l.size());
            at += 4ull * l.size();
        }
    }
    std::memcpy(staged + o_goff, gen_off.data(), 4ull * gen_off.size());
    std::memcpy(staged + o_fn, fieldnorm_lengths(), 4 * 256);
    if (doc_payload && n_docs) std::memcpy(staged + o_pay, doc_payload, 6ull * n_docs);
    if (sh.n_bytes) std::memcpy(staged + o_bytes, bytes, sh.n_bytes);
    if (total > o_bytes + sh.n_bytes) std::memset(staged + o_bytes + sh.n_bytes, 0, total - o_bytes - sh.n_bytes);

    size_t cub_bytes = 0, tb = 0;
    if (int rc = cast_cub_bytes(n_docs, n_gen_el, st.s, &cub_bytes)) return rc;
    HIP_TRY(in.alloc(total));
    HIP_TRY(keys.alloc(16ull * n_lex));
    HIP_TRY(tmp_key.alloc(16ull * n_lex));
    HIP_TRY(tmp_tf.alloc(4ull * n_lex));
    HIP_TRY(counts.alloc(4ull * (n_docs + 1ull)));
    HIP_TRY(cub.alloc(cub_bytes));
    HIP_TRY(h->d_start.alloc(8ull * (n_docs + 1ull)));
    HIP_TRY(h->d_length.alloc(4ull * n_docs));
    HIP_TRY(h->d_fieldnorm.alloc(n_docs));
    if (doc_payload) HIP_TRY(h->d_payload.alloc(6ull * n_docs));
    if (n_gen_el) {
        HIP_TRY(g_src.alloc(4ull * n_gen_el));
        HIP_TRY(g_slot.alloc(4ull * n_gen_el));
        HIP_TRY(g_ka.alloc(8ull * n_gen_el));
        HIP_TRY(g_kb.alloc(8ull * n_gen_el));
        HIP_TRY(g_va.alloc(4ull * n_gen_el));
        HIP_TRY(g_vb.alloc(4ull * n_gen_el));
        HIP_TRY(g_prefix.alloc(8ull * n_gen_el));
        HIP_TRY(g_head_pos.alloc(4ull * (n_gen_el + 1ull)));
    }
    uint8_t *d = in.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(d, stage.p, total, hipMemcpyHostToDevice, st.s));
    if (doc_payload && n_docs) HIP_TRY(hipMemcpyAsync(h->d_payload.p, staged + o_pay, 6ull * n_docs, hipMemcpyHostToDevice, st.s));
    HIP_TRY(hipEventRecord(ev_start.e, st.s));
    HIP_TRY(hipMemsetAsync(counts.p, 0, 4ull * (n_docs + 1ull), st.s));
    const uint32_t *d_doc = reinterpret_cast<const uint32_t *>(d + o_doc), *d_cnt = reinterpret_cast<const uint32_t *>(d + o_cnt),
                   *d_list = reinterpret_cast<const uint32_t *>(d + o_list), *d_goff = reinterpret_cast<const uint32_t *>(d + o_goff),
                   *d_fn = reinterpret_cast<const uint32_t *>(d + o_fn);
    const SortArgs sa{keys.as<Key>(), d_cnt, d_doc, tmp_key.as<Key>(), tmp_tf.as<uint32_t>(), counts.as<uint32_t>()};
    if (n_lex) {
        const size_t lds = size_t(stack_levels(sh.longest_lexeme)) * 8 * sizeof(uint32_t) * INTERN_THREADS;
        cast_intern_kernel<<<std::min(INTERN_GRID, grid_for(n_lex, INTERN_THREADS, MAX_GRID)), INTERN_THREADS, lds, st.s>>>(
            seed, reinterpret_cast<const uint32_t *>(d + o_bytes), reinterpret_cast<const uint64_t *>(d + o_off), n_lex, keys.as<Key>());
        HIP_TRY(hipGetLastError());
    }
    if (n_wave && n_lex) {
        cast_wave_kernel<<<grid_for(n_wave, WG / 64, MAX_GRID), WG, 0, st.s>>>(sa, d_list, n_wave);
        HIP_TRY(hipGetLastError());
    }
    if (n_group && n_lex) {
        cast_group_kernel<<<grid_for(n_group, 1, MAX_GRID), WG, 0, st.s>>>(sa, d_list + n_wave, n_group);
        HIP_TRY(hipGetLastError());
    }
    if (n_gen_el) {
        const GenArgs g{sa, d_list + n_wave + n_group, d_goff, n_gen, n_gen_el, g_src.as<uint32_t>(), g_slot.as<uint32_t>(), g_ka.as<ull>(), g_kb.as<ull>(),
                        g_va.as<uint32_t>(), g_vb.as<uint32_t>(), g_prefix.as<ull>(), g_head_pos.as<uint32_t>()};
        if (int rc = enqueue_general(st.s, g, cub.p, cub_bytes, grid_for(n_gen_el, WG, MAX_GRID))) return rc;
    }
    tb = cub_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub.p, tb, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(counts.as<uint32_t>(), WidenU32()),
                                            h->d_start.as<ull>(), int(n_docs + 1), st.s));
    HIP_TRY(hipEventRecord(ev_mid.e, st.s));
    ull n_elements = 0;
    HIP_TRY(hipMemcpyAsync(&n_elements, h->d_start.as<ull>() + n_docs, 8, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    h->n_elements = n_elements;
    HIP_TRY(h->d_key.alloc(16ull * n_elements));
    HIP_TRY(h->d_tf.alloc(4ull * n_elements));
    HIP_TRY(hipEventRecord(ev_resume.e, st.s));
    if (n_docs) {
        cast_gather_kernel<<<grid_for(n_docs, WG / 64, MAX_GRID), WG, 0, st.s>>>(tmp_key.as<Key>(), tmp_tf.as<uint32_t>(), d_doc, h->d_start.as<ull>(), n_docs, d_fn,
                                                                       h->d_key.as<Key>(), h->d_tf.as<uint32_t>(), h->d_length.as<uint32_t>(),
                                                                       h->d_fieldnorm.as<uint8_t>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev_done.e, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    float ms = 0, ms2 = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev_start.e, ev_mid.e));
    HIP_TRY(hipEventElapsedTime(&ms2, ev_resume.e, ev_done.e));
    g_kernel_ms = double(ms) + ms2;
    *out = h.release();
    return VBM25_OK;
}

int documents_download(const vbm25_documents *h, vbm25_growing **csr, uint32_t *doc_len) {
    if (!csr) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *csr = nullptr;
    if (!h) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (int rc = use_cast_device(h->device)) return rc;
    auto g = std::make_unique<vbm25_growing>();
    const size_t n = h->n_docs, e = h->n_elements;
    g->start.assign(n + 1, 0);
    g->key.resize(16 * e);
    g->tf.resize(e);
    g->fieldnorm.resize(n);
    g->deleted.assign(n, 0);
    HIP_TRY(hipMemcpy(g->start.data(), h->d_start.p, 8 * (n + 1), hipMemcpyDeviceToHost));
    if (e) {
        HIP_TRY(hipMemcpy(g->key.data(), h->d_key.p, 16 * e, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(g->tf.data(), h->d_tf.p, 4 * e, hipMemcpyDeviceToHost));
    }
    if (n) {
        HIP_TRY(hipMemcpy(g->fieldnorm.data(), h->d_fieldnorm.p, n, hipMemcpyDeviceToHost));
        if (h->has_payload) {
            g->payload.resize(3 * n);
            HIP_TRY(hipMemcpy(g->payload.data(), h->d_payload.p, 6 * n, hipMemcpyDeviceToHost));
        }
        if (doc_len) HIP_TRY(hipMemcpy(doc_len, h->d_length.p, 4 * n, hipMemcpyDeviceToHost));
    }
    *csr = g.release();
    return VBM25_OK;
}

int build_documents(const vbm25_documents *h, double k1, double b, vbm25_device_segment **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: the device builder has no CPU fallback (vbm25_segment_build is the host builder)");
    if (!h) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (!h->has_payload) return set_error(VBM25_ERR_INVALID, "the documents were cast without payloads: an index needs them");
    if (!h->n_docs) return set_error(VBM25_ERR_INVALID, "segment without documents");
    if (int rc = use_cast_device(h->device)) return rc;
    const uint32_t n = uint32_t(h->n_elements);  // (fewer than 2^31: a cast takes fewer lexemes than that)
    uint32_t n_terms = 0;
    std::vector<uint8_t> term_key;
    std::vector<uint64_t> term_start{0};
    HbmArray ka, kb, va, vb, flags, rank1, cub, post_doc, post_tf, d_tkey, d_tstart;
    Stream st;  // (of the call's own, as the cast's)
    Quiesce quiesce;
    if (n) {
        HIP_TRY(st.create());
        quiesce.s = st.s;
        size_t sort_b = 0, scan_b = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (const ull *)nullptr, (ull *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, int(n),
                                                  0, 64, st.s));
        HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_b, (const uint32_t *)nullptr, (uint32_t *)nullptr, int(n), st.s));
        const size_t cub_bytes = std::max(sort_b, scan_b);
        HIP_TRY(ka.alloc(8ull * n));
        HIP_TRY(kb.alloc(8ull * n));
        HIP_TRY(va.alloc(4ull * n));
        HIP_TRY(vb.alloc(4ull * n));
        HIP_TRY(flags.alloc(4ull * n));
        HIP_TRY(rank1.alloc(4ull * n));
        HIP_TRY(cub.alloc(cub_bytes));
        HIP_TRY(post_doc.alloc(4ull * n));
        HIP_TRY(post_tf.alloc(4ull * n));
        const Key *key = h->d_key.as<Key>();
        const uint32_t grid = grid_for(n, WG, MAX_GRID);
        build_key_kernel<<<grid, WG, 0, st.s>>>(key, nullptr, n, 0, ka.as<ull>(), va.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        size_t tb = cub_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub.p, tb, ka.as<ull>(), kb.as<ull>(), va.as<uint32_t>(), vb.as<uint32_t>(), int(n), 0, 64, st.s));
        build_key_kernel<<<grid, WG, 0, st.s>>>(key, vb.as<uint32_t>(), n, 1, ka.as<ull>(), nullptr);
        HIP_TRY(hipGetLastError());
        tb = cub_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub.p, tb, ka.as<ull>(), kb.as<ull>(), vb.as<uint32_t>(), va.as<uint32_t>(), int(n), 0, 64, st.s));
        build_flag_kernel<<<grid, WG, 0, st.s>>>(key, va.as<uint32_t>(), n, flags.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        tb = cub_bytes;
        HIP_TRY(hipcub::DeviceScan::InclusiveSum(cub.p, tb, flags.as<uint32_t>(), rank1.as<uint32_t>(), int(n), st.s));
        HIP_TRY(hipMemcpyAsync(&n_terms, rank1.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, st.s));
        HIP_TRY(hipStreamSynchronize(st.s));
        HIP_TRY(d_tkey.alloc(16ull * n_terms));
        HIP_TRY(d_tstart.alloc(8ull * (n_terms + 1ull)));
        build_emit_kernel<<<grid, WG, 0, st.s>>>(key, h->d_tf.as<uint32_t>(), h->d_start.as<ull>(), h->n_docs, va.as<uint32_t>(), flags.as<uint32_t>(),
                                                 rank1.as<uint32_t>(), n, post_doc.as<uint32_t>(), post_tf.as<uint32_t>(), d_tkey.as<Key>(),
                                                 d_tstart.as<ull>());
        HIP_TRY(hipGetLastError());
        term_key.resize(16ull * n_terms);
        term_start.resize(n_terms + 1ull);
        HIP_TRY(hipMemcpyAsync(term_key.data(), d_tkey.p, 16ull * n_terms, hipMemcpyDeviceToHost, st.s));
        HIP_TRY(hipMemcpyAsync(term_start.data(), d_tstart.p, 8ull * (n_terms + 1ull), hipMemcpyDeviceToHost, st.s));
        HIP_TRY(hipStreamSynchronize(st.s));
    }
    std::unique_ptr<vbm25_device_segment> ds;
    if (int rc = build_device_core(h->device, k1, b, h->n_docs, nullptr, h->d_length.as<uint32_t>(), nullptr, h->d_payload.as<uint16_t>(), n_terms,
                                   term_key.data(), term_start.data(), nullptr, nullptr, post_doc.as<uint32_t>(), post_tf.as<uint32_t>(), ds))
        return rc;
    *out = ds.release();
    return VBM25_OK;
}


// ---- the caster: a ring of slots that keep everything a cast needs ----
// what one batch's staged block holds and where (every part on a multiple of 16 bytes).  The one layout serves a batch (its own
// numbers) and the slot's capacity (the caster's maxima): every offset and the total grow with every number.
struct StageLayout {
    size_t o_doc, o_off, o_cnt, o_list, o_goff, o_fn, o_pay, o_plan, o_bytes, total;
    StageLayout(uint64_t n_docs, uint64_t n_lex, uint64_t n_gen, uint64_t n_plan, uint64_t n_bytes) {
        size_t at = 0;
        auto take = [&](size_t n) {
            const size_t o = at;
            at = align_up(at + n, 16);
            return o;
        };
        o_doc = take(4 * (n_docs + 1));
        o_off = take(8 * (n_lex + 1));
        o_cnt = take(4 * n_lex);
        o_list = take(4 * n_docs);
        o_goff = take(4 * (n_gen + 1));
        o_fn = take(4 * 256);
        o_pay = take(6 * n_docs);
        o_plan = take(sizeof(PackEntry) * n_plan);
        o_bytes = take(n_bytes);
        total = at;
    }
};

struct CastSlot {
    Stream stream;
    Event start, done;
    PinnedHost stage;            // the staged block of one batch
    PinnedHost n_elements;       // one ull: start[n_docs], copied back behind the scan
    HbmArray in, keys, tmp_key, tmp_tf, counts, cub, g_src, g_slot, g_ka, g_kb, g_va, g_vb, g_prefix, g_head_pos;
    vbm25_documents docs;        // the result arrays, at the caster's capacities; what collect hands out
    uint32_t launched = 0;       // LAUNCHED_* of the slot's last batch
};

// the kernels a batch's lexemes and wave class went through, as vbm25_debug_caster_launched reports them
enum : uint32_t { LAUNCHED_INTERN = 1, LAUNCHED_WAVE = 2, LAUNCHED_PACK = 4, LAUNCHED_PACK_FUSED = 8 };

}  // namespace

// vbm25_caster_free waits for every slot's stream before it deletes: the order of the members below does not matter to their destructors.
struct vbm25_caster {
    int device = 0;
    uint32_t max_docs = 0, max_lexemes = 0, max_long = 0;
    uint64_t max_bytes = 0;
    bool has_seed = false;
    Seed seed{};
    size_t in_capacity = 0, cub_bytes = 0;
    ResourceTally tally;  // every allocation and creation of the handle goes through it
    CastSlot slots[16];
    RingCursor ring;
    int last_collected = -1;
};

namespace {

int caster_create(int device, const uint8_t *seed32, uint32_t depth, uint32_t max_docs, uint32_t max_lexemes, uint64_t max_bytes,
                  uint32_t max_long_lexemes, vbm25_caster **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (depth < 1 || depth > 16) return set_error(VBM25_ERR_INVALID, "depth %u is outside 1 .. 16", depth);
    if (!max_docs || !max_lexemes) return set_error(VBM25_ERR_INVALID, "max_docs or max_lexemes is 0");
    if (max_docs >= (1u << 31) - 1u || max_lexemes >= (1u << 31))
        return set_error(VBM25_ERR_INVALID, "max_docs or max_lexemes is beyond one cast's limits (2^31 - 1 documents, 2^31 lexemes)");
    if (max_long_lexemes > max_lexemes) return set_error(VBM25_ERR_INVALID, "max_long_lexemes %u exceeds max_lexemes %u", max_long_lexemes, max_lexemes);
    if (max_bytes >= (1ull << 40)) return set_error(VBM25_ERR_INVALID, "max_bytes %llu is 2^40 or more", (unsigned long long)max_bytes);
    if (int rc = use_cast_device(device)) return rc;
    std::unique_ptr<vbm25_caster, void (*)(vbm25_caster *)> guard(new vbm25_caster, vbm25_caster_free);
    vbm25_caster *c = guard.get();
    ResourceTally &ta = c->tally;
    c->device = device;
    c->ring.depth = depth;
    c->max_docs = max_docs;
    c->max_lexemes = max_lexemes;
    c->max_bytes = max_bytes;
    c->max_long = max_long_lexemes;
    c->has_seed = seed32 != nullptr;
    seed_words(seed32, &c->seed);
    // (a batch has at most as many general-class documents and plan entries as documents)
    c->in_capacity = StageLayout(max_docs, max_lexemes, max_docs, max_docs, max_bytes).total;
    const uint64_t nd = max_docs, nl = max_lexemes, ng = max_long_lexemes;
    for (uint32_t i = 0; i < depth; ++i) {
        CastSlot &s = c->slots[i];
        HIP_TRY(ta.stream_create(s.stream));
        HIP_TRY(ta.event_create(s.start));
        HIP_TRY(ta.event_create(s.done));
        if (i == 0)
            if (int rc = cast_cub_bytes(max_docs, max_long_lexemes, s.stream.s, &c->cub_bytes)) return rc;
        HIP_TRY(ta.pinned_alloc(s.stage, c->in_capacity));
        HIP_TRY(ta.pinned_alloc(s.n_elements, 8));
        HIP_TRY(ta.device_alloc(s.in, c->in_capacity));
        HIP_TRY(ta.device_alloc(s.keys, 16 * nl));
        HIP_TRY(ta.device_alloc(s.tmp_key, 16 * nl));
        HIP_TRY(ta.device_alloc(s.tmp_tf, 4 * nl));
        HIP_TRY(ta.device_alloc(s.counts, 4 * (nd + 1)));
        HIP_TRY(ta.device_alloc(s.cub, c->cub_bytes));
        if (ng) {
            HIP_TRY(ta.device_alloc(s.g_src, 4 * ng));
            HIP_TRY(ta.device_alloc(s.g_slot, 4 * ng));
            HIP_TRY(ta.device_alloc(s.g_ka, 8 * ng));
            HIP_TRY(ta.device_alloc(s.g_kb, 8 * ng));
            HIP_TRY(ta.device_alloc(s.g_va, 4 * ng));
            HIP_TRY(ta.device_alloc(s.g_vb, 4 * ng));
            HIP_TRY(ta.device_alloc(s.g_prefix, 8 * ng));
            HIP_TRY(ta.device_alloc(s.g_head_pos, 4 * (ng + 1)));
        }
        s.docs.device = device;
        s.docs.caster = c;
        HIP_TRY(ta.device_alloc(s.docs.d_start, 8 * (nd + 1)));
        HIP_TRY(ta.device_alloc(s.docs.d_key, 16 * nl));
        HIP_TRY(ta.device_alloc(s.docs.d_tf, 4 * nl));
        HIP_TRY(ta.device_alloc(s.docs.d_length, 4 * nd));
        HIP_TRY(ta.device_alloc(s.docs.d_fieldnorm, nd));
        HIP_TRY(ta.device_alloc(s.docs.d_payload, 6 * nd));
    }
    *out = guard.release();
    return VBM25_OK;
}

int caster_submit(vbm25_caster *c, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *lex_count, const uint32_t *doc_lex, uint32_t n_docs,
                  const uint16_t *doc_payload) {
    if (!c) return set_error(VBM25_ERR_INVALID, "NULL argument");
    const uint32_t wave_max = g_wave_max.load(), group_max = g_group_max.load(), pack = g_cast_pack.load(), grid_cap = g_cast_grid.load();
    Shape sh;
    if (int rc = check_documents(c->has_seed, bytes, lex_off, lex_count, doc_lex, n_docs, &sh)) return rc;
    if (c->ring.full()) return set_error(VBM25_ERR_INVALID, "the caster's %u slots are all in flight: collect first", c->ring.depth);
    if (n_docs > c->max_docs) return set_error(VBM25_ERR_INVALID, "%u documents exceed the caster's max_docs %u", n_docs, c->max_docs);
    if (sh.n_lex > c->max_lexemes) return set_error(VBM25_ERR_INVALID, "%u lexemes exceed the caster's max_lexemes %u", sh.n_lex, c->max_lexemes);
    if (sh.n_bytes > c->max_bytes)
        return set_error(VBM25_ERR_INVALID, "%llu bytes exceed the caster's max_bytes %llu", (unsigned long long)sh.n_bytes, (unsigned long long)c->max_bytes);
    // pass 1: the classes' sizes and the plan's
    uint32_t n_class[3] = {0, 0, 0}, n_plan = 0, first_general = 0;
    uint64_t gen_el = 0;
    {
        PackRun run;
        PackEntry e;
        for (uint32_t d = 0; d < n_docs; ++d) {
            const uint32_t n = doc_lex[d + 1] - doc_lex[d];
            const DocClass cl = doc_class(n, wave_max, group_max);
            if (cl == CLASS_GENERAL && n && !gen_el) first_general = d;
            if (cl == CLASS_GENERAL) gen_el += n;
            ++n_class[cl];
            n_plan += pack_step(run, d, n, cl == CLASS_WAVE, e) ? 1u : 0u;
        }
        n_plan += pack_flush(run, e) ? 1u : 0u;
    }
    if (gen_el > c->max_long) {
        if (!c->max_long)
            return set_error(VBM25_ERR_UNSUPPORTED, "document %u has %u lexemes: the caster was created with max_long_lexemes 0 and takes no document of the general class",
                             first_general, doc_lex[first_general + 1] - doc_lex[first_general]);
        return set_error(VBM25_ERR_INVALID, "%llu lexemes in documents of the general class exceed the caster's max_long_lexemes %u",
                         (unsigned long long)gen_el, c->max_long);
    }
    const uint32_t n_lex = sh.n_lex, n_wave = n_class[0], n_group = n_class[1], n_gen = n_class[2], n_gen_el = uint32_t(gen_el);
    if (int rc = use_device(c->device)) return rc;
    CastSlot &s = c->slots[c->ring.tail()];
    {  // (hipcub is asked again for this batch's sizes -- a question, nothing is enqueued: its answer for less is expected to be less)
        size_t need = 0;
        if (int rc = cast_cub_bytes(n_docs, n_gen_el, s.stream.s, &need)) return rc;
        if (need > c->cub_bytes)
            return set_error(VBM25_ERR_UNSUPPORTED, "hipcub asks for %zu bytes of temporary storage for this batch, the caster holds %zu", need, c->cub_bytes);
    }
    const StageLayout L(n_docs, n_lex, n_gen, n_plan, sh.n_bytes);
    // pass 2: the lists, the general class's offsets and the plan, straight into the pinned block
    uint8_t *const staged = s.stage.as<uint8_t>();
    std::memcpy(staged + L.o_doc, doc_lex, 4ull * (n_docs + 1ull));
    std::memcpy(staged + L.o_off, lex_off, 8ull * (n_lex + 1ull));
    if (n_lex) std::memcpy(staged + L.o_cnt, lex_count, 4ull * n_lex);
    {
        uint32_t *list = reinterpret_cast<uint32_t *>(staged + L.o_list), *goff = reinterpret_cast<uint32_t *>(staged + L.o_goff);
        PackEntry *plan = reinterpret_cast<PackEntry *>(staged + L.o_plan);
        uint32_t at[3] = {0, n_wave, n_wave + n_group}, n_goff = 0, n_done = 0, el = 0;
        PackRun run;
        PackEntry e;
        goff[n_goff++] = 0;
        for (uint32_t d = 0; d < n_docs; ++d) {
            const uint32_t n = doc_lex[d + 1] - doc_lex[d];
            const DocClass cl = doc_class(n, wave_max, group_max);
            list[at[cl]++] = d;
            if (cl == CLASS_GENERAL) goff[n_goff++] = (el += n);
            if (pack_step(run, d, n, cl == CLASS_WAVE, e)) plan[n_done++] = e;
        }
        if (pack_flush(run, e)) plan[n_done++] = e;
    }
    std::memcpy(staged + L.o_fn, fieldnorm_lengths(), 4 * 256);
    if (doc_payload && n_docs) std::memcpy(staged + L.o_pay, doc_payload, 6ull * n_docs);
    if (sh.n_bytes) std::memcpy(staged + L.o_bytes, bytes, sh.n_bytes);
    if (L.total > L.o_bytes + sh.n_bytes) std::memset(staged + L.o_bytes + sh.n_bytes, 0, L.total - L.o_bytes - sh.n_bytes);

    hipStream_t st = s.stream.s;
    vbm25_documents &h = s.docs;
    uint8_t *d = s.in.as<uint8_t>();
    // a HIP error from here on leaves the slot out of the ring but with work enqueued: wait for it before the refusal returns, so that
    // the next submit, which takes this slot again, writes its pinned block under no copy in flight.  Let go of on success.
    Quiesce quiesce(st);
    HIP_TRY(hipMemcpyAsync(d, staged, L.total, hipMemcpyHostToDevice, st));
    if (doc_payload && n_docs) HIP_TRY(hipMemcpyAsync(h.d_payload.p, staged + L.o_pay, 6ull * n_docs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s.start.e, st));
    HIP_TRY(hipMemsetAsync(s.counts.p, 0, 4ull * (n_docs + 1ull), st));
    const uint32_t *d_doc = reinterpret_cast<const uint32_t *>(d + L.o_doc), *d_cnt = reinterpret_cast<const uint32_t *>(d + L.o_cnt),
                   *d_list = reinterpret_cast<const uint32_t *>(d + L.o_list), *d_goff = reinterpret_cast<const uint32_t *>(d + L.o_goff),
                   *d_fn = reinterpret_cast<const uint32_t *>(d + L.o_fn), *d_pool = reinterpret_cast<const uint32_t *>(d + L.o_bytes);
    const uint64_t *d_off = reinterpret_cast<const uint64_t *>(d + L.o_off);
    const PackEntry *d_plan = reinterpret_cast<const PackEntry *>(d + L.o_plan);
    const SortArgs sa{s.keys.as<Key>(), d_cnt, d_doc, s.tmp_key.as<Key>(), s.tmp_tf.as<uint32_t>(), s.counts.as<uint32_t>()};
    const uint32_t cap = grid_cap ? grid_cap : MAX_GRID;
    const uint32_t levels = stack_levels(sh.longest_lexeme);
    const bool fused = pack == 2 && n_lex && !n_group && !n_gen;  // (nobody but the packed waves needs the keys)
    uint32_t launched = 0;  // (which of the intern's and the wave class's kernels this batch takes: vbm25_debug_caster_launched)
    if (n_lex && !fused) {
        launched |= LAUNCHED_INTERN;
        const size_t lds = size_t(levels) * 8 * sizeof(uint32_t) * INTERN_THREADS;
        cast_intern_kernel<<<std::min(INTERN_GRID, grid_for(n_lex, INTERN_THREADS, cap)), INTERN_THREADS, lds, st>>>(c->seed, d_pool, d_off, n_lex, s.keys.as<Key>());
        HIP_TRY(hipGetLastError());
    }
    if (n_wave && n_lex) {
        if (fused) {  // a lexeme of several chunks: one wave a block, so that the stack (32 bytes a level a thread) fits the LDS
            const uint32_t threads = levels ? INTERN_THREADS : WG;
            launched |= LAUNCHED_PACK_FUSED;
            cast_pack_kernel<true><<<grid_for(n_plan, threads / 64, cap), threads, size_t(levels) * 8 * sizeof(uint32_t) * threads, st>>>(sa, d_plan, n_plan, c->seed,
                                                                                                                                   d_pool, d_off);
        } else if (pack) {
            launched |= LAUNCHED_PACK;
            cast_pack_kernel<false><<<grid_for(n_plan, WG / 64, cap), WG, 0, st>>>(sa, d_plan, n_plan, c->seed, d_pool, d_off);
        } else {
            launched |= LAUNCHED_WAVE;
            cast_wave_kernel<<<grid_for(n_wave, WG / 64, cap), WG, 0, st>>>(sa, d_list, n_wave);
        }
        HIP_TRY(hipGetLastError());
    }
    if (n_group && n_lex) {
        cast_group_kernel<<<grid_for(n_group, 1, cap), WG, 0, st>>>(sa, d_list + n_wave, n_group);
        HIP_TRY(hipGetLastError());
    }
    if (n_gen_el) {
        const GenArgs g{sa, d_list + n_wave + n_group, d_goff, n_gen, n_gen_el, s.g_src.as<uint32_t>(), s.g_slot.as<uint32_t>(), s.g_ka.as<ull>(),
                        s.g_kb.as<ull>(), s.g_va.as<uint32_t>(), s.g_vb.as<uint32_t>(), s.g_prefix.as<ull>(), s.g_head_pos.as<uint32_t>()};
        if (int rc = enqueue_general(st, g, s.cub.p, c->cub_bytes, grid_for(n_gen_el, WG, cap))) return rc;
    }
    size_t tb = c->cub_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.cub.p, tb, hipcub::TransformInputIterator<ull, WidenU32, const uint32_t *>(s.counts.as<uint32_t>(), WidenU32()),
                                            h.d_start.as<ull>(), int(n_docs + 1), st));
    // (key / tf have room for every lexeme: the gather goes straight behind the scan, and the number of elements travels home beside it)
    HIP_TRY(hipMemcpyAsync(s.n_elements.p, h.d_start.as<ull>() + n_docs, 8, hipMemcpyDeviceToHost, st));
    if (n_docs) {
        cast_gather_kernel<<<grid_for(n_docs, WG / 64, cap), WG, 0, st>>>(s.tmp_key.as<Key>(), s.tmp_tf.as<uint32_t>(), d_doc, h.d_start.as<ull>(), n_docs, d_fn,
                                                                          h.d_key.as<Key>(), h.d_tf.as<uint32_t>(), h.d_length.as<uint32_t>(),
                                                                          h.d_fieldnorm.as<uint8_t>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s.done.e, st));
    h.n_docs = n_docs;
    h.n_elements = 0;  // (known at collect)
    h.has_payload = doc_payload != nullptr;
    h.in_flight = true;
    s.launched = launched;
    c->ring.push();
    quiesce.s = nullptr;
    return VBM25_OK;
}

int caster_collect(vbm25_caster *c, const vbm25_documents **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (!c) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (c->ring.empty()) return set_error(VBM25_ERR_INVALID, "nothing is in flight on the caster");
    if (int rc = use_device(c->device)) return rc;
    CastSlot &s = c->slots[c->ring.head];
    HIP_TRY(hipEventSynchronize(s.done.e));
    s.docs.n_elements = *s.n_elements.as<ull>();
    s.docs.in_flight = false;
    *out = &s.docs;
    c->last_collected = int(c->ring.pop());
    return VBM25_OK;
}

// ---- vbm25_documents_extend ----
__global__ void __launch_bounds__(WG) extend_start_kernel(const ull *src_start, uint32_t n_src, ull base, ull *dst_start_at) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n_src; i += gridDim.x * WG) dst_start_at[i + 1] = src_start[i + 1] + base;
}

int documents_extend(vbm25_documents *dst, const vbm25_documents *src) {
    if (!dst || !src) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (dst == src) return set_error(VBM25_ERR_INVALID, "dst and src are the same handle");
    if (dst->caster) return set_error(VBM25_ERR_INVALID, "dst belongs to a caster: only an owned handle is extended");
    if (dst->device != src->device) return set_error(VBM25_ERR_INVALID, "dst is on device %d, src on device %d", dst->device, src->device);
    if (dst->has_payload != src->has_payload) return set_error(VBM25_ERR_INVALID, "one handle has payloads and the other has none");
    const uint64_t nd = uint64_t(dst->n_docs) + src->n_docs, ne = dst->n_elements + src->n_elements;
    if (nd >= (1ull << 31) - 1ull) return set_error(VBM25_ERR_UNSUPPORTED, "%llu documents: one handle takes fewer than 2^31 - 1", (unsigned long long)nd);
    if (ne >= (1ull << 31)) return set_error(VBM25_ERR_UNSUPPORTED, "%llu elements: one handle takes fewer than 2^31", (unsigned long long)ne);
    if (int rc = use_cast_device(dst->device)) return rc;
    if (!src->n_docs) return VBM25_OK;
    // per array: (the array, the bytes in use, the bytes needed, src's array, src's bytes)
    struct Part {
        HbmArray *a;
        uint64_t used, need;
        const void *from;
        uint64_t n_from;
    } parts[6] = {{&dst->d_start, 8ull * (dst->n_docs + 1ull), 8 * (nd + 1), nullptr, 0},
                  {&dst->d_key, 16 * dst->n_elements, 16 * ne, src->d_key.p, 16 * src->n_elements},
                  {&dst->d_tf, 4 * dst->n_elements, 4 * ne, src->d_tf.p, 4 * src->n_elements},
                  {&dst->d_length, 4ull * dst->n_docs, 4 * nd, src->d_length.p, 4ull * src->n_docs},
                  {&dst->d_fieldnorm, dst->n_docs, nd, src->d_fieldnorm.p, src->n_docs},
                  {&dst->d_payload, 6ull * dst->n_docs, 6 * nd, src->d_payload.p, 6ull * src->n_docs}};
    const int n_parts = dst->has_payload ? 6 : 5;
    HbmArray grown[6];
    Stream st;  // (of the call's own, as the cast's)
    HIP_TRY(st.create());
    Quiesce quiesce(st.s);
    // every larger array first: a failure so far leaves dst as it was.  Capacities at least double, so appending n chunks copies O(n) bytes.
    for (int i = 0; i < n_parts; ++i) {
        const Part &p = parts[i];
        if (p.need <= p.a->bytes) continue;
        HIP_TRY(grown[i].alloc(std::max<uint64_t>(p.need, 2 * uint64_t(p.a->bytes))));
    }
    for (int i = 0; i < n_parts; ++i) {
        const Part &p = parts[i];
        if (grown[i].p && p.used) HIP_TRY(hipMemcpyAsync(grown[i].p, p.a->p, p.used, hipMemcpyDeviceToDevice, st.s));
        uint8_t *to = static_cast<uint8_t *>(grown[i].p ? grown[i].p : p.a->p);
        if (p.from && p.n_from) HIP_TRY(hipMemcpyAsync(to + p.used, p.from, p.n_from, hipMemcpyDeviceToDevice, st.s));
    }
    ull *start = static_cast<ull *>(grown[0].p ? grown[0].p : dst->d_start.p);
    extend_start_kernel<<<grid_for(src->n_docs, WG, MAX_GRID), WG, 0, st.s>>>(src->d_start.as<ull>(), src->n_docs, dst->n_elements, start + dst->n_docs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st.s));
    for (int i = 0; i < n_parts; ++i)
        if (grown[i].p) {
            std::swap(grown[i].p, parts[i].a->p);  // (the old array goes with `grown`)
            std::swap(grown[i].bytes, parts[i].a->bytes);
        }
    dst->n_docs = uint32_t(nd);
    dst->n_elements = ne;
    return VBM25_OK;
}

}  // namespace

namespace vbm25 {
int cast_tuning_set(const char *name, long long value) {
    const std::string n(name);
    if (n == "cast_pack") {
        if (value < 0 || value > 2) return set_error(VBM25_ERR_INVALID, "%s %lld is outside 0 .. 2", name, value);
        g_cast_pack.store(uint32_t(value));
        return VBM25_OK;
    }
    if (n == "cast_grid") {
        if (value < 0 || value > (long long)MAX_GRID) return set_error(VBM25_ERR_INVALID, "%s %lld is outside 0 .. %u", name, value, MAX_GRID);
        g_cast_grid.store(uint32_t(value));
        return VBM25_OK;
    }
    std::atomic<uint32_t> &slot = n == "cast_wave_max" ? g_wave_max : g_group_max;
    const uint32_t bound = n == "cast_wave_max" ? CAST_WAVE_MAX : CAST_GROUP_MAX;
    if (value < 0 || value > (long long)bound) return set_error(VBM25_ERR_INVALID, "%s %lld is outside 0 .. %u", name, value, bound);
    slot.store(uint32_t(value));
    return VBM25_OK;
}
void cast_tuning_reset() {
    g_wave_max.store(CAST_WAVE_MAX);
    g_group_max.store(CAST_GROUP_MAX);
    g_cast_pack.store(CAST_PACK_DEFAULT);
    g_cast_grid.store(0);
}
}  // namespace vbm25

extern "C" {

int vbm25_documents_cast(int device, const uint8_t *seed32, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *lex_count,
                         const uint32_t *doc_lex, uint32_t n_docs, const uint16_t *doc_payload, vbm25_documents **out) {
    return guarded([&] { return documents_cast(device, seed32, bytes, lex_off, lex_count, doc_lex, n_docs, doc_payload, out); });
}

int vbm25_documents_info(const vbm25_documents *h, uint32_t *n_docs, uint64_t *n_elements, int *device) {
    if (!h) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_docs) *n_docs = h->n_docs;
    if (n_elements) *n_elements = h->n_elements;
    if (device) *device = h->device;
    return VBM25_OK;
}

int vbm25_documents_download(const vbm25_documents *h, vbm25_growing **csr, uint32_t *doc_len) {
    return guarded([&] { return documents_download(h, csr, doc_len); });
}

uint64_t vbm25_documents_device_bytes(const vbm25_documents *h) { return h ? handle_bytes(h) : 0; }

void vbm25_documents_free(vbm25_documents *h) {
    if (!h || h->caster) return;  // (a collected handle is its caster's)
    (void)hipSetDevice(h->device);
    delete h;
}

int vbm25_device_segment_build_documents(const vbm25_documents *h, double k1, double b, vbm25_device_segment **out) {
    return guarded([&] { return build_documents(h, k1, b, out); });
}

int vbm25_documents_extend(vbm25_documents *dst, const vbm25_documents *src) {
    return guarded([&] { return documents_extend(dst, src); });
}

int vbm25_caster_create(int device, const uint8_t *seed32, uint32_t depth, uint32_t max_docs, uint32_t max_lexemes, uint64_t max_bytes,
                        uint32_t max_long_lexemes, vbm25_caster **out) {
    return guarded([&] { return caster_create(device, seed32, depth, max_docs, max_lexemes, max_bytes, max_long_lexemes, out); });
}

void vbm25_caster_free(vbm25_caster *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (CastSlot &s : c->slots)
        if (s.stream.s) (void)hipStreamSynchronize(s.stream.s);  // nothing is freed under a kernel or a copy in flight
    delete c;  // (with the slots' vbm25_documents: a collected handle is not used after this)
}

uint64_t vbm25_caster_device_bytes(const vbm25_caster *c) { return c ? c->tally.device_bytes : 0; }

int vbm25_caster_info(const vbm25_caster *c, uint32_t *depth, int *device, uint64_t *allocations) {
    if (!c) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (depth) *depth = c->ring.depth;
    if (device) *device = c->device;
    if (allocations) *allocations = c->tally.allocations;
    return VBM25_OK;
}

int vbm25_caster_submit(vbm25_caster *c, const uint8_t *bytes, const uint64_t *lex_off, const uint32_t *lex_count, const uint32_t *doc_lex,
                        uint32_t n_docs, const uint16_t *doc_payload) {
    return guarded([&] { return caster_submit(c, bytes, lex_off, lex_count, doc_lex, n_docs, doc_payload); });
}

int vbm25_caster_collect(vbm25_caster *c, const vbm25_documents **out) {
    return guarded([&] { return caster_collect(c, out); });
}

int vbm25_caster_in_flight(const vbm25_caster *c) { return c ? int(c->ring.count) : 0; }

// tools/caster_cost.py: the device time of the last collected batch's kernels (upload excluded), by the slot's HIP events.  Not in the header.
int vbm25_debug_caster_kernel_ms(vbm25_caster *c, double *ms) {
    if (!c || !ms || c->last_collected < 0) return set_error(VBM25_ERR_INVALID, "no collected batch");
    const CastSlot &s = c->slots[c->last_collected];
    HIP_TRY(elapsed_ms(s.start, s.done, ms));
    return VBM25_OK;
}

// tests/test_gpu_caster.py: which kernels the last collected batch's lexemes and wave class went through -- 1 cast_intern_kernel,
// 2 cast_wave_kernel, 4 cast_pack_kernel with keys from HBM, 8 cast_pack_kernel interning in its lanes.  Not in the header.
int vbm25_debug_caster_launched(const vbm25_caster *c, uint32_t *mask) {
    if (!c || !mask || c->last_collected < 0) return set_error(VBM25_ERR_INVALID, "no collected batch");
    *mask = c->slots[c->last_collected].launched;
    return VBM25_OK;
}

// tools/cast_cost.py: the device time of the calling thread's last cast's kernels (upload and the host's allocation in front of the
// gather excluded), by HIP events.  Not in the header.
int vbm25_debug_cast_kernel_ms(double *ms) {
    if (!ms || g_kernel_ms < 0) return set_error(VBM25_ERR_INVALID, "no cast on this thread");
    *ms = g_kernel_ms;
    return VBM25_OK;
}

}  // extern "C"
