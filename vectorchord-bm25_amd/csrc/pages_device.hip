// pages_device.hip -- the device readers: a bm25 index relation in the reference's on-disk format -> a sealed segment in HBM
// (vbm25_device_segment_from_pages, below) and its vectors tape -> a device growing segment (vbm25_device_growing_from_pages,
// further down).  The sealed segment: same accept / refuse contract as the host reader (csrc/pages.cpp) followed by check_desc
// (csrc/segment.cpp); the result is byte for byte what vbm25_segment_from_pages flattens, without a host copy of the index.
//
//   host pass      Meta, Jump, then the four tapes by Opaque.next (pages_parse.h: walk_relation): one header check and one memcpy of the
//                  8 KiB image into pinned staging per page; a chunk of 1024 pages goes up asynchronously while the next one fills
//                  (two staging buffers).  Kept per page: its id and the running tuple count.  No tuple is touched on the host.
//   tape_kernel    documents / tokens / summaries: one wave per page, lane i takes slot i + 1 (+ 64 ...): line pointer validated,
//                  fields written at prefix[page] + i into the segment's planes
//   (scan)         ceil(df / 128) -> term_first_block, in 64 bits (hipcub)
//   term_kernel    one thread per token: its summaries lie inside the tape and begin where its pointer says; check_desc's per-term rules
//   tape_kernel    blocks: summary j points at the tape's j-th tuple, header against codec metadata, padded body length; check_desc's
//                  per-block rules (the first / last block of a token from the head flags term_kernel set)
//   (scan)         body lengths -> blk_off8; the total in 64 bits
//   copy_kernel    one wave per block page, 16 lanes per block: 8-byte units, doc bytes, zero padding, tf bytes, zero padding
// Every kernel is a loop over the functions of pages_parse.h and finishes normally on any input; errors meet in one 64-bit word
// (atomicMin of (class, tape, position, reason)): the reported one is the first in walk order.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <unordered_set>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "pages_parse.h"
#include "vectors_parse.h"

namespace {

using namespace vbm25;
using namespace vbm25::pgs;

// the last call's cost on this thread (vbm25_debug_pages_device_stats): kernels and scans between HIP events, bytes over the host
// link in both directions, host memory the call allocated (pinned staging included)
thread_local double g_stats[4];

constexpr uint32_t WG_THREADS = 256, MAX_GRID = 2048;

// one wave per page of tape TAPE, lane i takes slot i + 1 (+ 64 ...)
template <uint32_t TAPE>
__global__ void __launch_bounds__(WG_THREADS) tape_kernel(Planes c, unsigned long long *err) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    const uint32_t n_pages = c.tape[TAPE].n_pages;
    for (uint32_t p = wave; p < n_pages; p += n_waves) {
        const uint32_t base = c.tape[TAPE].pre[p], n = c.tape[TAPE].pre[p + 1] - base;
        for (uint32_t i = lane; i < n; i += 64) {
            const uint32_t r = TAPE == T_DOCS ? doc_lane(c, p, i) : TAPE == T_TOKENS ? token_lane(c, p, i) : TAPE == T_SUMMARIES ? summary_lane(c, p, i) : block_lane(c, p, i);
            if (r) atomicMin(err, (unsigned long long)error_key(TAPE, (uint64_t)base + i, r));
        }
    }
}

__global__ void __launch_bounds__(WG_THREADS) term_kernel(Planes c, unsigned long long *err) {
    const uint32_t n = c.tape[T_TOKENS].n_tuples;
    for (uint32_t t = blockIdx.x * WG_THREADS + threadIdx.x; t < n; t += gridDim.x * WG_THREADS) {
        const uint32_t r = term_lane(c, t);
        if (r) atomicMin(err, (unsigned long long)error_key(T_TOKENS, t, r));
    }
}

// one wave per block page, COPY_LANES lanes per block: a body of 16 (b_d + b_t) bytes is one or two coalesced requests
__global__ void __launch_bounds__(WG_THREADS) copy_kernel(Planes c) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    const uint32_t n_pages = c.tape[T_BLOCKS].n_pages;
    for (uint32_t p = wave; p < n_pages; p += n_waves) {
        const uint32_t n = c.tape[T_BLOCKS].pre[p + 1] - c.tape[T_BLOCKS].pre[p];
        for (uint32_t i = lane / COPY_LANES; i < n; i += 64 / COPY_LANES) copy_lane(c, p, i, lane % COPY_LANES);
    }
}

// out[t] = src[idx[t]]: the body offsets at the tokens' first blocks (the algorithmic bytes per token)
__global__ void __launch_bounds__(WG_THREADS) gather_kernel(uint32_t n, const uint32_t *idx, const uint32_t *src, uint32_t *out) {
    for (uint32_t t = blockIdx.x * WG_THREADS + threadIdx.x; t < n; t += gridDim.x * WG_THREADS) out[t] = src[idx[t]];
}

// Pinned staging of the host pass: pages fill one buffer while the other one's chunk is on its way up
struct Stager {
    hipStream_t s = nullptr;
    PinnedHost pin[2];
    Event ev[2];
    bool in_flight[2] = {false, false};
    int cur = 0;
    uint32_t fill = 0, tape = 0;
    uint64_t bytes_up = 0;
    std::vector<std::unique_ptr<HbmArray>> chunks[N_TAPES];

    int init(hipStream_t stream) {
        s = stream;
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(pin[i].alloc((size_t)CHUNK_PAGES * BLCKSZ));
            HIP_TRY(hipEventCreateWithFlags(&ev[i].e, hipEventDisableTiming));
        }
        return VBM25_OK;
    }
    int flush() {
        if (!fill) return VBM25_OK;
        auto d = std::make_unique<HbmArray>();
        HIP_TRY(d->alloc((size_t)fill * BLCKSZ));
        HIP_TRY(hipMemcpyAsync(d->p, pin[cur].p, (size_t)fill * BLCKSZ, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(ev[cur].e, s));
        in_flight[cur] = true;
        bytes_up += (uint64_t)fill * BLCKSZ;
        chunks[tape].push_back(std::move(d));
        fill = 0;
        cur ^= 1;
        if (in_flight[cur]) {  // the buffer to fill next: its chunk had a whole chunk's walk to arrive
            HIP_TRY(hipEventSynchronize(ev[cur].e));
            in_flight[cur] = false;
        }
        return VBM25_OK;
    }
    int add(uint32_t t, const uint8_t *image) {
        if (t != tape || fill == CHUNK_PAGES) {
            if (int rc = flush()) return rc;
            tape = t;
        }
        std::memcpy(static_cast<uint8_t *>(pin[cur].p) + (size_t)fill * BLCKSZ, image, BLCKSZ);
        ++fill;
        return VBM25_OK;
    }
};

int corrupt(const char *what, uint32_t page) { return set_error(VBM25_ERR_CORRUPT, "data corruption: %s (page %u)", what, page); }

int from_pages_impl(vbm25_read_page_fn read_page, void *ctx, int device, vbm25_device_segment **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!read_page) return set_error(VBM25_ERR_INVALID, "NULL argument");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: the device reader has no CPU fallback (vbm25_segment_from_pages is the host reader)");
    if (device < 0 || device >= n_dev) return set_error(VBM25_ERR_INVALID, "device %d out of range (%d devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    for (double &x : g_stats) x = 0.0;

    Stream stream;
    HIP_TRY(stream.create());
    hipStream_t s = stream.s;
    Stager st;
    if (int rc = st.init(s)) return rc;

    // ---- the host pass
    Walk w;
    int sink_rc = 0;
    const bool walked = walk_relation(read_page, ctx, w, [&](uint32_t tape, uint32_t, const uint8_t *image) { return st.add(tape, image); }, sink_rc);
    if (!walked) {
        (void)hipStreamSynchronize(s);  // nothing is freed under a copy in flight
        return sink_rc ? sink_rc : corrupt(w.what, w.bad_page);
    }
    if (int rc = st.flush()) return rc;
    const uint32_t n_docs = w.n_docs, n_tok = w.pre[T_TOKENS].back(), n_sum = w.pre[T_SUMMARIES].back();
    if (n_sum >= (uint32_t)INT_MAX || n_tok >= (uint32_t)INT_MAX) return set_error(VBM25_ERR_UNSUPPORTED, "more than 2^31 tokens or blocks");
    uint64_t host_bytes = 2ull * CHUNK_PAGES * BLCKSZ, bytes_down = 0;

    // ---- the tapes' tables
    HbmArray d_chunk[N_TAPES], d_pid[N_TAPES], d_pre[N_TAPES];
    std::vector<const uint8_t *> chunk_ptr[N_TAPES];
    Planes c{};
    c.n_docs = n_docs;
    for (uint32_t t = 0; t < N_TAPES; ++t) {
        const size_t np = w.pid[t].size();
        for (const auto &d : st.chunks[t]) chunk_ptr[t].push_back(d->as<uint8_t>());
        HIP_TRY(d_chunk[t].alloc(sizeof(void *) * chunk_ptr[t].size()));
        HIP_TRY(d_pid[t].alloc(4 * np));
        HIP_TRY(d_pre[t].alloc(4 * (np + 1)));
        if (np) {
            HIP_TRY(hipMemcpyAsync(d_chunk[t].p, chunk_ptr[t].data(), sizeof(void *) * chunk_ptr[t].size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_pid[t].p, w.pid[t].data(), 4 * np, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipMemcpyAsync(d_pre[t].p, w.pre[t].data(), 4 * (np + 1), hipMemcpyHostToDevice, s));
        st.bytes_up += 8 * chunk_ptr[t].size() + 8 * np + 4;
        host_bytes += 8 * np + 4 + 8 * chunk_ptr[t].size();
        c.tape[t] = TapeView{d_chunk[t].as<const uint8_t *>(), d_pid[t].as<uint32_t>(), d_pre[t].as<uint32_t>(), (uint32_t)np, w.pre[t].back()};
    }

    // ---- the segment's planes and the call's scratch
    auto ds = std::make_unique<vbm25_device_segment>();
    ds->device = device;
    ds->k1 = w.k1;
    ds->b = w.b;
    ds->n_docs = n_docs;
    ds->n_terms = n_tok;
    ds->n_blocks = n_sum;
    ds->sum_len = w.sum_len;
    HbmArray d_key, d_tok_page, d_tok_slot, d_tok_nb, d_tok_fb, d_sum_page, d_sum_slot, d_head, d_len8, d_err, d_total, d_tmp, d_bnd;
    HIP_TRY(ds->d_doc_fieldnorm.alloc(n_docs));
    HIP_TRY(ds->d_doc_payload.alloc(6ull * n_docs));
    HIP_TRY(ds->d_term_df.alloc(4ull * n_tok));
    HIP_TRY(ds->d_term_wand_fn.alloc(n_tok));
    HIP_TRY(ds->d_term_wand_tf.alloc(4ull * n_tok));
    HIP_TRY(ds->d_term_first_block.alloc(4ull * (n_tok + 1)));
    HIP_TRY(ds->d_blk_min.alloc(4ull * n_sum));
    HIP_TRY(ds->d_blk_max.alloc(4ull * n_sum));
    HIP_TRY(ds->d_blk_wand_tf.alloc(4ull * n_sum));
    HIP_TRY(ds->d_blk_n.alloc(n_sum));
    HIP_TRY(ds->d_blk_wand_fn.alloc(n_sum));
    HIP_TRY(ds->d_blk_meta_doc.alloc(n_sum));
    HIP_TRY(ds->d_blk_meta_tf.alloc(n_sum));
    HIP_TRY(ds->d_blk_off8.alloc(4ull * (n_sum + 1)));
    HIP_TRY(d_key.alloc(16ull * n_tok));
    HIP_TRY(d_tok_page.alloc(4ull * n_tok));
    HIP_TRY(d_tok_slot.alloc(2ull * n_tok));
    HIP_TRY(d_tok_nb.alloc(4ull * n_tok));
    HIP_TRY(d_tok_fb.alloc(8ull * n_tok));
    HIP_TRY(d_sum_page.alloc(4ull * n_sum));
    HIP_TRY(d_sum_slot.alloc(2ull * n_sum));
    HIP_TRY(d_head.alloc(n_sum + 1ull));
    HIP_TRY(d_len8.alloc(4ull * (n_sum + 1)));
    HIP_TRY(d_err.alloc(8));
    HIP_TRY(d_total.alloc(8));
    c.doc_fieldnorm = ds->d_doc_fieldnorm.as<uint8_t>();
    c.doc_payload = ds->d_doc_payload.as<uint16_t>();
    c.term_key = d_key.as<uint8_t>();
    c.term_wand_fn = ds->d_term_wand_fn.as<uint8_t>();
    c.term_wand_tf = ds->d_term_wand_tf.as<uint32_t>();
    c.term_df = ds->d_term_df.as<uint32_t>();
    c.term_first_block = ds->d_term_first_block.as<uint32_t>();
    c.tok_page = d_tok_page.as<uint32_t>();
    c.tok_slot = d_tok_slot.as<uint16_t>();
    c.tok_nb = d_tok_nb.as<uint32_t>();
    c.tok_fb = d_tok_fb.as<unsigned long long>();
    c.blk_min = ds->d_blk_min.as<uint32_t>();
    c.blk_max = ds->d_blk_max.as<uint32_t>();
    c.blk_wand_tf = ds->d_blk_wand_tf.as<uint32_t>();
    c.blk_n = ds->d_blk_n.as<uint8_t>();
    c.blk_wand_fn = ds->d_blk_wand_fn.as<uint8_t>();
    c.blk_meta_doc = ds->d_blk_meta_doc.as<uint8_t>();
    c.blk_meta_tf = ds->d_blk_meta_tf.as<uint8_t>();
    c.sum_blk_page = d_sum_page.as<uint32_t>();
    c.sum_blk_slot = d_sum_slot.as<uint16_t>();
    c.blk_head = d_head.as<uint8_t>();
    c.len8 = d_len8.as<uint32_t>();
    c.off8 = ds->d_blk_off8.as<uint32_t>();
    unsigned long long *err = d_err.as<unsigned long long>();

    Event ev[4];
    for (Event &e : ev) HIP_TRY(e.create());
    HIP_TRY(hipEventRecord(ev[0].e, s));
    HIP_TRY(hipMemsetAsync(d_err.p, 0xff, 8, s));
    HIP_TRY(hipMemsetAsync(d_total.p, 0, 8, s));
    HIP_TRY(hipMemsetAsync(d_head.p, 0, n_sum + 1ull, s));
    HIP_TRY(hipMemsetAsync(d_len8.p, 0, 4ull * (n_sum + 1), s));
    HIP_TRY(hipMemsetAsync(ds->d_term_first_block.p, 0, 4, s));
    if (n_docs) tape_kernel<T_DOCS><<<grid_for(c.tape[T_DOCS].n_pages, 4, MAX_GRID), WG_THREADS, 0, s>>>(c, err);
    if (n_tok) {
        tape_kernel<T_TOKENS><<<grid_for(c.tape[T_TOKENS].n_pages, 4, MAX_GRID), WG_THREADS, 0, s>>>(c, err);
        hipcub::TransformInputIterator<unsigned long long, WidenU32, const uint32_t *> wide(c.tok_nb, WidenU32());
        HIP_TRY(with_cub_temp(d_tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, wide, d_tok_fb.as<unsigned long long>(), (int)n_tok, s); }));
    }
    if (n_sum) tape_kernel<T_SUMMARIES><<<grid_for(c.tape[T_SUMMARIES].n_pages, 4, MAX_GRID), WG_THREADS, 0, s>>>(c, err);
    if (n_tok) term_kernel<<<grid_for(n_tok, WG_THREADS, MAX_GRID), WG_THREADS, 0, s>>>(c, err);
    HbmArray d_tmp2, d_tmp3;
    if (n_sum) {
        tape_kernel<T_BLOCKS><<<grid_for(c.tape[T_BLOCKS].n_pages, 4, MAX_GRID), WG_THREADS, 0, s>>>(c, err);
        HIP_TRY(with_cub_temp(d_tmp2, [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, c.len8, ds->d_blk_off8.as<uint32_t>(), (int)(n_sum + 1), s); }));
        // a 32-bit scan wraps silently beyond 2^32 units of 8 bytes: the total in 64 bits as well
        hipcub::TransformInputIterator<unsigned long long, WidenU32, const uint32_t *> wide(c.len8, WidenU32());
        HIP_TRY(with_cub_temp(d_tmp3, [&](void *t, size_t &tb) { return hipcub::DeviceReduce::Sum(t, tb, wide, d_total.as<unsigned long long>(), (int)n_sum, s); }));
    } else {
        HIP_TRY(hipMemsetAsync(ds->d_blk_off8.p, 0, 4, s));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1].e, s));
    unsigned long long key = 0, total8 = 0;
    HIP_TRY(hipMemcpyAsync(&key, d_err.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&total8, d_total.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    bytes_down += 16;

    // ---- the verdict, in the host reader's order
    bool ascending = true;
    uint32_t unordered_at = 0;
    if (key == NO_ERROR || key_reason(key) >= R_DESC) {
        ds->term_key.resize(16ull * n_tok);
        if (n_tok) HIP_TRY(hipMemcpy(ds->term_key.data(), d_key.p, 16ull * n_tok, hipMemcpyDeviceToHost));
        bytes_down += 16ull * n_tok;
        for (uint32_t t = 1; t < n_tok && ascending; ++t)
            if (std::memcmp(ds->term_key.data() + 16ull * (t - 1), ds->term_key.data() + 16ull * t, 16) >= 0) ascending = false, unordered_at = t;
    }
    const char *what = nullptr;
    if (int rc = verdict(w, key, ascending, what)) {
        if (rc != VBM25_ERR_CORRUPT) return set_error(rc, "%s", what);
        const uint64_t at = key != NO_ERROR ? key : !ascending ? error_key(T_TOKENS, unordered_at, 0) : error_key(T_TOKENS, 0, 0);
        return corrupt(what, error_page(w, at));
    }
    if (total8 > 0xffffffffull) return set_error(VBM25_ERR_UNSUPPORTED, "block bodies exceed 32 GiB");

    // ---- the bodies, and what the host keeps of the tokens
    ds->blob_bytes = 8ull * total8;
    HIP_TRY(ds->d_blob.alloc(ds->blob_bytes));
    c.blob = ds->d_blob.as<uint8_t>();
    ds->term_df.resize(n_tok);
    ds->term_first_block.assign(size_t(n_tok) + 1, 0);
    ds->term_bytes.assign(n_tok, 0);
    HIP_TRY(hipEventRecord(ev[2].e, s));
    if (n_sum) copy_kernel<<<grid_for(c.tape[T_BLOCKS].n_pages, 4, MAX_GRID), WG_THREADS, 0, s>>>(c);
    if (n_tok) {
        HIP_TRY(d_bnd.alloc(4ull * (n_tok + 1)));
        gather_kernel<<<grid_for(n_tok + 1ull, WG_THREADS, MAX_GRID), WG_THREADS, 0, s>>>(n_tok + 1, c.term_first_block, c.off8, d_bnd.as<uint32_t>());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[3].e, s));
    std::vector<uint32_t> bnd(size_t(n_tok) + 1, 0);
    if (n_tok) {
        HIP_TRY(hipMemcpyAsync(ds->term_df.data(), ds->d_term_df.p, 4ull * n_tok, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(ds->term_first_block.data(), ds->d_term_first_block.p, 4ull * (n_tok + 1), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(bnd.data(), d_bnd.p, 4ull * (n_tok + 1), hipMemcpyDeviceToHost, s));
        bytes_down += 12ull * n_tok + 8;
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t t = 0; t < n_tok; ++t)
        ds->term_bytes[t] = 8ull * (bnd[t + 1] - bnd[t]) + 40ull * (ds->term_first_block[t + 1] - ds->term_first_block[t]) + ds->term_df[t];
    float ms_a = 0, ms_b = 0;
    HIP_TRY(hipEventElapsedTime(&ms_a, ev[0].e, ev[1].e));
    HIP_TRY(hipEventElapsedTime(&ms_b, ev[2].e, ev[3].e));
    host_bytes += 16ull * n_tok + 4ull * n_tok + 4ull * (n_tok + 1) + 8ull * n_tok + 4ull * (n_tok + 1);  // keys, df, first blocks, bytes, bnd
    g_stats[0] = (double)ms_a + (double)ms_b;
    g_stats[1] = (double)st.bytes_up;
    g_stats[2] = (double)bytes_down;
    g_stats[3] = (double)host_bytes;
    *out = ds.release();
    return VBM25_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The vectors tape -> a device growing segment (vbm25_device_growing_from_pages; vectors_parse.h has the tuple layout and the lanes).
//   host pass            Meta, Jump, the vectors tape by Opaque.next (walk_vectors), staged and uploaded as above
//   vec_classify_kernel  one wave per page, lane i takes slot i + 1 (+ 64 ...): line pointer, length, tag, element range
//   (scans)              t_sum: attempt number and documents ended; t_last: is the tuple open (hipcub, 64 bits)
//   vec_resolve_kernel   one thread per tuple: continuation / end without a start; an open _0 finishes its attempt
//   vec_kept_kernel      one thread per tuple: the elements it gives (none in an attempt that did not finish)
//   (scan)               t_eoff: element offsets, the total in 64 bits
//   vec_finish_kernel    one wave per page, lane per slot: fieldnorm from the _2; deleted, payload and start[g + 1] from the _0
//   vec_copy_kernel      one wave per page, lanes over the page's ELEMENTS: 20 bytes -> the key plane (16) and the tf plane (4)
//   vec_check_kernel     the same lanes: keys strictly ascending inside a document (vbm25_growing_upload's rule)
// then the device half of vbm25_growing_upload (growing.hip) on those arrays.
// ---------------------------------------------------------------------------------------------------------------------------------
struct TupleIncrement {
    __host__ __device__ unsigned long long operator()(uint32_t meta) const { return tuple_increment(meta); }
};
struct MaxU64 {
    __host__ __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; }
};

thread_local double g_vec_stats[4];

__global__ void __launch_bounds__(WG_THREADS) vec_classify_kernel(VecPlanes c, unsigned long long *err) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    for (uint32_t p = wave; p < c.tape.n_pages; p += n_waves) {
        const uint32_t base = c.tape.pre[p], n = c.tape.pre[p + 1] - base;
        for (uint32_t i = lane; i < n; i += 64)
            if (const uint32_t r = classify_lane(c, p, i)) atomicMin(err, (unsigned long long)error_key(0, (uint64_t)base + i, r));
    }
}

__global__ void __launch_bounds__(WG_THREADS) vec_resolve_kernel(VecPlanes c, unsigned long long *err) {
    for (uint64_t g = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x; g < c.tape.n_tuples; g += (uint64_t)gridDim.x * WG_THREADS)
        if (const uint32_t r = resolve_lane(c, g)) atomicMin(err, (unsigned long long)error_key(0, g, r));
}

__global__ void __launch_bounds__(WG_THREADS) vec_kept_kernel(VecPlanes c) {
    for (uint64_t g = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x; g < c.tape.n_tuples; g += (uint64_t)gridDim.x * WG_THREADS) kept_lane(c, g);
}

__global__ void __launch_bounds__(WG_THREADS) vec_finish_kernel(VecPlanes c) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    for (uint32_t p = wave; p < c.tape.n_pages; p += n_waves) {
        const uint32_t n = c.tape.pre[p + 1] - c.tape.pre[p];
        for (uint32_t i = lane; i < n; i += 64) finish_lane(c, p, i);
    }
}

__global__ void __launch_bounds__(WG_THREADS) vec_copy_kernel(VecPlanes c) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    for (uint32_t p = wave; p < c.tape.n_pages; p += n_waves) {
        const uint32_t m = page_elements(c, p);
        for (uint32_t j = lane; j < m; j += 64) copy_element_lane(c, p, j);
    }
}

__global__ void __launch_bounds__(WG_THREADS) vec_check_kernel(VecPlanes c, unsigned long long *err) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    for (uint32_t p = wave; p < c.tape.n_pages; p += n_waves) {
        const uint32_t m = page_elements(c, p);
        for (uint32_t j = lane; j < m; j += 64) {
            uint32_t doc = 0;
            if (const uint32_t r = check_element_lane(c, p, j, doc)) atomicMin(err, (unsigned long long)error_key(0, doc, r));
        }
    }
}

// The vectors tape's CSR in HBM: where the reader's first half leaves it and what its callers keep (the vacuum handle) or build a
// device growing segment of
struct VecCsr {
    uint32_t n_docs = 0;
    uint64_t n_el = 0;
    HbmArray *start, *key, *tf, *fieldnorm, *deleted, *payload;
    double kernel_ms = 0.0;
    uint64_t bytes_down = 0;
};

// The reader's first half: the host pass and the kernels above, up to a validated CSR in HBM (synchronised).  The pages are staged
// through `st` into its chunk list `slot`; ptr_vectors: Jump.ptr_vectors of a Jump tuple the caller has read (NULL: Meta and Jump
// are read here).  Refusals in vbm25_device_growing_from_pages' documented order.
int vectors_csr(hipStream_t s, Stager &st, uint32_t slot, vbm25_read_page_fn read_page, void *ctx, const uint32_t *ptr_vectors,
                uint32_t sealed_docs, VecCsr &o) {
    // ---- the host pass
    Walk w;
    int sink_rc = 0;
    auto sink = [&](uint32_t, uint32_t, const uint8_t *image) { return st.add(slot, image); };
    const bool walked = ptr_vectors ? walk_vectors_from(read_page, ctx, w, *ptr_vectors, sink, sink_rc) : walk_vectors(read_page, ctx, w, sink, sink_rc);
    if (!walked) {
        (void)hipStreamSynchronize(s);  // nothing is freed under a copy in flight
        return sink_rc ? sink_rc : corrupt(w.what, w.bad_page);
    }
    if (int rc = st.flush()) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    const size_t np = w.pid[0].size();
    const uint64_t n = w.pre[0].back();
    if (n + 1 >= (uint64_t)INT_MAX) {
        (void)hipStreamSynchronize(s);
        return set_error(VBM25_ERR_UNSUPPORTED, "more than 2^31 tuples on the vectors tape");
    }
    uint64_t bytes_down = 0;

    // ---- the tape's tables and the call's scratch.  From here on a failure returns through the buffers' destructors: hipFree waits
    // for the device, nothing is freed under a kernel or a copy in flight
    HbmArray d_chunk, d_pre, d_meta, d_cnt, d_mark, d_sum, d_last, d_fin, d_kept, d_eoff, d_err, d_tmp[3];
    std::vector<const uint8_t *> chunk_ptr;
    for (const auto &d : st.chunks[slot]) chunk_ptr.push_back(d->as<uint8_t>());
    HIP_TRY(d_chunk.alloc(sizeof(void *) * chunk_ptr.size()));
    HIP_TRY(d_pre.alloc(4 * (np + 1)));
    if (np) HIP_TRY(hipMemcpyAsync(d_chunk.p, chunk_ptr.data(), sizeof(void *) * chunk_ptr.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_pre.p, w.pre[0].data(), 4 * (np + 1), hipMemcpyHostToDevice, s));
    st.bytes_up += 8 * chunk_ptr.size() + 4 * (np + 1);
    HIP_TRY(d_meta.alloc(4 * n));
    HIP_TRY(d_cnt.alloc(4 * n));
    HIP_TRY(d_mark.alloc(8 * n));
    HIP_TRY(d_sum.alloc(8 * n));
    HIP_TRY(d_last.alloc(8 * n));
    HIP_TRY(d_fin.alloc(n + 1));
    HIP_TRY(d_kept.alloc(4 * (n + 1)));
    HIP_TRY(d_eoff.alloc(8 * (n + 1)));
    HIP_TRY(d_err.alloc(8));
    VecPlanes c{};
    c.tape = TapeView{d_chunk.as<const uint8_t *>(), nullptr, d_pre.as<uint32_t>(), (uint32_t)np, (uint32_t)n};
    c.t_meta = d_meta.as<uint32_t>();
    c.t_cnt = d_cnt.as<uint32_t>();
    c.t_mark = d_mark.as<unsigned long long>();
    c.t_sum = d_sum.as<unsigned long long>();
    c.t_last = d_last.as<unsigned long long>();
    c.finished = d_fin.as<uint8_t>();
    c.t_kept = d_kept.as<uint32_t>();
    c.t_eoff = d_eoff.as<unsigned long long>();
    unsigned long long *err = d_err.as<unsigned long long>();
    const uint32_t page_grid = grid_for(np, 4, MAX_GRID), tuple_grid = grid_for(n, WG_THREADS, MAX_GRID);

    Event ev[4];
    for (Event &e : ev) HIP_TRY(e.create());
    HIP_TRY(hipEventRecord(ev[0].e, s));
    HIP_TRY(hipMemsetAsync(d_err.p, 0xff, 8, s));
    HIP_TRY(hipMemsetAsync(d_fin.p, 0, n + 1, s));
    HIP_TRY(hipMemsetAsync(d_kept.p, 0, 4 * (n + 1), s));
    if (n) {
        vec_classify_kernel<<<page_grid, WG_THREADS, 0, s>>>(c, err);
        hipcub::TransformInputIterator<unsigned long long, TupleIncrement, const uint32_t *> inc(c.t_meta, TupleIncrement());
        HIP_TRY(with_cub_temp(d_tmp[0], [&](void *t, size_t &tb) { return hipcub::DeviceScan::InclusiveSum(t, tb, inc, d_sum.as<unsigned long long>(), (int)n, s); }));
        HIP_TRY(with_cub_temp(d_tmp[1], [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveScan(t, tb, c.t_mark, d_last.as<unsigned long long>(), MaxU64(), 0ull, (int)n, s); }));
        vec_resolve_kernel<<<tuple_grid, WG_THREADS, 0, s>>>(c, err);
        vec_kept_kernel<<<tuple_grid, WG_THREADS, 0, s>>>(c);
    }
    {   // n + 1 entries: the last one is the total
        hipcub::TransformInputIterator<unsigned long long, WidenU32, const uint32_t *> wide(c.t_kept, WidenU32());
        HIP_TRY(with_cub_temp(d_tmp[2], [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, wide, d_eoff.as<unsigned long long>(), (int)(n + 1), s); }));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1].e, s));
    unsigned long long key = 0, counts = 0, n_el = 0;
    HIP_TRY(hipMemcpyAsync(&key, d_err.p, 8, hipMemcpyDeviceToHost, s));
    if (n) HIP_TRY(hipMemcpyAsync(&counts, d_sum.as<unsigned long long>() + (n - 1), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&n_el, d_eoff.as<unsigned long long>() + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    bytes_down += 24;

    // ---- the verdict so far: the host reader's refusals, then vbm25_growing_upload's in its order
    if (key != NO_ERROR) return corrupt(vreason_text(key_reason(key)), error_page(w, key));
    const uint32_t n_docs = (uint32_t)counts;  // every _0 of a tape without a refusal ended a document
    if ((uint64_t)sealed_docs + n_docs > (1ull << 32))
        return set_error(VBM25_ERR_INVALID, "%u sealed + %llu growing documents exceed 2^32: the doc id ranges would collide", sealed_docs,
                         (unsigned long long)n_docs);
    if (n_el >= (1ull << 31))
        return set_error(VBM25_ERR_UNSUPPORTED, "%llu growing elements: the device path takes fewer than 2^31", n_el);

    // ---- the CSR
    HbmArray &d_start = *o.start, &d_key = *o.key, &d_tf = *o.tf, &d_fn = *o.fieldnorm, &d_del = *o.deleted, &d_payload = *o.payload;
    HIP_TRY(d_start.alloc(8ull * (n_docs + 1ull)));
    HIP_TRY(d_key.alloc(16ull * n_el));
    HIP_TRY(d_tf.alloc(4ull * n_el));
    HIP_TRY(d_fn.alloc(n_docs));
    HIP_TRY(d_del.alloc(n_docs));
    HIP_TRY(d_payload.alloc(6ull * n_docs));
    c.n_docs = n_docs;
    c.n_el = n_el;
    c.start = d_start.as<unsigned long long>();
    c.key = d_key.as<uint8_t>();
    c.tf = d_tf.as<uint32_t>();
    c.fieldnorm = d_fn.as<uint8_t>();
    c.deleted = d_del.as<uint8_t>();
    c.payload = d_payload.as<uint16_t>();
    HIP_TRY(hipEventRecord(ev[2].e, s));
    HIP_TRY(hipMemsetAsync(d_start.p, 0, 8, s));
    if (n_docs) vec_finish_kernel<<<page_grid, WG_THREADS, 0, s>>>(c);
    if (n_el) {
        vec_copy_kernel<<<page_grid, WG_THREADS, 0, s>>>(c);
        vec_check_kernel<<<page_grid, WG_THREADS, 0, s>>>(c, err);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[3].e, s));
    HIP_TRY(hipMemcpyAsync(&key, d_err.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    bytes_down += 8;
    if (key != NO_ERROR)
        return set_error(VBM25_ERR_INVALID, "growing document %u: keys must be strictly ascending", (uint32_t)key_pos(key));
    float ms_a = 0, ms_b = 0;
    HIP_TRY(hipEventElapsedTime(&ms_a, ev[0].e, ev[1].e));
    HIP_TRY(hipEventElapsedTime(&ms_b, ev[2].e, ev[3].e));
    o.n_docs = n_docs;
    o.n_el = n_el;
    o.kernel_ms = (double)ms_a + (double)ms_b;
    o.bytes_down = bytes_down;
    return VBM25_OK;
}

int growing_from_pages_impl(vbm25_index *index, vbm25_read_page_fn read_page, void *ctx, vbm25_device_growing **out, vbm25_growing **csr) {
    if (csr) *csr = nullptr;
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!index || !read_page) return set_error(VBM25_ERR_INVALID, "NULL argument");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: the device reader has no CPU fallback (vbm25_growing_from_pages is the host reader)");
    int device = 0;
    uint32_t sealed_docs = 0;
    if (int rc = index_device_and_docs(index, &device, &sealed_docs)) return rc;
    HIP_TRY(hipSetDevice(device));
    for (double &x : g_vec_stats) x = 0.0;

    Stream stream;
    HIP_TRY(stream.create());
    hipStream_t s = stream.s;
    // (the planes before the stager: they go last, after the stream's work has been waited for)
    HbmArray d_start, d_key, d_tf, d_fn, d_del, d_payload;
    Stager st;
    if (int rc = st.init(s)) return rc;
    VecCsr v;
    v.start = &d_start, v.key = &d_key, v.tf = &d_tf, v.fieldnorm = &d_fn, v.deleted = &d_del, v.payload = &d_payload;
    if (int rc = vectors_csr(s, st, 0, read_page, ctx, nullptr, sealed_docs, v)) return rc;
    const uint32_t n_docs = v.n_docs;
    const uint64_t n_el = v.n_el;
    uint64_t bytes_down = v.bytes_down;

    // ---- the CSR's host copy, when asked for
    std::unique_ptr<vbm25_growing> host;
    if (csr) {
        host = std::make_unique<vbm25_growing>();
        host->start.resize(n_docs + 1ull);
        host->key.resize(16ull * n_el);
        host->tf.resize(n_el);
        host->fieldnorm.resize(n_docs);
        host->payload.resize(3ull * n_docs);
        host->deleted.resize(n_docs);
        HIP_TRY(hipMemcpyAsync(host->start.data(), d_start.p, 8ull * (n_docs + 1ull), hipMemcpyDeviceToHost, s));
        if (n_el) {
            HIP_TRY(hipMemcpyAsync(host->key.data(), d_key.p, 16ull * n_el, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(host->tf.data(), d_tf.p, 4ull * n_el, hipMemcpyDeviceToHost, s));
        }
        if (n_docs) {
            HIP_TRY(hipMemcpyAsync(host->fieldnorm.data(), d_fn.p, n_docs, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(host->payload.data(), d_payload.p, 6ull * n_docs, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(host->deleted.data(), d_del.p, n_docs, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        bytes_down += 8ull * (n_docs + 1ull) + 20ull * n_el + 8ull * n_docs;
    }

    // ---- the segment: the device half of vbm25_growing_upload
    const GrowingDeviceArrays a{n_docs, n_el, d_start.as<uint64_t>(), d_key.as<uint8_t>(), d_tf.as<uint32_t>(), d_fn.as<uint8_t>(),
                                d_del.as<uint8_t>(), d_payload.as<uint16_t>()};
    if (int rc = growing_from_device_arrays(index, a, out)) return rc;
    g_vec_stats[0] = v.kernel_ms;
    g_vec_stats[1] = (double)st.bytes_up;
    g_vec_stats[2] = (double)bytes_down;
    g_vec_stats[3] = (double)n_el;
    if (csr) *csr = host.release();
    return VBM25_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// A relation's compaction inputs -> HBM (vbm25_device_vacuum_from_pages): the sealed documents' deleted flags as words, then the
// vectors tape's CSR by vectors_csr above, both kept in the handle.
//   host pass            Meta and Jump once; the documents tape by Opaque.next, staged and uploaded as above; then the vectors tape
//   doc_deleted_kernel   one wave per documents-tape page, lane i takes slot i + 1 (+ 64 ...): doc_deleted_lane, a ballot per round of
//                        64 slots, the round's 64 flags ORed into the one or two words they fall into
//   (reductions)         popcounts of the words, nonzero bytes of the growing `deleted` plane (hipcub)
// A page holds up to 680 document tuples = 10 x 64 + 40, so the rounds of a page are not word aligned and the words at a page boundary
// belong to two waves.  The words are zeroed first and written with atomicOr only: OR commutes, the result does not depend on the
// order the waves run in, and a round costs two atomics where a byte-per-document plane packed by a second kernel would cost a
// store per document, a second pass over n_docs bytes and the plane itself.  No grid cap and no stride: one wave per page.
// ---------------------------------------------------------------------------------------------------------------------------------
struct PopCount64 {
    __host__ __device__ uint32_t operator()(unsigned long long w) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return (uint32_t)__popcll(w);
#else
        return (uint32_t)__builtin_popcountll(w);
#endif
    }
};
struct NonZeroByte {
    __host__ __device__ uint32_t operator()(uint8_t v) const { return v != 0; }
};

thread_local double g_vac_stats[4];

__global__ void __launch_bounds__(WG_THREADS) doc_deleted_kernel(TapeView docs, uint32_t n_docs, unsigned long long *words, unsigned long long *err) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p64 = ((uint64_t)blockIdx.x * WG_THREADS + threadIdx.x) >> 6;
    if (p64 >= docs.n_pages) return;  // (whole waves)
    const uint32_t p = (uint32_t)p64, base = docs.pre[p], n = docs.pre[p + 1] - base;
    for (uint32_t r = 0; r < n; r += 64) {  // every lane of the wave takes every round: the ballot reads them all
        const uint32_t i = r + lane;
        bool deleted = false;
        if (i < n) {
            if (const uint32_t reason = doc_deleted_lane(docs, p, i, deleted)) atomicMin(err, (unsigned long long)error_key(T_DOCS, (uint64_t)base + i, reason));
            // a tape longer than Jump's count is refused by the caller: its surplus tuples have no bit
            if ((uint64_t)base + i >= n_docs) deleted = false;
        }
        const unsigned long long m = __ballot(deleted);
        if (!m) continue;
        const uint64_t first = (uint64_t)base + r;  // the document of lane 0; every set bit of m is a document < n_docs
        uint64_t lo, hi;
        flag_round_words(first, m, lo, hi);
        if (lane == 0 && lo) atomicOr(words + (first >> 6), (unsigned long long)lo);
        if (lane == 1 && hi) atomicOr(words + (first >> 6) + 1, (unsigned long long)hi);
    }
}

const char *doc_reason_text(uint32_t r) { return r == R_TUPLE_SHORT ? "document tuple too short" : reason_text(r); }

int vacuum_from_pages_impl(vbm25_index *index, vbm25_read_page_fn read_page, void *ctx, vbm25_device_vacuum **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!index || !read_page) return set_error(VBM25_ERR_INVALID, "NULL argument");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: the device reader has no CPU fallback (vbm25_sealed_deleted_from_pages and "
                                           "vbm25_growing_from_pages are the host readers)");
    int device = 0;
    uint32_t sealed_docs = 0;
    if (int rc = index_device_and_docs(index, &device, &sealed_docs)) return rc;
    HIP_TRY(hipSetDevice(device));
    for (double &x : g_vac_stats) x = 0.0;

    Stream stream;
    HIP_TRY(stream.create());
    hipStream_t s = stream.s;
    auto dv = std::make_unique<vbm25_device_vacuum>();  // (before the stager: its planes go last)
    dv->device = device;
    Stager st;
    if (int rc = st.init(s)) return rc;

    // ---- the host pass over the documents tape.  A refusal of the walk is held back until the lanes have looked at the pages in
    // front of it: the host reader meets their tuples first
    Walk w;
    const uint8_t *j = read_meta_jump(read_page, ctx, w);
    if (!j) return corrupt(w.what, w.bad_page);
    const uint32_t ptr_vectors = host_rd32(j), ptr_documents = host_rd32(j + 44), n_docs = w.n_docs;
    int sink_rc = 0;
    std::unordered_set<uint32_t> seen;
    const bool walked = walk_tape_pages(read_page, ctx, w, T_DOCS, ptr_documents, seen,
                                        [&](uint32_t tape, uint32_t, const uint8_t *image) { return st.add(tape, image); }, sink_rc, true);
    int rc = !walked && sink_rc ? sink_rc : st.flush();
    if (rc) {
        (void)hipStreamSynchronize(s);  // nothing is freed under a copy in flight
        return rc;
    }
    const size_t np = w.pid[T_DOCS].size();
    const uint32_t W = (uint32_t)(((uint64_t)n_docs + 63u) / 64u);
    uint64_t bytes_down = 0;

    // ---- the flags.  From here on a failure returns through the buffers' destructors (hipFree waits for the device)
    float ms_flags = 0;
    {
        HbmArray d_chunk, d_pre, d_err, d_cnt, d_tmp;
        std::vector<const uint8_t *> chunk_ptr;
        for (const auto &d : st.chunks[T_DOCS]) chunk_ptr.push_back(d->as<uint8_t>());
        HIP_TRY(d_chunk.alloc(sizeof(void *) * chunk_ptr.size()));
        HIP_TRY(d_pre.alloc(4 * (np + 1)));
        HIP_TRY(d_err.alloc(8));
        HIP_TRY(d_cnt.alloc(4));
        HIP_TRY(dv->d_sealed_deleted.alloc(8ull * W));
        if (np) HIP_TRY(hipMemcpyAsync(d_chunk.p, chunk_ptr.data(), sizeof(void *) * chunk_ptr.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pre.p, w.pre[T_DOCS].data(), 4 * (np + 1), hipMemcpyHostToDevice, s));
        st.bytes_up += 8 * chunk_ptr.size() + 4 * (np + 1);
        Event ev[2];
        for (Event &e : ev) HIP_TRY(e.create());
        HIP_TRY(hipEventRecord(ev[0].e, s));
        HIP_TRY(hipMemsetAsync(d_err.p, 0xff, 8, s));
        HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 4, s));
        HIP_TRY(hipMemsetAsync(dv->d_sealed_deleted.p, 0, W ? 8ull * W : 16, s));
        const TapeView docs{d_chunk.as<const uint8_t *>(), nullptr, d_pre.as<uint32_t>(), (uint32_t)np, w.pre[T_DOCS].back()};
        if (np && docs.n_tuples)
            doc_deleted_kernel<<<(uint32_t)((np + 3) / 4), WG_THREADS, 0, s>>>(docs, n_docs, dv->d_sealed_deleted.as<unsigned long long>(),
                                                                               d_err.as<unsigned long long>());
        if (W) {
            hipcub::TransformInputIterator<uint32_t, PopCount64, const unsigned long long *> pop(dv->d_sealed_deleted.as<unsigned long long>(), PopCount64());
            HIP_TRY(with_cub_temp(d_tmp, [&](void *t, size_t &tb) { return hipcub::DeviceReduce::Sum(t, tb, pop, d_cnt.as<uint32_t>(), (int)W, s); }));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[1].e, s));
        unsigned long long key = 0;
        HIP_TRY(hipMemcpyAsync(&key, d_err.p, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&dv->n_sealed_deleted, d_cnt.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        bytes_down += 12;
        // ---- the verdict on the documents tape, in vbm25_sealed_deleted_from_pages' order
        if (key != NO_ERROR) return corrupt(doc_reason_text(key_reason(key)), error_page(w, key));
        if (!walked) return corrupt(w.what, w.bad_page);
        if (w.pre[T_DOCS].back() != n_docs) return corrupt("document count differs from the Jump tuple", ptr_documents);
        HIP_TRY(hipEventElapsedTime(&ms_flags, ev[0].e, ev[1].e));
    }
    st.chunks[T_DOCS].clear();  // (synchronised above: the documents tape's images are done with)
    dv->n_sealed = n_docs;

    // ---- the vectors tape, into the handle's planes
    VecCsr v;
    v.start = &dv->d_start, v.key = &dv->d_key, v.tf = &dv->d_tf, v.fieldnorm = &dv->d_fieldnorm, v.deleted = &dv->d_deleted, v.payload = &dv->d_payload;
    if (int rc2 = vectors_csr(s, st, 1, read_page, ctx, &ptr_vectors, sealed_docs, v)) return rc2;
    dv->n_grow = v.n_docs;
    dv->n_elements = v.n_el;
    if (v.n_docs) {
        HbmArray d_cnt, d_tmp;
        HIP_TRY(d_cnt.alloc(4));
        hipcub::TransformInputIterator<uint32_t, NonZeroByte, const uint8_t *> nz(dv->d_deleted.as<uint8_t>(), NonZeroByte());
        HIP_TRY(with_cub_temp(d_tmp, [&](void *t, size_t &tb) { return hipcub::DeviceReduce::Sum(t, tb, nz, d_cnt.as<uint32_t>(), (int)v.n_docs, s); }));
        HIP_TRY(hipMemcpyAsync(&dv->n_grow_deleted, d_cnt.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        bytes_down += 4;
    }
    if (n_docs != sealed_docs)
        return set_error(VBM25_ERR_INVALID, "the relation holds %u sealed documents, the index %u: the index of another relation", n_docs, sealed_docs);
    g_vac_stats[0] = (double)ms_flags + v.kernel_ms;
    g_vac_stats[1] = (double)st.bytes_up;
    g_vac_stats[2] = (double)(bytes_down + v.bytes_down);
    g_vac_stats[3] = (double)v.n_el;
    *out = dv.release();
    return VBM25_OK;
}

int vacuum_read_impl(const vbm25_device_vacuum *v, uint64_t *sealed_deleted_words, uint8_t *growing_deleted) {
    if (!v) return set_error(VBM25_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(v->device));
    const uint64_t W = ((uint64_t)v->n_sealed + 63u) / 64u;
    if (sealed_deleted_words && W) HIP_TRY(hipMemcpy(sealed_deleted_words, v->d_sealed_deleted.p, 8ull * W, hipMemcpyDeviceToHost));
    if (growing_deleted && v->n_grow) HIP_TRY(hipMemcpy(growing_deleted, v->d_deleted.p, v->n_grow, hipMemcpyDeviceToHost));
    return VBM25_OK;
}

}  // namespace

extern "C" int vbm25_device_segment_from_pages(vbm25_read_page_fn read_page, void *ctx, int device, vbm25_device_segment **out) {
    return vbm25::guarded([&] { return from_pages_impl(read_page, ctx, device, out); });
}

// The last successful vbm25_device_segment_from_pages of this thread (tools/pages_device_cost.py; not part of the ABI): [0] ms of the
// kernels and scans between HIP events, [1] bytes host -> device, [2] bytes device -> host, [3] bytes of host memory the call
// allocated (pinned staging, the per-page tables, the segment's host members)
extern "C" int vbm25_debug_pages_device_stats(double *out4) {
    if (!out4) return vbm25::set_error(VBM25_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) out4[i] = g_stats[i];
    return VBM25_OK;
}

extern "C" int vbm25_device_growing_from_pages(vbm25_index *index, vbm25_read_page_fn read_page, void *ctx, vbm25_device_growing **out,
                                               vbm25_growing **csr) {
    return vbm25::guarded([&] { return growing_from_pages_impl(index, read_page, ctx, out, csr); });
}

// The last successful vbm25_device_growing_from_pages of this thread (tools/growing_pages_cost.py; not part of the ABI): [0] ms of the
// reader's kernels and scans between HIP events (the segment's build behind them is vbm25_growing_upload's), [1] bytes host ->
// device, [2] bytes device -> host, [3] elements read
extern "C" int vbm25_debug_growing_pages_stats(double *out4) {
    if (!out4) return vbm25::set_error(VBM25_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) out4[i] = g_vec_stats[i];
    return VBM25_OK;
}

extern "C" int vbm25_device_vacuum_from_pages(vbm25_index *index, vbm25_read_page_fn read_page, void *ctx, vbm25_device_vacuum **out) {
    return vbm25::guarded([&] { return vacuum_from_pages_impl(index, read_page, ctx, out); });
}
extern "C" int vbm25_device_vacuum_info(const vbm25_device_vacuum *v, uint32_t *n_sealed, uint32_t *n_sealed_deleted, uint32_t *n_grow,
                                        uint32_t *n_grow_deleted, uint64_t *n_elements) {
    if (!v) return vbm25::set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_sealed) *n_sealed = v->n_sealed;
    if (n_sealed_deleted) *n_sealed_deleted = v->n_sealed_deleted;
    if (n_grow) *n_grow = v->n_grow;
    if (n_grow_deleted) *n_grow_deleted = v->n_grow_deleted;
    if (n_elements) *n_elements = v->n_elements;
    return VBM25_OK;
}
extern "C" int vbm25_device_vacuum_read(const vbm25_device_vacuum *v, uint64_t *sealed_deleted_words, uint8_t *growing_deleted) {
    return vbm25::guarded([&] { return vacuum_read_impl(v, sealed_deleted_words, growing_deleted); });
}
extern "C" void vbm25_device_vacuum_free(vbm25_device_vacuum *v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    delete v;
}

// The last successful vbm25_device_vacuum_from_pages of this thread (tools/vacuum_device_cost.py; not part of the ABI): [0] ms of the
// reader's kernels, scans and reductions between HIP events, [1] bytes host -> device, [2] bytes device -> host, [3] elements read
extern "C" int vbm25_debug_vacuum_pages_stats(double *out4) {
    if (!out4) return vbm25::set_error(VBM25_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) out4[i] = g_vac_stats[i];
    return VBM25_OK;
}
