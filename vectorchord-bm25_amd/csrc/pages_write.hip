// pages_write.hip -- the device writer: a sealed segment in HBM -> the page images flush.rs:40-158 writes for it
// (vbm25_device_segment_page_count, vbm25_device_segment_write_pages, vbm25_device_segment_write_relation).  The inverse of
// pages_device.hip; pages_emit.h holds every per-page and per-tuple function, the kernels here are loops over them.
//
//   layout   documents, tokens, summaries: 680, 226, 291 tuples a page.  Blocks (tuples of 32 .. 1040 bytes, packed greedily):
//     (scan)           cost[j] = the costs align8(len) + 4 of the block tuples in front of j, in 64 bits (hipcub)
//     next_kernel      one thread per block: the block a page ends in front of if it begins here (a search over <= 226 prefix sums)
//     double_kernel    log2(pages) rounds: page_start[k + 2^r] = next^(2^r)(page_start[k]) for k < 2^r, and next^(2^(r + 1)) for
//                      every block -- the orbit of block 0, which is the first block of every page
//     count_kernel     the orbit's length (4 bytes go down: the host sizes the call with it)
//     ids_kernel       one thread per page of the three interleaved tapes: its rank in the allocation order (its own index plus two
//                      binary searches) -> its page id
//   fill     fill_kernel<tape>, one wave per page of a chunk of 1024 images: header, line pointers, tuples from the top down, zeros,
//            next; block bodies from the blob 16 lanes a tuple.  Every 8-byte word of an image is stored exactly once.
//   host     a chunk and its 1024 page ids come down into one of two pinned buffers while the callbacks of the chunk before run;
//            then the two address trees (one id per documents page, one key -- from the segment's host keys -- and one id per tokens
//            page) are assembled and handed out.  The keys go UP once (16 bytes a token: the segment keeps them on the host only);
//            no per-document, per-term or per-block array comes down.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "pages_emit.h"

namespace {

using namespace vbm25;
using namespace vbm25::pge;

// the last call's cost on this thread (vbm25_debug_pages_write_stats)
thread_local double g_stats[6];

constexpr uint32_t WG_THREADS = 256, MAX_GRID = 2048;

struct CostOf {
    const uint8_t *n, *md, *mt;
    __host__ __device__ unsigned long long operator()(uint32_t j) const { return block_cost(n, md, mt, j); }
};

__global__ void __launch_bounds__(WG_THREADS) next_kernel(const unsigned long long *cost, uint32_t n, uint32_t *next) {
    for (uint32_t j = blockIdx.x * WG_THREADS + threadIdx.x; j <= n; j += gridDim.x * WG_THREADS) next[j] = j < n ? next_start(cost, n, j) : n;
}

// jump = next^have, page_start[0 .. have) known: the orbit's next `have` entries (below cap) and jump2 = next^(2 have)
__global__ void __launch_bounds__(WG_THREADS) double_kernel(const uint32_t *jump, uint32_t *jump2, uint32_t n, uint32_t *page_start, uint32_t have,
                                                            uint32_t cap) {
    const uint32_t units = n + 1 > have ? n + 1 : have;
    for (uint32_t t = blockIdx.x * WG_THREADS + threadIdx.x; t < units; t += gridDim.x * WG_THREADS) {
        if (t < have && t + have < cap) page_start[t + have] = jump[page_start[t]];
        if (t <= n && jump2) jump2[t] = jump[jump[t]];
    }
}

// page_start ascends to n and stays there: the entries below n are the pages
__global__ void __launch_bounds__(WG_THREADS) count_kernel(const uint32_t *page_start, uint32_t cap, uint32_t n, uint32_t *n_pages) {
    for (uint32_t k = blockIdx.x * WG_THREADS + threadIdx.x; k + 1 < cap; k += gridDim.x * WG_THREADS)
        if (page_start[k] < n && page_start[k + 1] >= n) *n_pages = k + 1;
}

__global__ void __launch_bounds__(WG_THREADS) ids_kernel(Emit c, uint32_t units) {
    for (uint32_t u = blockIdx.x * WG_THREADS + threadIdx.x; u < units; u += gridDim.x * WG_THREADS) page_ids_lane(c, u);
}

// one wave per page: pages [p0, p0 + np) of tape TAPE into out (np images) and their ids into pid_out
template <uint32_t TAPE>
__global__ void __launch_bounds__(WG_THREADS) fill_kernel(Emit c, uint32_t p0, uint32_t np, uint64_t *out, uint32_t *pid_out) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * WG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WG_THREADS) >> 6;
    for (uint32_t i = wave; i < np; i += n_waves) {
        fill_page<TAPE>(c, p0 + i, out + (size_t)i * WORDS, lane, 64);
        if (lane == 0) pid_out[i] = tape_page_id(c, TAPE, p0 + i);
    }
}

int callback_error(uint32_t page, int rc) { return set_error(VBM25_ERR_INVALID, "write_page returned %d for page %u: the write stopped there", rc, page); }

struct Sink {
    vbm25_write_page_fn fn;
    void *ctx;
    uint64_t pages = 0;
    int operator()(uint32_t id, const uint8_t *image) {
        ++pages;
        if (const int rc = fn(ctx, id, image)) return callback_error(id, rc);
        return VBM25_OK;
    }
};

// count_only: *count and nothing else.  relation: the allocator is sequential from page 1 and the four pages of build.rs follow.
int write_impl(const vbm25_device_segment *seg, const uint32_t *page_ids, uint32_t n_page_ids, uint32_t first_page, vbm25_write_page_fn fn,
               void *ctx, vbm25_flushed *flushed, bool count_only, uint32_t *count) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(VBM25_ERR_DEVICE, "no HIP device: the device writer has no CPU fallback");
    if (seg->device < 0 || seg->device >= n_dev) return set_error(VBM25_ERR_INVALID, "device %d out of range (%d devices)", seg->device, n_dev);
    HIP_TRY(hipSetDevice(seg->device));
    for (double &x : g_stats) x = 0.0;

    Stream stream;
    HIP_TRY(stream.create());
    hipStream_t s = stream.s;
    HbmArray d_cost, d_jump[2], d_start, d_count, d_tmp, d_ids, d_key, d_tok_pid, d_sum_pid, d_blk_pid, d_img, d_pid;
    PinnedHost pin[2];
    Event ev_layout[2], ev[2][3];  // ev, per staging buffer: fill begins, fill ends, copies end
    Quiesce quiesce{s};
    for (Event &e : ev_layout) HIP_TRY(e.create());

    const uint32_t n_docs = seg->n_docs, n_terms = seg->n_terms, n = seg->n_blocks;
    Emit c{};
    c.n_docs = n_docs;
    c.n_terms = n_terms;
    c.n_blocks = n;
    c.n_pages[T_DOCS] = pages_for(n_docs, DOCS_PER_PAGE);
    c.n_pages[T_TOKENS] = pages_for(n_terms, TOKENS_PER_PAGE);
    c.n_pages[T_SUMMARIES] = pages_for(n, SUMMARIES_PER_PAGE);
    c.n_pages[T_BLOCKS] = 1;
    c.doc_fieldnorm = seg->d_doc_fieldnorm.as<uint8_t>();
    c.doc_payload = seg->d_doc_payload.as<uint16_t>();
    c.term_wand_fn = seg->d_term_wand_fn.as<uint8_t>();
    c.term_wand_tf = seg->d_term_wand_tf.as<uint32_t>();
    c.term_df = seg->d_term_df.as<uint32_t>();
    c.term_first_block = seg->d_term_first_block.as<uint32_t>();
    c.blk_min = seg->d_blk_min.as<uint32_t>();
    c.blk_max = seg->d_blk_max.as<uint32_t>();
    c.blk_wand_tf = seg->d_blk_wand_tf.as<uint32_t>();
    c.blk_n = seg->d_blk_n.as<uint8_t>();
    c.blk_wand_fn = seg->d_blk_wand_fn.as<uint8_t>();
    c.blk_meta_doc = seg->d_blk_meta_doc.as<uint8_t>();
    c.blk_meta_tf = seg->d_blk_meta_tf.as<uint8_t>();
    c.off8 = seg->d_blk_off8.as<uint32_t>();
    c.blob = seg->d_blob.as<uint8_t>();

    // ---- the blocks tape's page breaks
    const uint32_t cap = n / MIN_BLOCKS_PER_PAGE + 2;  // a page that is not the last holds at least MIN_BLOCKS_PER_PAGE tuples
    HIP_TRY(d_cost.alloc(8ull * (n + 1ull)));
    HIP_TRY(d_start.alloc(4ull * cap));
    HIP_TRY(hipEventRecord(ev_layout[0].e, s));
    HIP_TRY(hipMemsetAsync(d_cost.p, 0, 8, s));
    HIP_TRY(hipMemsetAsync(d_start.p, 0, 4ull * cap, s));  // n == 0: {0, 0}
    if (n) {
        HIP_TRY(d_jump[0].alloc(4ull * (n + 1ull)));
        HIP_TRY(d_jump[1].alloc(4ull * (n + 1ull)));
        HIP_TRY(d_count.alloc(4));
        HIP_TRY(hipMemsetAsync(d_count.p, 0, 4, s));
        hipcub::CountingInputIterator<uint32_t> idx(0);
        hipcub::TransformInputIterator<unsigned long long, CostOf, hipcub::CountingInputIterator<uint32_t>> costs(idx, CostOf{c.blk_n, c.blk_meta_doc, c.blk_meta_tf});
        HIP_TRY(with_cub_temp(d_tmp, [&](void *t, size_t &tb) { return hipcub::DeviceScan::InclusiveSum(t, tb, costs, d_cost.as<unsigned long long>() + 1, (int)n, s); }));
        next_kernel<<<grid_for(n + 1ull, WG_THREADS, MAX_GRID), WG_THREADS, 0, s>>>(d_cost.as<unsigned long long>(), n, d_jump[0].as<uint32_t>());
        int cur = 0;
        for (uint64_t have = 1; have < cap; have *= 2, cur ^= 1) {
            const bool last = 2 * have >= cap;
            double_kernel<<<grid_for(std::max<uint64_t>(n + 1ull, have), WG_THREADS, MAX_GRID), WG_THREADS, 0, s>>>(
                d_jump[cur].as<uint32_t>(), last ? nullptr : d_jump[cur ^ 1].as<uint32_t>(), n, d_start.as<uint32_t>(), (uint32_t)have, cap);
        }
        count_kernel<<<grid_for(cap, WG_THREADS, MAX_GRID), WG_THREADS, 0, s>>>(d_start.as<uint32_t>(), cap, n, d_count.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        uint32_t b = 0;
        HIP_TRY(hipMemcpyAsync(&b, d_count.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (b == 0) return set_error(VBM25_ERR_CORRUPT, "the blocks tape's page breaks did not close: the segment's block metadata is inconsistent");
        c.n_pages[T_BLOCKS] = b;
    }
    c.cost = d_cost.as<unsigned long long>();
    c.page_start = d_start.as<uint32_t>();
    const uint64_t total = flush_pages(c.n_pages, n_docs, n_terms);
    if (total + 4 > 0xffffffffull) return set_error(VBM25_ERR_UNSUPPORTED, "%llu pages: more than a relation holds", (unsigned long long)total);
    *count = (uint32_t)total;
    if (count_only) return VBM25_OK;

    // ---- the page ids
    uint64_t bytes_up = 0, bytes_down = 4;
    if (page_ids) {
        if (n_page_ids != total) return set_error(VBM25_ERR_INVALID, "%u page ids for a segment of %llu pages", n_page_ids, (unsigned long long)total);
        std::vector<uint32_t> sorted(page_ids, page_ids + n_page_ids);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.back() == NONE) return set_error(VBM25_ERR_INVALID, "page id 0xFFFFFFFF is not a page");
        for (size_t i = 1; i < sorted.size(); ++i)
            if (sorted[i] == sorted[i - 1]) return set_error(VBM25_ERR_INVALID, "page id %u is given twice", sorted[i]);
        HIP_TRY(d_ids.alloc(4ull * total));
        HIP_TRY(hipMemcpyAsync(d_ids.p, page_ids, 4ull * total, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));  // the caller's array is pageable
        bytes_up += 4ull * total;
        c.page_ids = d_ids.as<uint32_t>();
    } else if ((uint64_t)first_page + total > 0xffffffffull) {
        return set_error(VBM25_ERR_INVALID, "first_page %u + %llu pages reach beyond page id 2^32 - 2", first_page, (unsigned long long)total);
    }
    c.first_page = first_page;
    auto id_of = [&](uint32_t alloc) { return page_ids ? page_ids[alloc] : first_page + alloc; };
    HIP_TRY(d_key.alloc(16ull * n_terms));
    if (n_terms) {
        HIP_TRY(hipMemcpyAsync(d_key.p, seg->term_key.data(), 16ull * n_terms, hipMemcpyHostToDevice, s));
        bytes_up += 16ull * n_terms;
    }
    c.term_key = d_key.as<uint8_t>();
    HIP_TRY(d_tok_pid.alloc(4ull * c.n_pages[T_TOKENS]));
    HIP_TRY(d_sum_pid.alloc(4ull * c.n_pages[T_SUMMARIES]));
    HIP_TRY(d_blk_pid.alloc(4ull * c.n_pages[T_BLOCKS]));
    c.tok_pid = d_tok_pid.as<uint32_t>();
    c.sum_pid = d_sum_pid.as<uint32_t>();
    c.blk_pid = d_blk_pid.as<uint32_t>();
    const uint32_t id_units = std::max(c.n_pages[T_BLOCKS], std::max(c.n_pages[T_SUMMARIES], c.n_pages[T_TOKENS]));
    ids_kernel<<<grid_for(id_units, WG_THREADS, MAX_GRID), WG_THREADS, 0, s>>>(c, id_units);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev_layout[1].e, s));

    // ---- the images, a chunk at a time: chunk i's callbacks run while chunk i + 1 is filled and copied
    constexpr size_t IMG_BYTES = (size_t)CHUNK_PAGES * BLCKSZ, PID_BYTES = 4ull * CHUNK_PAGES;
    HIP_TRY(d_img.alloc(IMG_BYTES));
    HIP_TRY(d_pid.alloc(PID_BYTES));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(pin[i].alloc(IMG_BYTES + PID_BYTES));
        for (Event &e : ev[i]) HIP_TRY(e.create());
    }
    Sink sink{fn, ctx};
    std::vector<uint32_t> tok_pid(c.n_pages[T_TOKENS]);
    double fill_ms = 0, copy_ms = 0;
    struct Pending {
        int buf = -1;
        uint32_t tape = 0, p0 = 0, np = 0;
    } pending;
    auto drain = [&]() -> int {
        if (pending.buf < 0) return VBM25_OK;
        Event *e = ev[pending.buf];
        HIP_TRY(hipEventSynchronize(e[2].e));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, e[0].e, e[1].e));
        HIP_TRY(hipEventElapsedTime(&b, e[1].e, e[2].e));
        fill_ms += a;
        copy_ms += b;
        const uint8_t *img = static_cast<const uint8_t *>(pin[pending.buf].p);
        const uint32_t *ids = reinterpret_cast<const uint32_t *>(img + IMG_BYTES);
        if (pending.tape == T_TOKENS) std::copy(ids, ids + pending.np, tok_pid.begin() + pending.p0);
        pending.buf = -1;
        for (uint32_t i = 0; i < pending.np; ++i)
            if (int rc = sink(ids[i], img + (size_t)i * BLCKSZ)) return rc;
        return VBM25_OK;
    };
    int buf = 0;
    for (uint32_t tape = 0; tape < N_TAPES; ++tape)
        for (uint32_t p0 = 0; p0 < c.n_pages[tape]; p0 += CHUNK_PAGES, buf ^= 1) {
            const uint32_t np = std::min(CHUNK_PAGES, c.n_pages[tape] - p0), grid = grid_for(np, WG_THREADS / 64, MAX_GRID);
            uint64_t *out = d_img.as<uint64_t>();
            uint32_t *pid_out = d_pid.as<uint32_t>();
            HIP_TRY(hipEventRecord(ev[buf][0].e, s));
            if (tape == T_DOCS) fill_kernel<T_DOCS><<<grid, WG_THREADS, 0, s>>>(c, p0, np, out, pid_out);
            else if (tape == T_TOKENS) fill_kernel<T_TOKENS><<<grid, WG_THREADS, 0, s>>>(c, p0, np, out, pid_out);
            else if (tape == T_SUMMARIES) fill_kernel<T_SUMMARIES><<<grid, WG_THREADS, 0, s>>>(c, p0, np, out, pid_out);
            else fill_kernel<T_BLOCKS><<<grid, WG_THREADS, 0, s>>>(c, p0, np, out, pid_out);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ev[buf][1].e, s));
            uint8_t *h = static_cast<uint8_t *>(pin[buf].p);
            HIP_TRY(hipMemcpyAsync(h, d_img.p, (size_t)np * BLCKSZ, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(h + IMG_BYTES, d_pid.p, 4ull * np, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(ev[buf][2].e, s));
            bytes_down += (uint64_t)np * (BLCKSZ + 4);
            if (int rc = drain()) return rc;
            pending.buf = buf;
            pending.tape = tape;
            pending.p0 = p0;
            pending.np = np;
        }
    if (int rc = drain()) return rc;

    // ---- the address trees
    const uint32_t alloc = c.n_pages[T_DOCS] + c.n_pages[T_TOKENS] + c.n_pages[T_SUMMARIES] + c.n_pages[T_BLOCKS];
    vbm25_flushed f;
    if (int rc = address_tapes(c.n_pages, n_docs, n_terms, seg->sum_len, seg->term_key.data(), tok_pid.data(), alloc, id_of, sink, &f)) return rc;
    if (sink.pages != total) return set_error(VBM25_ERR_INVALID, "internal error: %llu pages written, %llu counted", (unsigned long long)sink.pages, (unsigned long long)total);
    *flushed = f;
    float layout_ms = 0;
    HIP_TRY(hipEventElapsedTime(&layout_ms, ev_layout[0].e, ev_layout[1].e));
    g_stats[0] = layout_ms;
    g_stats[1] = fill_ms;
    g_stats[2] = copy_ms;
    g_stats[3] = (double)bytes_down;
    g_stats[4] = (double)bytes_up;
    g_stats[5] = (double)total;
    return VBM25_OK;
}

}  // namespace

extern "C" int vbm25_device_segment_page_count(const vbm25_device_segment *seg, uint32_t *n_pages) {
    return vbm25::guarded([&]() -> int {
        if (!seg || !n_pages) return vbm25::set_error(VBM25_ERR_INVALID, "NULL argument");
        return write_impl(seg, nullptr, 0, 0, nullptr, nullptr, nullptr, true, n_pages);
    });
}

extern "C" int vbm25_device_segment_write_pages(const vbm25_device_segment *seg, const uint32_t *page_ids, uint32_t n_page_ids, uint32_t first_page,
                                                vbm25_write_page_fn write_page, void *ctx, vbm25_flushed *out) {
    return vbm25::guarded([&]() -> int {
        if (!seg || !write_page || !out) return vbm25::set_error(VBM25_ERR_INVALID, "NULL argument");
        uint32_t count = 0;
        return write_impl(seg, page_ids, n_page_ids, first_page, write_page, ctx, out, false, &count);
    });
}

extern "C" int vbm25_device_segment_write_relation(const vbm25_device_segment *seg, const uint8_t *seed32, vbm25_write_page_fn write_page, void *ctx,
                                                   uint32_t *n_pages) {
    return vbm25::guarded([&]() -> int {
        if (n_pages) *n_pages = 0;
        if (!seg || !write_page) return vbm25::set_error(VBM25_ERR_INVALID, "NULL argument");
        uint32_t count = 0;
        vbm25_flushed f;
        if (int rc = write_impl(seg, nullptr, 0, 1, write_page, ctx, &f, false, &count)) return rc;
        Sink sink{write_page, ctx};
        if (int rc = fixed_pages(f, count, seg->k1, seg->b, seed32, sink)) return rc;
        if (n_pages) *n_pages = count + 4;
        return VBM25_OK;
    });
}

// The last successful write of this thread (tools/pages_write_cost.py; not part of the ABI): [0] ms of the layout kernels and scans,
// [1] ms of the fill kernels, [2] ms of the copies to the host (HIP events; the copies of a chunk wait behind nothing but its fill),
// [3] bytes device -> host, [4] bytes host -> device, [5] pages
extern "C" int vbm25_debug_pages_write_stats(double *out6) {
    if (!out6) return vbm25::set_error(VBM25_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 6; ++i) out6[i] = g_stats[i];
    return VBM25_OK;
}
