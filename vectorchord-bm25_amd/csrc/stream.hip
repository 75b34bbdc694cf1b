// stream.hip -- vbm25_stream, the pipelined ring of batch objects, and what an idle batch takes on with its next query set
// (batch_attach_check, batch_attach: a ring slot here, a shard in multi.hip).  No kernel of its own.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "vbm25_internal.h"
#include "host_objects.h"
#include "ring.h"

// ---------------------------------------------------------------------------
// The pipelined boundary (include/vbm25.h): a ring of batch objects, each with its own stream and pinned staging.  submit =
// set_queries (staged) + run, enqueued on the slot's stream; merge_kernel writes the counts and the 24-byte records straight into
// the slot's pinned output buffer (pinned_results: posted writes over PCIe -- no download command on the step, only the 4-byte
// flag is copied); collect = the oldest slot's stream synchronisation and one copy out of its pinned buffer.  The kernels of
// neighbouring batches are launched into each other's tails: on C3 a pipelined step is SHORTER than a step of a loop over resident
// batches on one stream (0.21 against 0.235 ms, profiles/r5_stream_host_time.txt).  With the records downloaded by copy
// commands (three per batch) the same ring took 0.25 ms.
// ---------------------------------------------------------------------------
struct vbm25_stream {
    std::vector<vbm25_batch *> slots;
    vbm25::RingCursor ring;  // over the slots: ring.count batches are in flight
    vbm25_index *index = nullptr;
    // what the next submit takes (vbm25_stream_set_growing / _set_filter): a slot picks them up when it is idle, at its next submit --
    // the batches in flight keep what they were submitted with, and the setters wait for nobody
    const vbm25_device_growing *growing = nullptr;
    const vbm25_filter *filter = nullptr;
    ~vbm25_stream() {
        for (vbm25_batch *b : slots) vbm25_batch_destroy(b);
    }
};

namespace vbm25 {

// An idle batch (a ring slot, a shard) takes the segment, the filter and the selectors of its next query set: sel = nq selectors that
// go up with the queries in the staged block (k > 1024: read on the host), NULL or all UINT32_MAX = no filter.  The pairing rules of
// vbm25_batch_set_filter / _set_growing, checked before anything changes; no copy, no synchronisation.
int batch_attach_check(const vbm25_batch *b, const vbm25_device_growing *gs, const vbm25_filter *f, const uint32_t *sel, uint32_t nq,
                       bool *on_out) {
    if (gs && gs->index != b->index) return set_error(VBM25_ERR_INVALID, "the growing segment belongs to another index");
    if (f && f->index != b->index) return set_error(VBM25_ERR_INVALID, "the filter belongs to another index");
    bool on = false;
    if (f && sel)
        if (int rc = filter_selector_check(f, sel, nq, &on)) return rc;
    if (on && gs) {
        if (!f->grow_serial) return set_error(VBM25_ERR_UNSUPPORTED, "a growing segment is attached and the filter has no growing bitmaps");
        if (f->grow_serial != gs->serial)
            return set_error(VBM25_ERR_INVALID, "the filter's growing bitmaps belong to another upload than the attached growing segment");
        if (int rc = filter_growing_count_check(f, gs)) return rc;
    }
    *on_out = on;
    return VBM25_OK;
}
int batch_attach(vbm25_batch *b, const vbm25_device_growing *gs, const vbm25_filter *f, const uint32_t *sel, uint32_t nq, bool on) {
    if (gs) {
        if (int rc = use_device(b->device)) return rc;
        if (int rc = batch_growing_buffers(b, gs)) {
            b->growing = nullptr;
            return rc;
        }
    }
    b->growing = gs;
    b->filter = on ? f : nullptr;
    b->filt_on = on;
    b->stage_sel = on ? sel : nullptr;
    if (on && b->bigk) {
        b->h_filt_sel.assign(b->max_queries, UINT32_MAX);
        std::copy(sel, sel + nq, b->h_filt_sel.begin());
    }
    return VBM25_OK;
}
// set_queries (staged) + run + the flag's download, on the batch's own stream
static int batch_submit(vbm25_batch *b, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq) {
    const bool fast = !b->bigk;
    const int rcq = vbm25_batch_set_queries_impl(b, term_ids, q_off, nq, fast);
    b->stage_sel = nullptr;
    if (rcq) return rcq;
    void *st = fast ? b->lat_stream : nullptr;
    if (int rc = b->growing ? batch_run_growing_impl(b, st) : vbm25_batch_run_impl(b, st)) return rc;
    return vbm25_batch_enqueue_download(b);
}

static int stream_create_impl(vbm25_index *ix, uint32_t depth, uint32_t max_queries, uint32_t max_total_terms, uint32_t k, vbm25_stream **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ix) return set_error(VBM25_ERR_INVALID, "index is NULL");
    if (depth == 0 || depth > 16) return set_error(VBM25_ERR_INVALID, "depth must be 1..16");
    auto s = std::make_unique<vbm25_stream>();
    for (uint32_t i = 0; i < depth; ++i) {
        vbm25_batch *b = nullptr;
        if (int rc = vbm25_batch_create(ix, max_queries, std::max(max_total_terms, 1u), k, &b)) return rc;
        b->pinned_results = true;
        s->slots.push_back(b);
    }
    s->ring.depth = depth;
    s->index = ix;
    *out = s.release();
    return VBM25_OK;
}
static int stream_set_growing_impl(vbm25_stream *s, const vbm25_device_growing *gs) {
    if (!s) return set_error(VBM25_ERR_INVALID, "stream is NULL");
    if (gs && gs->index != s->index) return set_error(VBM25_ERR_INVALID, "the growing segment belongs to another index");
    s->growing = gs;
    return VBM25_OK;
}
static int stream_set_filter_impl(vbm25_stream *s, const vbm25_filter *f) {
    if (!s) return set_error(VBM25_ERR_INVALID, "stream is NULL");
    if (f && f->index != s->index) return set_error(VBM25_ERR_INVALID, "the filter belongs to another index");
    s->filter = f;
    return VBM25_OK;
}
static int stream_submit_impl(vbm25_stream *s, bool filtered, const uint32_t *q_filter, const uint32_t *term_ids, const uint32_t *q_off,
                              uint32_t nq) {
    if (!s || !q_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (s->ring.full()) return set_error(VBM25_ERR_INVALID, "%u batches in flight: collect one first", s->ring.count);
    if (filtered && !s->filter) return set_error(VBM25_ERR_INVALID, "the stream has no filter set");
    if (filtered && !q_filter && nq) return set_error(VBM25_ERR_INVALID, "q_filter is NULL");
    vbm25_batch *b = s->slots[s->ring.tail()];
    if (nq > b->max_queries) return set_error(VBM25_ERR_INVALID, "%u queries exceed the batch capacity %u", nq, b->max_queries);
    bool on = false;
    if (int rc = batch_attach_check(b, s->growing, filtered ? s->filter : nullptr, q_filter, nq, &on)) return rc;
    if (int rc = batch_attach(b, s->growing, s->filter, q_filter, nq, on)) return rc;
    if (int rc = batch_submit(b, term_ids, q_off, nq)) return rc;
    s->ring.push();
    return VBM25_OK;
}
static int stream_collect_impl(vbm25_stream *s, vbm25_hit *hits, uint32_t *n_hits, uint32_t *nq_out) {
    if (!s) return set_error(VBM25_ERR_INVALID, "stream is NULL");
    if (s->ring.empty()) return set_error(VBM25_ERR_INVALID, "no batch in flight");
    vbm25_batch *b = s->slots[s->ring.head];
    if ((!hits || !n_hits) && b->nq) return set_error(VBM25_ERR_INVALID, "NULL argument");
    const int rc = vbm25_batch_finish_download(b, hits, n_hits);
    if (nq_out) *nq_out = b->nq;
    s->ring.pop();
    return rc;
}

}  // namespace vbm25

using namespace vbm25;

extern "C" {

int vbm25_stream_create(vbm25_index *ix, uint32_t depth, uint32_t max_queries, uint32_t max_total_terms, uint32_t k, vbm25_stream **out) {
    return guarded([&] { return stream_create_impl(ix, depth, max_queries, max_total_terms, k, out); });
}
void vbm25_stream_destroy(vbm25_stream *s) { delete s; }
int vbm25_stream_submit(vbm25_stream *s, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq) {
    return guarded([&] { return stream_submit_impl(s, false, nullptr, term_ids, q_off, nq); });
}
int vbm25_stream_submit_filtered(vbm25_stream *s, const uint32_t *q_filter, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq) {
    return guarded([&] { return stream_submit_impl(s, true, q_filter, term_ids, q_off, nq); });
}
int vbm25_stream_set_growing(vbm25_stream *s, const vbm25_device_growing *gs) {
    return guarded([&] { return stream_set_growing_impl(s, gs); });
}
int vbm25_stream_set_filter(vbm25_stream *s, const vbm25_filter *f) {
    return guarded([&] { return stream_set_filter_impl(s, f); });
}
int vbm25_stream_collect(vbm25_stream *s, vbm25_hit *hits, uint32_t *n_hits, uint32_t *nq_out) {
    return guarded([&] { return stream_collect_impl(s, hits, n_hits, nq_out); });
}
int vbm25_stream_in_flight(const vbm25_stream *s) { return s ? int(s->ring.count) : 0; }

}  // extern "C"
