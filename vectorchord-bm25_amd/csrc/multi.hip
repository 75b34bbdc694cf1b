// multi.hip -- vbm25_multi: the index replicated over several GPUs of one node, a batch cut into one shard per replica, one host
// thread per device.  No kernel of its own: every shard is a vbm25_batch (search.hip).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "host_objects.h"

using namespace vbm25;

// ---------------------------------------------------------------------------
// Several GPUs of one node behind the C ABI (BASELINE.json configs[3]).  The path shards by
// independent queries: the index is replicated, a batch is cut into contiguous shards, nothing is exchanged between the
// GPUs but the replicas themselves -- made ONCE, GPU to GPU (hipMemcpyPeerAsync over xGMI: one host upload, n - 1 peer
// copies, derived arrays included).  The hit records go straight from every GPU to the caller's host buffer (pinned
// staging, one asynchronous copy per device and run): the caller is the host, so a device-side gather (peer copies or
// RCCL) would only add a hop.  One host thread drives all devices: every device has its own batch objects and stream,
// the shards run concurrently, fetch waits for all of them.
// ---------------------------------------------------------------------------

// One host thread per device (round 5): a shard's set_queries -- validation, routing, staging in pinned memory: 80 us per 1024
// queries -- and the enqueue of its scan were done for all the devices by the caller's thread, one after the other; at eight devices
// that was 0.78 ms of host time per step against 0.28 ms of device time (profiles/r5_multi_enqueue.txt).  The workers live as long
// as the vbm25_multi; a call hands every worker its part and waits for all of them.
struct MultiWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;  // (empty: none)
    bool quit = false, done = true;
    int rc = 0;
    char err[ERROR_TEXT_BYTES] = "";
    void loop() {
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv.wait(lk, [&] { return quit || job; });
            if (quit) return;
            std::function<int()> f = std::move(job);
            job = nullptr;
            lk.unlock();
            int r;
            try {  // (an exception on a worker thread would be std::terminate: it becomes the part's error code)
                r = f();
            } catch (const std::bad_alloc &) {
                r = set_error(VBM25_ERR_NOMEM, "out of host memory in a device worker");
            } catch (const std::exception &e) {
                r = set_error(VBM25_ERR_DEVICE, "exception in a device worker: %s", e.what());
            }
            lk.lock();
            rc = r;
            if (r) error_text_read(err);
            done = true;
            cv.notify_all();
        }
    }
};
struct vbm25_multi {
    std::vector<vbm25_index *> replicas;  // [0] is the one uploaded from the host
    vbm25_multi_batch *scratch = nullptr;  // batch object re-used by vbm25_multi_search_batch
    std::vector<std::unique_ptr<MultiWorker>> workers;  // one per replica beyond the first (the caller's thread takes part 0)
    ~vbm25_multi() {
        for (auto &w : workers) {
            {
                std::lock_guard<std::mutex> g(w->m);
                w->quit = true;
            }
            w->cv.notify_all();
            if (w->th.joinable()) w->th.join();
        }
        for (vbm25_index *ix : replicas) vbm25_index_destroy(ix);
    }
    // fn(i) for every part i, concurrently; the first error (by part number) is the call's
    // The workers and their one job slot belong to the vbm25_multi: calls on different vbm25_multi_batch objects of one vbm25_multi from
    // several threads are serialised here (vbm25.h says so).
    std::mutex call_m;
    int each_part(size_t n, const std::function<int(size_t)> &fn) {
        std::lock_guard<std::mutex> call_guard(call_m);
        while (workers.size() + 1 < n) {
            workers.emplace_back(new MultiWorker);
            MultiWorker *w = workers.back().get();
            w->th = std::thread([w] { w->loop(); });
        }
        for (size_t i = 1; i < n; ++i) {
            MultiWorker *w = workers[i - 1].get();
            std::lock_guard<std::mutex> g(w->m);
            w->done = false;
            w->job = [&fn, i] { return fn(i); };
            w->cv.notify_all();
        }
        int rc = 0;
        try {  // (the workers hold a reference to fn: they are always waited for, whatever part 0 does)
            rc = n ? fn(0) : 0;
        } catch (const std::bad_alloc &) {
            rc = set_error(VBM25_ERR_NOMEM, "out of host memory");
        } catch (const std::exception &e) {
            rc = set_error(VBM25_ERR_DEVICE, "exception in part 0: %s", e.what());
        }
        char err[ERROR_TEXT_BYTES];
        error_text_read(err);
        for (size_t i = 1; i < n; ++i) {
            MultiWorker *w = workers[i - 1].get();
            std::unique_lock<std::mutex> lk(w->m);
            w->cv.wait(lk, [&] { return w->done; });
            if (w->rc && !rc) {
                rc = w->rc;
                std::memcpy(err, w->err, sizeof err);
            }
        }
        if (rc) error_text_write(err);
        return rc;
    }
};
struct vbm25_multi_batch {
    vbm25_multi *multi = nullptr;
    uint32_t max_queries = 0, max_terms = 0, k = 0, nq = 0;
    std::vector<vbm25_batch *> parts;      // one per replica
    std::vector<uint32_t> lo;              // shard bounds: replica i has the queries [lo[i], lo[i + 1])
    std::vector<std::vector<uint32_t>> off_parts;  // per part: its queries' offsets rebased to 0
    uint32_t tune_generation = 0;          // of the tuning switches its parts copied (vbm25_multi_search_batch rebuilds a stale one)
    // vbm25_multi_batch_set_growing / _set_filter: per replica its own handles; the selectors of the whole batch (max_queries), cut by
    // the shard bounds when set_queries fixes them and staged with each shard's queries
    std::vector<const vbm25_device_growing *> growing;
    std::vector<const vbm25_filter *> filters;
    std::vector<uint32_t> sel;
    bool sel_on = false;                   // some selector names a bitmap
    ~vbm25_multi_batch() {
        for (vbm25_batch *b : parts) vbm25_batch_destroy(b);
    }
};

namespace {

// the first replica: uploaded from the host (desc), or made of the device segment on the segment's device (from_device)
int multi_create_impl(const vbm25_index_desc *desc, const vbm25_device_segment *dseg, bool from_device, const int *devices, int n_devices,
                      vbm25_multi **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!devices || n_devices <= 0) return set_error(VBM25_ERR_INVALID, "no devices given");
    if (from_device) {
        if (!dseg) return set_error(VBM25_ERR_INVALID, "device segment is NULL");
        if (devices[0] != dseg->device)
            return set_error(VBM25_ERR_INVALID, "devices[0] is %d, the segment lives on device %d: the first replica is made where the segment is",
                             devices[0], dseg->device);
    }
    auto m = std::make_unique<vbm25_multi>();
    vbm25_index *first = nullptr;
    if (int rc = from_device ? vbm25_index_create_from_device(dseg, &first) : vbm25_index_create(desc, devices[0], &first)) return rc;
    m->replicas.push_back(first);
    for (int i = 1; i < n_devices; ++i) {
        vbm25_index *r = nullptr;
        if (int rc = clone_index(first, devices[i], &r)) return rc;
        m->replicas.push_back(r);
    }
    *out = m.release();
    return VBM25_OK;
}

int multi_batch_create_impl(vbm25_multi *m, uint32_t max_queries, uint32_t max_total_terms, uint32_t k, vbm25_multi_batch **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!m) return set_error(VBM25_ERR_INVALID, "multi is NULL");
    if (!max_queries) return set_error(VBM25_ERR_INVALID, "max_queries is 0");
    auto mb = std::make_unique<vbm25_multi_batch>();
    mb->multi = m;
    mb->max_queries = max_queries;
    mb->max_terms = max_total_terms;
    mb->k = k;
    const uint32_t n = uint32_t(m->replicas.size());
    const uint32_t per = (max_queries + n - 1) / n;  // a shard is at most this many queries; it may hold all the terms
    for (vbm25_index *ix : m->replicas) {
        vbm25_batch *b = nullptr;
        if (int rc = vbm25_batch_create(ix, per, std::max(max_total_terms, 1u), k, &b)) return rc;
        b->pinned_results = true;
        mb->parts.push_back(b);
    }
    mb->lo.assign(n + 1, 0);
    mb->growing.assign(n, nullptr);
    mb->filters.assign(n, nullptr);
    mb->tune_generation = tuning_snapshot().generation;
    *out = mb.release();
    return VBM25_OK;
}

int multi_batch_set_queries_body(vbm25_multi_batch *mb, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq) {
    if (!mb || !q_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (nq > mb->max_queries) return set_error(VBM25_ERR_INVALID, "%u queries exceed the batch capacity %u", nq, mb->max_queries);
    if (q_off[0] != 0) return set_error(VBM25_ERR_INVALID, "q_off[0] must be 0");
    const uint32_t n = uint32_t(mb->parts.size());
    mb->nq = nq;
    for (uint32_t i = 0; i <= n; ++i) {  // contiguous, balanced shards (the first nq % n get one query more)
        const uint32_t base = nq / n, rem = nq % n;
        mb->lo[i] = i * base + std::min(i, rem);
    }
    for (uint32_t i = 0; i < n; ++i)
        if (q_off[mb->lo[i + 1]] < q_off[mb->lo[i]]) return set_error(VBM25_ERR_INVALID, "q_off not monotone");
    mb->off_parts.resize(n);
    // every shard by its device's own host thread: validation, routing and staging of the shards run side by side
    return mb->multi->each_part(n, [&](size_t i) -> int {
        const uint32_t a = mb->lo[i], b = mb->lo[i + 1];
        std::vector<uint32_t> &off = mb->off_parts[i];
        off.resize(size_t(b - a) + 1);
        for (uint32_t q = a; q <= b; ++q) off[q - a] = q_off[q] - q_off[a];
        // the shard's filter and its cut of the selectors (they ride in the shard's staged block)
        vbm25_batch *part = mb->parts[i];
        const uint32_t *sel = mb->filters[i] && mb->sel_on ? mb->sel.data() + a : nullptr;
        bool on = false;
        if (int rc = batch_attach_check(part, mb->growing[i], mb->filters[i], sel, b - a, &on)) return rc;
        if (int rc = batch_attach(part, mb->growing[i], mb->filters[i], sel, b - a, on)) return rc;
        // staged in the part's pinned memory, copied on its own stream: the devices' uploads overlap
        const int rc = vbm25_batch_set_queries_impl(part, term_ids ? term_ids + q_off[a] : nullptr, off.data(), b - a, true);
        part->stage_sel = nullptr;
        return rc;
    });
}

// A failed call leaves no queries in any part (include/vbm25.h): a shard that rejected the new set must not keep its old one, whose
// records fetch would write at the new set's shard offset -- past the end of the caller's buffers
int multi_batch_set_queries_impl(vbm25_multi_batch *mb, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq) {
    auto clear = [mb] {
        mb->nq = 0;
        std::fill(mb->lo.begin(), mb->lo.end(), 0u);
        for (vbm25_batch *b : mb->parts) batch_clear_queries(b);
    };
    int rc;
    try {
        rc = multi_batch_set_queries_body(mb, term_ids, q_off, nq);
    } catch (...) {
        if (mb) clear();
        throw;
    }
    if (rc && mb) clear();
    return rc;
}

int multi_batch_run_impl(vbm25_multi_batch *mb) {
    if (!mb) return set_error(VBM25_ERR_INVALID, "batch is NULL");
    // every device on its own stream, enqueued by its own host thread: the shards run concurrently
    return mb->multi->each_part(mb->parts.size(), [&](size_t i) -> int {
        vbm25_batch *b = mb->parts[i];
        if (!b->nq) return VBM25_OK;
        void *st = b->bigk ? nullptr : b->lat_stream;
        if (int rc = b->growing ? batch_run_growing_impl(b, st) : vbm25_batch_run_impl(b, st)) return rc;
        return vbm25_batch_enqueue_download(b);  // the shard's records to pinned host memory, behind its scan
    });
}

// a filter with selectors that name a bitmap and a growing segment on one replica: the pairing rules of the batch setters
int multi_pair_check(const vbm25_filter *f, const vbm25_device_growing *gs, size_t i) {
    if (!f || !gs) return VBM25_OK;
    if (!f->grow_serial) return set_error(VBM25_ERR_UNSUPPORTED, "replica %zu: a growing segment and a filter without growing bitmaps", i);
    if (f->grow_serial != gs->serial)
        return set_error(VBM25_ERR_INVALID, "replica %zu: the filter's growing bitmaps belong to another upload than the growing segment", i);
    return filter_growing_count_check(f, gs);
}

// per_device NULL: every replica's segment detached.  Everything is checked before any replica changes.
int multi_batch_set_growing_impl(vbm25_multi_batch *mb, const vbm25_device_growing *const *per_device) {
    if (!mb) return set_error(VBM25_ERR_INVALID, "batch is NULL");
    const size_t n = mb->parts.size();
    for (size_t i = 0; per_device && i < n; ++i) {
        if (per_device[i] && per_device[i]->index != mb->multi->replicas[i])
            return set_error(VBM25_ERR_INVALID, "growing segment %zu does not belong to replica %zu's index", i, i);
        if (mb->sel_on)
            if (int rc = multi_pair_check(mb->filters[i], per_device[i], i)) return rc;
    }
    for (size_t i = 0; i < n; ++i) {
        const vbm25_device_growing *gs = per_device ? per_device[i] : nullptr;
        vbm25_batch *b = mb->parts[i];
        if (int rc = use_device(b->device)) return rc;
        if (int rc = batch_quiesce(b)) return rc;  // (a run in flight reads the old segment to its end)
        if (gs)
            if (int rc = batch_growing_buffers(b, gs)) return rc;
        b->growing = gs;
        mb->growing[i] = gs;
    }
    return VBM25_OK;
}

// per_device NULL: no filter.  q_filter: max_queries selectors; a selector must be UINT32_MAX or below every filter's bitmap count.
int multi_batch_set_filter_impl(vbm25_multi_batch *mb, const vbm25_filter *const *per_device, const uint32_t *q_filter) {
    if (!mb) return set_error(VBM25_ERR_INVALID, "batch is NULL");
    const size_t n = mb->parts.size();
    if (!per_device) {
        std::fill(mb->filters.begin(), mb->filters.end(), nullptr);
        mb->sel_on = false;
        for (vbm25_batch *b : mb->parts) {  // (the current query set's next run filters nothing either)
            b->filter = nullptr;
            b->filt_on = false;
        }
        return VBM25_OK;
    }
    if (!q_filter) return set_error(VBM25_ERR_INVALID, "q_filter is NULL");
    uint32_t f_min = UINT32_MAX;
    for (size_t i = 0; i < n; ++i) {
        if (!per_device[i]) return set_error(VBM25_ERR_INVALID, "filter %zu is NULL", i);
        if (per_device[i]->index != mb->multi->replicas[i])
            return set_error(VBM25_ERR_INVALID, "filter %zu does not belong to replica %zu's index", i, i);
        f_min = std::min(f_min, per_device[i]->n_bitmaps);
    }
    bool on = false;
    for (uint32_t q = 0; q < mb->max_queries; ++q) {
        if (q_filter[q] == UINT32_MAX) continue;
        if (q_filter[q] >= f_min) return set_error(VBM25_ERR_INVALID, "query %u: selector %u, a filter has %u bitmaps", q, q_filter[q], f_min);
        on = true;
    }
    for (size_t i = 0; on && i < n; ++i)
        if (int rc = multi_pair_check(per_device[i], mb->growing[i], i)) return rc;
    mb->filters.assign(per_device, per_device + n);
    mb->sel.assign(q_filter, q_filter + mb->max_queries);
    mb->sel_on = on;
    return VBM25_OK;
}

int multi_batch_fetch_impl(vbm25_multi_batch *mb, vbm25_hit *hits, uint32_t *n_hits) {
    if (!mb || (!hits && mb->nq) || (!n_hits && mb->nq)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    // every part is drained -- by its device's own host thread -- whatever another one returns: no stream is left with a download
    // pending that the next fetch would take for its own; the first error (by part number) is the call's
    return mb->multi->each_part(mb->parts.size(), [&](size_t i) -> int {
        vbm25_batch *b = mb->parts[i];
        if (!b->nq) return VBM25_OK;
        const int rc = vbm25_batch_finish_download(b, hits + size_t(mb->lo[i]) * mb->k, n_hits + mb->lo[i]);
        b->download_enqueued = false;
        return rc;
    });
}

}  // namespace

extern "C" {

int vbm25_multi_create(const vbm25_index_desc *desc, const int *devices, int n_devices, vbm25_multi **out) {
    return guarded([&] { return multi_create_impl(desc, nullptr, false, devices, n_devices, out); });
}
int vbm25_multi_create_from_device(const vbm25_device_segment *seg, const int *devices, int n_devices, vbm25_multi **out) {
    return guarded([&] { return multi_create_impl(nullptr, seg, true, devices, n_devices, out); });
}
void vbm25_multi_destroy(vbm25_multi *m) {
    if (!m) return;
    if (m->scratch) vbm25_multi_batch_destroy(m->scratch);
    delete m;
}
int vbm25_multi_device_count(const vbm25_multi *m) { return m ? int(m->replicas.size()) : 0; }
int vbm25_multi_index(vbm25_multi *m, int i, vbm25_index **out) {
    if (!m || !out || i < 0 || size_t(i) >= m->replicas.size()) return set_error(VBM25_ERR_INVALID, "bad argument");
    *out = m->replicas[size_t(i)];
    return VBM25_OK;
}
int vbm25_multi_batch_create(vbm25_multi *m, uint32_t max_queries, uint32_t max_total_terms, uint32_t k, vbm25_multi_batch **out) {
    return guarded([&] { return multi_batch_create_impl(m, max_queries, max_total_terms, k, out); });
}
void vbm25_multi_batch_destroy(vbm25_multi_batch *mb) { delete mb; }
int vbm25_multi_batch_set_queries(vbm25_multi_batch *mb, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq) {
    return guarded([&] { return multi_batch_set_queries_impl(mb, term_ids, q_off, nq); });
}
int vbm25_multi_batch_set_growing(vbm25_multi_batch *mb, const vbm25_device_growing *const *per_device) {
    return guarded([&] { return multi_batch_set_growing_impl(mb, per_device); });
}
int vbm25_multi_batch_set_filter(vbm25_multi_batch *mb, const vbm25_filter *const *per_device, const uint32_t *q_filter) {
    return guarded([&] { return multi_batch_set_filter_impl(mb, per_device, q_filter); });
}
int vbm25_multi_batch_run(vbm25_multi_batch *mb) {
    return guarded([&] { return multi_batch_run_impl(mb); });
}
int vbm25_multi_batch_fetch(vbm25_multi_batch *mb, vbm25_hit *hits, uint32_t *n_hits) {
    return guarded([&] { return multi_batch_fetch_impl(mb, hits, n_hits); });
}
int vbm25_multi_search_batch(vbm25_multi *m, const uint32_t *term_ids, const uint32_t *q_off, uint32_t nq, uint32_t k,
                             vbm25_hit *hits, uint32_t *n_hits) {
    return guarded([&]() -> int {
        if (!m || !q_off) return set_error(VBM25_ERR_INVALID, "NULL argument");
        if (nq == 0) return k ? VBM25_OK : set_error(VBM25_ERR_INVALID, "number of needed rows is set to 0");
        vbm25_multi_batch *mb = m->scratch;
        const uint32_t n_terms = q_off[nq] ? q_off[nq] : 1;
        if (!mb || mb->k != k || mb->max_queries < nq || mb->max_terms < n_terms || mb->tune_generation != tuning_snapshot().generation) {
            if (mb) vbm25_multi_batch_destroy(mb);
            m->scratch = nullptr;
            if (int rc = multi_batch_create_impl(m, std::max(nq, 16u), std::max(n_terms, 256u), k, &mb)) return rc;
            m->scratch = mb;
        }
        if (int rc = multi_batch_set_queries_impl(mb, term_ids, q_off, nq)) return rc;
        if (int rc = multi_batch_run_impl(mb)) return rc;
        return multi_batch_fetch_impl(mb, hits, n_hits);
    });
}

}  // extern "C"
