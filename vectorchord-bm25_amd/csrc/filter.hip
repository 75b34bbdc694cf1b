// filter.hip -- vbm25_filter's own life: the sealed bitmaps (create, update, read), the growing bitmaps (set, update, extend in
// place: filter_extend.h), and a filter carried across a compaction (remap: maintain.hip does the work).  How a batch applies a filter
// is search.hip's.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <utility>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "host_objects.h"
#include "filter_extend.h"

namespace vbm25 {

// ---------------------------------------------------------------------------
// Filtered search: bm25::search's `filter` (search.rs:217-236) as per-query document bitmaps.  The kernels check a candidate's bit
// where it is admitted to a top-k list (query_filter, device_types.h), a filtered query starts from threshold 0 (no theta0), and the
// k > 1024 path wipes the rejected documents' scores before its sort.  The records are those of the unfiltered full ranking with the
// rejected documents removed, cut to k.
// ---------------------------------------------------------------------------
static int filter_check_words(const vbm25_filter *f, const uint64_t *w) {
    const uint32_t tail = f->index->n_docs & 63u;  // bits at or beyond n_docs must be zero
    if (f->words && tail && (w[f->words - 1] >> tail) != 0)
        return set_error(VBM25_ERR_INVALID, "bitmap has bits set at or beyond n_docs = %u", f->index->n_docs);
    return VBM25_OK;
}

static int vbm25_filter_create_impl(vbm25_index *ix, uint32_t n_bitmaps, const uint64_t *words, vbm25_filter **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ix) return set_error(VBM25_ERR_INVALID, "index is NULL");
    if (n_bitmaps == 0 || n_bitmaps == UINT32_MAX) return set_error(VBM25_ERR_INVALID, "n_bitmaps must be 1 .. 2^32 - 2");
    if (int rc = use_device(ix->device)) return rc;
    auto f = std::make_unique<vbm25_filter>();
    f->index = ix;
    f->device = ix->device;
    f->n_bitmaps = n_bitmaps;
    f->words = (ix->n_docs + 63u) / 64u;
    const size_t bytes = 8ull * n_bitmaps * f->words;
    if (words)
        for (uint32_t i = 0; i < n_bitmaps; ++i)
            if (int rc = filter_check_words(f.get(), words + size_t(i) * f->words)) return rc;
    if (int rc = f->bits.alloc(bytes)) return rc;
    if (words && bytes) HIP_TRY(hipMemcpy(f->bits.p, words, bytes, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(f->bits.p, 0, bytes ? bytes : 16));
    *out = f.release();
    return VBM25_OK;
}

static int vbm25_filter_update_impl(vbm25_filter *f, uint32_t i, const uint64_t *words) {
    if (!f || !words) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (i >= f->n_bitmaps) return set_error(VBM25_ERR_INVALID, "bitmap %u of a filter of %u", i, f->n_bitmaps);
    if (int rc = filter_check_words(f, words)) return rc;
    if (int rc = use_device(f->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (runs in flight read the old bits to their end)
    if (f->words) HIP_TRY(hipMemcpy(f->bits.as<uint64_t>() + size_t(i) * f->words, words, 8ull * f->words, hipMemcpyHostToDevice));
    return VBM25_OK;
}

// a filter's growing bitmaps are sized for the n_grow they were set at: after vbm25_device_growing_append they are stale until
// vbm25_filter_set_growing is called again (rejecting the new documents silently would hide inserts from filtered queries)
int filter_growing_count_check(const vbm25_filter *f, const vbm25_device_growing *gs) {
    if (f->grow_n == gs->n_grow) return VBM25_OK;
    return set_error(VBM25_ERR_INVALID, "the filter's growing bitmaps cover %u documents and the growing segment holds %u (appended to since): "
                                        "set the growing bitmaps again", f->grow_n, gs->n_grow);
}

// The selectors of a query set against a filter: every one of the n is UINT32_MAX (the query takes no bitmap) or names a bitmap of f.
// *any (may be NULL): some selector names one.
int filter_selector_check(const vbm25_filter *f, const uint32_t *sel, uint32_t n, bool *any) {
    bool on = false;
    for (uint32_t q = 0; q < n; ++q) {
        if (sel[q] == UINT32_MAX) continue;
        if (sel[q] >= f->n_bitmaps)
            return set_error(VBM25_ERR_INVALID, "query %u: selector %u, the filter has %u bitmaps", q, sel[q], f->n_bitmaps);
        on = true;
    }
    if (any) *any = on;
    return VBM25_OK;
}

// ---------------------------------------------------------------------------
// Filters on the growing segment: a filter's F growing bitmaps (one bit per growing document g of one upload) go with its F sealed
// bitmaps -- query q's selector s names both.  The records are those of the host composition with the rejected growing documents
// treated as deleted.  The filter names the upload by its serial number; the batch setters and every run check it.
// ---------------------------------------------------------------------------
static int filter_check_growing_words(uint32_t n_grow, uint32_t gw, const uint64_t *w) {
    const uint32_t tail = n_grow & 63u;  // bits at or beyond n_grow must be zero
    if (gw && tail && (w[gw - 1] >> tail) != 0)
        return set_error(VBM25_ERR_INVALID, "growing bitmap has bits set at or beyond n_grow = %u", n_grow);
    return VBM25_OK;
}

static int vbm25_filter_set_growing_impl(vbm25_filter *f, const vbm25_device_growing *gs, const uint64_t *words) {
    if (!f) return set_error(VBM25_ERR_INVALID, "filter is NULL");
    if (gs && gs->index != f->index) return set_error(VBM25_ERR_INVALID, "the growing segment belongs to another index");
    const uint32_t gw = gs ? (gs->n_grow + 63u) / 64u : 0u;
    if (gs && words)
        for (uint32_t i = 0; i < f->n_bitmaps; ++i)
            if (int rc = filter_check_growing_words(gs->n_grow, gw, words + size_t(i) * gw)) return rc;
    if (int rc = use_device(f->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (runs in flight read the old bits to their end)
    DeviceBuffer nb;  // the new bitmaps (none: the old ones are freed with it)
    if (gs) {
        const size_t bytes = 8ull * f->n_bitmaps * gw;
        if (int rc = nb.alloc(bytes)) return rc;
        if (words && bytes) HIP_TRY(hipMemcpy(nb.p, words, bytes, hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(nb.p, 0, bytes ? bytes : 16));
    }
    std::swap(f->grow_bits.p, nb.p);
    std::swap(f->grow_bits.bytes, nb.bytes);
    f->grow_serial = gs ? gs->serial : 0;
    f->grow_n = gs ? gs->n_grow : 0;
    f->grow_words = gw;
    f->grow_stride = gw;
    return VBM25_OK;
}

static int vbm25_filter_update_growing_impl(vbm25_filter *f, uint32_t i, const uint64_t *words) {
    if (!f || !words) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (!f->grow_serial) return set_error(VBM25_ERR_INVALID, "the filter has no growing bitmaps");
    if (i >= f->n_bitmaps) return set_error(VBM25_ERR_INVALID, "bitmap %u of a filter of %u", i, f->n_bitmaps);
    if (int rc = filter_check_growing_words(f->grow_n, f->grow_words, words)) return rc;
    if (int rc = use_device(f->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (runs in flight read the old bits to their end)
    if (f->grow_words)
        HIP_TRY(hipMemcpy(f->grow_bits.as<uint64_t>() + size_t(i) * f->grow_stride, words, 8ull * f->grow_words, hipMemcpyHostToDevice));
    return VBM25_OK;
}

// Growing bitmaps extended in place after vbm25_device_growing_append: only the delta's F x ceil(d / 64) words cross the host link,
// filter_extend_growing_kernel (growing.h) merges them in.  The bitmaps have a capacity in words (grow_stride) that grows
// geometrically: most calls keep the stride and touch the tail words only, a growth step re-strides all F bitmaps into a new buffer
// on the device.  Everything that can fail short of the device itself comes before the filter changes.
static int vbm25_filter_extend_growing_impl(vbm25_filter *f, const vbm25_device_growing *gs, const uint64_t *words) {
    if (!f || !gs) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (!f->grow_serial) return set_error(VBM25_ERR_INVALID, "the filter has no growing bitmaps");
    if (f->grow_serial != gs->serial) return set_error(VBM25_ERR_INVALID, "the filter's growing bitmaps belong to another upload than this segment");
    if (gs->n_grow < f->grow_n)
        return set_error(VBM25_ERR_INVALID, "the filter's growing bitmaps cover %u documents, the segment holds %u", f->grow_n, gs->n_grow);
    const uint32_t d = gs->n_grow - f->grow_n;
    if (d == 0) return VBM25_OK;
    const uint32_t dw = (d + 63u) / 64u, F = f->n_bitmaps, n_old = f->grow_n, new_words = (gs->n_grow + 63u) / 64u;
    if (words && (d & 63u))
        for (uint32_t i = 0; i < F; ++i)
            if ((words[size_t(i) * dw + dw - 1] >> (d & 63u)) != 0)
                return set_error(VBM25_ERR_INVALID, "delta bitmap %u has bits set at or beyond the %u new documents", i, d);
    if (int rc = use_device(f->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (runs in flight read the old bits to their end)
    const unsigned long long *delta = nullptr;
    if (words) {
        const size_t bytes = 8ull * F * dw;
        if (!f->grow_stage.p || f->grow_stage.bytes < bytes)
            if (int rc = batch_grow_buffer(f->grow_stage, std::max(bytes, 2 * f->grow_stage.bytes))) return rc;
        HIP_TRY(hipMemcpy(f->grow_stage.p, words, bytes, hipMemcpyHostToDevice));
        delta = f->grow_stage.as<unsigned long long>();
    }
    auto launch = [&](const unsigned long long *src, uint32_t src_stride, unsigned long long *dst, uint32_t dst_stride, uint32_t w0) {
        const unsigned long long total = (unsigned long long)F * (new_words - w0);
        const uint32_t grid = uint32_t(std::min<unsigned long long>((total + 255) / 256, 4096));
        filter_extend_growing_kernel<<<grid, 256>>>(src, src_stride, f->grow_words, dst, dst_stride, F, n_old, delta, dw, w0, new_words);
    };
    if (new_words <= f->grow_stride) {
        if (delta) {  // (an all-zero delta: the words beyond the old count are zero already)
            launch(f->grow_bits.as<unsigned long long>(), f->grow_stride, f->grow_bits.as<unsigned long long>(), f->grow_stride, n_old >> 6);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipDeviceSynchronize());
        }
    } else {
        const uint32_t stride = uint32_t(std::min<uint64_t>(std::max<uint64_t>(new_words, 2ull * f->grow_stride), 1ull << 26));
        DeviceBuffer nb;
        if (int rc = nb.alloc(8ull * F * stride)) return rc;
        HIP_TRY(hipMemset(nb.p, 0, nb.bytes));
        launch(f->grow_bits.as<unsigned long long>(), f->grow_stride, nb.as<unsigned long long>(), stride, 0u);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        std::swap(f->grow_bits.p, nb.p);
        std::swap(f->grow_bits.bytes, nb.bytes);
        f->grow_stride = stride;
    }
    f->grow_n = gs->n_grow;
    f->grow_words = new_words;
    return VBM25_OK;
}

// A filter carried across vbm25_index_maintain: the relabel is the monotone compaction the two deletion inputs define, so the new
// filter's bitmap i is the old sealed bitmap i's bits of the kept documents followed by the old growing bitmap i's bits of the live
// ones (filter_remap_device, maintain.hip).  The old filter is only read.  Everything is checked, and the new words are written,
// before *out is set: a failure leaves nothing behind.
// del.dev: vbm25_filter_remap_device, the three deletion arguments taken from the handle (n_grow is then the handle's)
static int vbm25_filter_remap_impl(const vbm25_filter *old, const RemapDeletions &del, uint32_t n_grow, vbm25_index *nix, vbm25_filter **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!old || !nix) return set_error(VBM25_ERR_INVALID, "NULL argument");
    const vbm25_device_vacuum *dv = del.dev;
    const uint64_t *sealed_deleted = dv ? nullptr : del.sealed_deleted;  // (the handle's words have no bits at or beyond n_docs)
    if (dv) {
        int n_dev = 0;  // before the handles are looked into: without a device there is none of them
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
            return set_error(VBM25_ERR_DEVICE, "no HIP device: a filter lives on the device");
    }
    if (nix->device != old->device)
        return set_error(VBM25_ERR_INVALID, "the new index is on device %d, the filter on device %d", nix->device, old->device);
    const uint32_t N = old->index->n_docs;
    if (dv) {
        if (dv->device != old->device)
            return set_error(VBM25_ERR_INVALID, "the compaction inputs are on device %d, the filter on device %d", dv->device, old->device);
        if (dv->n_sealed != N)
            return set_error(VBM25_ERR_INVALID, "the compaction inputs are of %u sealed documents, the filter's index holds %u", dv->n_sealed, N);
        n_grow = dv->n_grow;
    }
    if (sealed_deleted && (N & 63u) && (sealed_deleted[old->words - 1] >> (N & 63u)))
        return set_error(VBM25_ERR_INVALID, "sealed_deleted has bits at or beyond n_docs = %u", N);
    if (n_grow) {
        if (!old->grow_serial) return set_error(VBM25_ERR_UNSUPPORTED, "%u growing documents and the filter has no growing bitmaps", n_grow);
        if (old->grow_n != n_grow)
            return set_error(VBM25_ERR_INVALID, "the filter's growing bitmaps cover %u documents, the compaction took %u", old->grow_n, n_grow);
    }
    if (int rc = use_device(old->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (device-side writers of the old bits and extends in flight end first)
    auto f = std::make_unique<vbm25_filter>();
    f->index = nix;
    f->device = nix->device;
    f->n_bitmaps = old->n_bitmaps;
    f->words = (nix->n_docs + 63u) / 64u;
    if (int rc = f->bits.alloc(8ull * f->n_bitmaps * f->words)) return rc;
    if (int rc = filter_remap_device(old->device, old->n_bitmaps, N, old->bits.p, n_grow, del, n_grow ? old->grow_bits.p : nullptr,
                                     old->grow_stride, nix->n_docs, f->bits.p))
        return rc;
    *out = f.release();
    return VBM25_OK;
}

static int vbm25_filter_read_impl(const vbm25_filter *f, uint32_t i, int growing, uint64_t *words) {
    if (!f || !words) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (growing && !f->grow_serial) return set_error(VBM25_ERR_INVALID, "the filter has no growing bitmaps");
    if (i >= f->n_bitmaps) return set_error(VBM25_ERR_INVALID, "bitmap %u of a filter of %u", i, f->n_bitmaps);
    if (int rc = use_device(f->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (device-side writers of the bits end first)
    const uint32_t n = growing ? f->grow_words : f->words;
    const uint64_t *src = growing ? f->grow_bits.as<uint64_t>() + size_t(i) * f->grow_stride : f->bits.as<uint64_t>() + size_t(i) * f->words;
    if (n) HIP_TRY(hipMemcpy(words, src, 8ull * n, hipMemcpyDeviceToHost));
    return VBM25_OK;
}

}  // namespace vbm25

using namespace vbm25;

extern "C" {

int vbm25_filter_create(vbm25_index *ix, uint32_t n_bitmaps, const uint64_t *words, vbm25_filter **out) {
    return guarded([&] { return vbm25_filter_create_impl(ix, n_bitmaps, words, out); });
}
int vbm25_filter_update(vbm25_filter *f, uint32_t i, const uint64_t *words) {
    return guarded([&] { return vbm25_filter_update_impl(f, i, words); });
}
int vbm25_filter_device_words(vbm25_filter *f, uint32_t i, void **dev) {
    if (!f || !dev) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (i >= f->n_bitmaps) return set_error(VBM25_ERR_INVALID, "bitmap %u of a filter of %u", i, f->n_bitmaps);
    *dev = f->bits.as<uint64_t>() + size_t(i) * f->words;
    return VBM25_OK;
}
void vbm25_filter_destroy(vbm25_filter *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    delete f;
}
int vbm25_filter_set_growing(vbm25_filter *f, const vbm25_device_growing *gs, const uint64_t *words) {
    return guarded([&] { return vbm25_filter_set_growing_impl(f, gs, words); });
}
int vbm25_filter_update_growing(vbm25_filter *f, uint32_t i, const uint64_t *words) {
    return guarded([&] { return vbm25_filter_update_growing_impl(f, i, words); });
}
int vbm25_filter_extend_growing(vbm25_filter *f, const vbm25_device_growing *gs, const uint64_t *words) {
    return guarded([&] { return vbm25_filter_extend_growing_impl(f, gs, words); });
}
int vbm25_filter_growing_device_words(vbm25_filter *f, uint32_t i, void **dev) {
    if (!f || !dev) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (!f->grow_serial) return set_error(VBM25_ERR_INVALID, "the filter has no growing bitmaps");
    if (i >= f->n_bitmaps) return set_error(VBM25_ERR_INVALID, "bitmap %u of a filter of %u", i, f->n_bitmaps);
    *dev = f->grow_bits.as<uint64_t>() + size_t(i) * f->grow_stride;
    return VBM25_OK;
}
int vbm25_filter_remap(const vbm25_filter *old, const uint64_t *sealed_deleted, uint32_t n_grow, const uint8_t *growing_deleted,
                       vbm25_index *new_index, vbm25_filter **out) {
    return guarded([&] { return vbm25_filter_remap_impl(old, RemapDeletions{sealed_deleted, growing_deleted, nullptr}, n_grow, new_index, out); });
}
int vbm25_filter_remap_device(const vbm25_filter *old, const vbm25_device_vacuum *in, vbm25_index *new_index, vbm25_filter **out) {
    if (out) *out = nullptr;
    if (out && !in) return set_error(VBM25_ERR_INVALID, "NULL argument");  // (a NULL handle is not "nothing deleted")
    return guarded([&] { return vbm25_filter_remap_impl(old, RemapDeletions{nullptr, nullptr, in}, 0, new_index, out); });
}
int vbm25_filter_read(const vbm25_filter *f, uint32_t i, int growing, uint64_t *words) {
    return guarded([&] { return vbm25_filter_read_impl(f, i, growing, words); });
}

}  // extern "C"
