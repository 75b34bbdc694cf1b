// growing.hip -- vbm25_device_growing's own life: upload (from the host's CSR or from arrays in HBM), append, append_documents, delete,
// free.  The kernels are growing_build.h's and growing_append.h's; what a batch does with the segment at query time is search.hip's.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "host_objects.h"
#include "growing_build.h"
#include "growing_append.h"

namespace vbm25 {

static std::atomic<uint64_t> g_growing_serial{0};  // uploads so far (vbm25_device_growing::serial)

// the CSR of an upload or of an append's delta: `held_docs` / `held_el` are the growing documents and postings the segment holds already
static int growing_desc_check(const vbm25_index *ix, const vbm25_growing_desc *d, uint64_t held_docs, uint64_t held_el, uint64_t *e_first_out,
                              uint64_t *n_el_out) {
    const uint32_t n = d->n_docs;
    if (uint64_t(ix->n_docs) + held_docs + n > (1ull << 32))
        return set_error(VBM25_ERR_INVALID, "%u sealed + %llu growing documents exceed 2^32: the doc id ranges would collide", ix->n_docs,
                         (unsigned long long)(held_docs + n));
    if (n && (!d->start || !d->fieldnorm || !d->payload)) return set_error(VBM25_ERR_INVALID, "growing arrays missing");
    const uint64_t e_first = n ? d->start[0] : 0, e_end = n ? d->start[n] : 0;
    for (uint32_t g = 0; g < n; ++g)
        if (d->start[g + 1] < d->start[g]) return set_error(VBM25_ERR_INVALID, "start not monotone at document %u", g);
    if (e_end > d->n_elements) return set_error(VBM25_ERR_INVALID, "start reaches element %llu of %llu", (unsigned long long)e_end,
                                                (unsigned long long)d->n_elements);
    const uint64_t n_el = e_end - e_first;
    if (n_el && (!d->key || !d->tf)) return set_error(VBM25_ERR_INVALID, "growing arrays missing");
    if (held_el + n_el >= (1ull << 31)) return set_error(VBM25_ERR_UNSUPPORTED, "%llu growing elements: the device path takes fewer than 2^31",
                                                         (unsigned long long)(held_el + n_el));
    for (uint32_t g = 0; g < n; ++g)  // Document::checked_new, vector.rs:56-61
        for (uint64_t e = d->start[g] + 1; e < d->start[g + 1]; ++e)
            if (std::memcmp(d->key + 16ull * (e - 1), d->key + 16ull * e, 16) >= 0)
                return set_error(VBM25_ERR_INVALID, "growing document %u: keys must be strictly ascending", g);
    *e_first_out = e_first;
    *n_el_out = n_el;
    return VBM25_OK;
}

static void swap_buffers(DeviceBuffer &a, DeviceBuffer &b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
}

// vbm25_growing_upload, device half: the CSR in HBM on the index's device -> the segment.  `start` may begin anywhere (the kernels
// take it relative to start[0]); `payload`: the buffer of a.payload when the segment may keep it, NULL: the segment takes a copy.
static int growing_build(vbm25_index *ix, const GrowingDeviceArrays &a, DeviceBuffer *payload, vbm25_device_growing **out) {
    const uint32_t n = a.n_docs;
    const uint64_t n_el = a.n_elements;
    auto gs = std::make_unique<vbm25_device_growing>();
    gs->index = ix;
    gs->device = ix->device;
    gs->serial = g_growing_serial.fetch_add(1) + 1;
    gs->n_grow = n;
    gs->n_tiles = uint32_t((uint64_t(n) + GT - 1) / GT);
    const uint32_t nt = ix->n_terms;
    DeviceBuffer tkey, keys, vals, keys2, vals2, cnt, tmp;
    int rc = 0;
    if (payload) {
        swap_buffers(gs->payload, *payload);
    } else {
        if ((rc = gs->payload.alloc(6ull * n))) return rc;
        if (n) HIP_TRY(hipMemcpy(gs->payload.p, a.payload, 6ull * n, hipMemcpyDeviceToDevice));
    }
    if ((rc = tkey.upload(ix->term_key.data(), 16ull * nt)) || (rc = keys.alloc(8ull * n_el)) || (rc = vals.alloc(4ull * n_el)) ||
        (rc = keys2.alloc(8ull * n_el)) || (rc = vals2.alloc(4ull * n_el)) || (rc = cnt.alloc(4)) ||
        (rc = gs->term_start.alloc(4ull * (nt + 1ull))))
        return rc;
    HIP_TRY(hipMemset(cnt.p, 0, 4));
    HIP_TRY(hipMemset(gs->term_start.p, 0, 4ull * (nt + 1ull)));
    uint32_t n_post = 0;
    if (n_el) {
        if (n) grow_map_kernel<<<(n + 255) / 256, 256>>>(tkey.as<ulonglong2>(), nt, n, a.start, reinterpret_cast<const ulonglong2 *>(a.key),
                                                         a.tf, a.deleted, keys.as<unsigned long long>(), vals.as<uint32_t>(),
                                                         cnt.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        // (term id, g) ascending: a stable order of the postings by term with g ascending inside a term (flush.hip's sort of the mappings)
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) {
            return hipcub::DeviceRadixSort::SortPairs(t, tb, keys.as<unsigned long long>(), keys2.as<unsigned long long>(), vals.as<uint32_t>(),
                                                      vals2.as<uint32_t>(), (int)n_el);
        }));
        HIP_TRY(hipMemcpy(&n_post, cnt.p, 4, hipMemcpyDeviceToHost));
    }
    gs->n_post = n_post;
    if ((rc = gs->post_g.alloc(4ull * n_post)) || (rc = gs->post_c.alloc(8ull * n_post))) return rc;
    if (n_post)
        grow_post_kernel<<<(n_post + 255) / 256, 256>>>(keys2.as<unsigned long long>(), vals2.as<uint32_t>(), n_post, nt,
                                                         ix->term_s0.as<double>(), ix->s1.as<double>(), a.fieldnorm,
                                                         gs->post_g.as<uint32_t>(), gs->post_c.as<double>(), gs->term_start.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    gs->term_start_host.resize(nt + 1ull);
    HIP_TRY(hipMemcpy(gs->term_start_host.data(), gs->term_start.p, 4ull * (nt + 1ull), hipMemcpyDeviceToHost));
    // tile tables for the terms with at least one posting per tile (they take at most about as much as the postings' ids); the
    // shorter lists are binary-searched
    std::vector<uint32_t> tab_idx(nt, NONE32);
    uint64_t n_tab = 0;
    if (gs->n_tiles > 1)
        for (uint32_t t = 0; t < nt; ++t)
            if (gs->term_start_host[t + 1] - gs->term_start_host[t] >= gs->n_tiles && n_tab + gs->n_tiles + 1u < NONE32) {
                tab_idx[t] = uint32_t(n_tab);
                n_tab += gs->n_tiles + 1u;
            }
    if ((rc = gs->tab_idx.upload(tab_idx.data(), 4ull * nt)) || (rc = gs->tab.alloc(4ull * n_tab))) return rc;
    if (n_tab) grow_tab_kernel<<<(n_post + 255) / 256, 256>>>(keys2.as<unsigned long long>(), n_post, gs->dev(), gs->tab.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    gs->count_bytes();
    *out = gs.release();
    return VBM25_OK;
}

// vbm25_growing_upload, host half: the checked CSR of the caller goes up
static int vbm25_growing_upload_impl(vbm25_index *ix, const vbm25_growing_desc *d, vbm25_device_growing **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ix || !d) return set_error(VBM25_ERR_INVALID, "NULL argument");
    const uint32_t n = d->n_docs;
    uint64_t e_first = 0, n_el = 0;
    if (int rc = growing_desc_check(ix, d, 0, 0, &e_first, &n_el)) return rc;
    if (int rc = use_device(ix->device)) return rc;
    DeviceBuffer start, key, tf, fn, del, payload;
    int rc = 0;
    if ((rc = start.upload(d->start, 8ull * (n + 1ull))) || (rc = key.upload(d->key ? d->key + 16ull * e_first : nullptr, 16ull * n_el)) ||
        (rc = tf.upload(d->tf ? d->tf + e_first : nullptr, 4ull * n_el)) || (rc = fn.upload(d->fieldnorm, n)) ||
        (d->deleted && (rc = del.upload(d->deleted, n))) || (rc = payload.upload(d->payload, 6ull * n)))
        return rc;
    const GrowingDeviceArrays a{n, n_el, start.as<uint64_t>(), key.as<uint8_t>(), tf.as<uint32_t>(), fn.as<uint8_t>(),
                                d->deleted ? del.as<uint8_t>() : nullptr, payload.as<uint16_t>()};
    return growing_build(ix, a, &payload, out);
}

// vbm25_device_growing_from_pages (pages_device.hip) reads the vectors tape into a CSR on the index's device and builds from there
int growing_from_device_arrays(vbm25_index *ix, const GrowingDeviceArrays &a, vbm25_device_growing **out) {
    if (int rc = use_device(ix->device)) return rc;
    return growing_build(ix, a, nullptr, out);
}

// ---------------------------------------------------------------------------
// vbm25_device_growing_append / vbm25_device_growing_delete (growing_append.h).  Both wait for the device first (a run in flight ends
// on the old arrays) and return when the segment is the new one.  An append validates, allocates and computes into the spare arrays
// and the stage, none of which a search reads, and only then swaps them in: a failure at any point leaves the segment as it was.
// ---------------------------------------------------------------------------

// room for `need` bytes in a buffer nobody reads (a spare, the stage); the contents are not kept.  A buffer that is too small is
// replaced by one half as large again as needed: sizes grow geometrically, a run of small appends allocates (and hipFree
// synchronises) only now and then.
static int reserve_spare(DeviceBuffer &b, size_t need) {
    if (b.p && b.bytes >= need) return VBM25_OK;
    DeviceBuffer nb;
    if (int rc = nb.alloc(need + need / 2)) return rc;
    swap_buffers(b, nb);
    return VBM25_OK;
}

constexpr size_t GROW_STAGE_KEEP = 16u << 20;  // a larger stage (a bulk append) is released at the end of the call

// The append behind its checks.  The delta's arrays (d's, its elements e_first .. e_first + n_el) are on the host (`kind`
// hipMemcpyHostToDevice: vbm25_device_growing_append) or in HBM on the segment's device (hipMemcpyDeviceToDevice:
// vbm25_device_growing_append_documents); they go into the stage either way, and everything behind the copies reads the stage.
// With hipMemcpyDeviceToDevice no pointer of `d` may be dereferenced on the host: this body only hands them to hipMemcpy.
static int device_growing_append_core(vbm25_device_growing *gs, const vbm25_growing_desc *d, uint64_t e_first, uint64_t n_el, hipMemcpyKind kind) {
    const vbm25_index *ix = gs->index;
    const uint32_t n = d->n_docs, g0 = gs->n_grow, nt = ix->n_terms;
    if (!n) return VBM25_OK;
    if (uint64_t(g0) + n > 0xffffffffull) return set_error(VBM25_ERR_INVALID, "%llu growing documents: at most 2^32 - 1", (unsigned long long)g0 + n);
    if (int rc = use_device(gs->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (runs in flight read the old arrays to their end)
    // on every way out: a stage that a bulk append made larger than GROW_STAGE_KEEP is given back (small appends keep theirs, so a
    // run of them allocates nothing; a bulk append pays one hipFree, little next to its sort), and device_bytes is counted again
    struct ReleaseStageAndCount {
        vbm25_device_growing *gs;
        ~ReleaseStageAndCount() {
            if (gs->stage.bytes > GROW_STAGE_KEEP) {
                DeviceBuffer none;
                swap_buffers(gs->stage, none);
            }
            gs->count_bytes();
        }
    } on_exit{gs};
    const uint32_t n_new = g0 + n, n_tiles = uint32_t((uint64_t(n_new) + GT - 1) / GT);
    int rc = 0;
    if (!gs->term_key.p && (rc = gs->term_key.upload(ix->term_key.data(), 16ull * nt))) {  // (once per segment: 16 B per term)
        DeviceBuffer none;  // a buffer whose copy failed holds no keys
        swap_buffers(gs->term_key, none);
        return rc;
    }
    // the stage: the delta's arrays, the sort's and the scan's
    size_t sort_tb = 0, scan_tb = 0, stage_bytes = 0;
    if (n_el)
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tb, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                                   (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n_el));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tb, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)(nt + 1u)));
    auto take = [&](size_t bytes) {
        const size_t at = stage_bytes;
        stage_bytes += (bytes + 255u) & ~size_t(255);
        return at;
    };
    const size_t o_start = take(8ull * (n + 1ull)), o_key = take(16ull * n_el), o_tf = take(4ull * n_el), o_fn = take(n), o_del = take(n),
                 o_keys = take(8ull * n_el), o_vals = take(4ull * n_el), o_keys2 = take(8ull * n_el), o_vals2 = take(4ull * n_el),
                 o_cnt = take(8), o_ins = take(4ull * n_el), o_flags = take(4ull * (nt + 1ull)), o_offs = take(4ull * (nt + 1ull)),
                 o_tterm = take(4ull * nt), o_sort = take(sort_tb), o_scan = take(scan_tb);
    if ((rc = reserve_spare(gs->stage, stage_bytes))) return rc;
    uint8_t *sp = gs->stage.as<uint8_t>();
    auto at = [&](size_t o) { return static_cast<void *>(sp + o); };
    uint64_t *start = static_cast<uint64_t *>(at(o_start));
    unsigned long long *keys = static_cast<unsigned long long *>(at(o_keys)), *keys2 = static_cast<unsigned long long *>(at(o_keys2));
    uint32_t *tf = static_cast<uint32_t *>(at(o_tf)), *vals = static_cast<uint32_t *>(at(o_vals)), *vals2 = static_cast<uint32_t *>(at(o_vals2));
    uint32_t *cnt = static_cast<uint32_t *>(at(o_cnt)), *ins = static_cast<uint32_t *>(at(o_ins)), *flags = static_cast<uint32_t *>(at(o_flags)),
             *offs = static_cast<uint32_t *>(at(o_offs)), *tterm = static_cast<uint32_t *>(at(o_tterm));
    uint8_t *fn = static_cast<uint8_t *>(at(o_fn)), *del = static_cast<uint8_t *>(at(o_del));
    HIP_TRY(hipMemcpy(start, d->start, 8ull * (n + 1ull), kind));
    HIP_TRY(hipMemcpy(fn, d->fieldnorm, n, kind));
    if (d->deleted) HIP_TRY(hipMemcpy(del, d->deleted, n, kind));
    HIP_TRY(hipMemsetAsync(cnt, 0, 8));
    // 1. the delta's postings as sorted (term, g) keys
    uint32_t n_dpost = 0;
    if (n_el) {
        HIP_TRY(hipMemcpy(at(o_key), d->key + 16ull * e_first, 16ull * n_el, kind));
        HIP_TRY(hipMemcpy(tf, d->tf + e_first, 4ull * n_el, kind));
        grow_append_map_kernel<<<uint32_t((n_el + 255) / 256), 256>>>(gs->term_key.as<ulonglong2>(), nt, n, g0, start, uint32_t(n_el),
                                                                      static_cast<const ulonglong2 *>(at(o_key)), tf,
                                                                      d->deleted ? del : nullptr, keys, vals, cnt);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(at(o_sort), sort_tb, keys, keys2, vals, vals2, (int)n_el));
        HIP_TRY(hipMemcpy(&n_dpost, cnt, 4, hipMemcpyDeviceToHost));
    }
    const uint32_t n_post = gs->n_post + n_dpost;
    // every array the new segment needs, before anything is written
    DeviceBuffer new_payload;  // (only when the payloads outgrow their buffer)
    if ((rc = reserve_spare(gs->post_g2, 4ull * n_post)) || (rc = reserve_spare(gs->post_c2, 8ull * n_post)) ||
        (rc = reserve_spare(gs->term_start2, 4ull * (nt + 1ull))) || (rc = reserve_spare(gs->tab_idx2, 4ull * nt)))
        return rc;
    if (gs->payload.bytes < 6ull * n_new) {
        if ((rc = new_payload.alloc(6ull * n_new + 3ull * n_new))) return rc;  // (half as much again, as reserve_spare)
        if (g0) HIP_TRY(hipMemcpyAsync(new_payload.p, gs->payload.p, 6ull * g0, hipMemcpyDeviceToDevice));
    }
    uint16_t *payload = new_payload.p ? new_payload.as<uint16_t>() : gs->payload.as<uint16_t>();
    HIP_TRY(hipMemcpy(payload + 3ull * g0, d->payload, 6ull * n, kind));  // (behind the documents the searches read)
    // 2 - 4. the merged postings and their term starts
    uint32_t *new_start = gs->term_start2.as<uint32_t>(), *new_g = gs->post_g2.as<uint32_t>();
    double *new_c = gs->post_c2.as<double>();
    grow_append_starts_kernel<<<nt / 256 + 1, 256>>>(keys2, n_dpost, nt, gs->term_start.as<uint32_t>(), new_start);
    if (n_dpost)
        grow_append_post_kernel<<<(n_dpost + 255) / 256, 256>>>(keys2, vals2, n_dpost, g0, ix->term_s0.as<double>(), ix->s1.as<double>(), fn,
                                                                gs->term_start.as<uint32_t>(), ins, new_g, new_c);
    if (gs->n_post)
        grow_append_move_kernel<<<(gs->n_post + 256 * GA_ITEMS - 1) / (256 * GA_ITEMS), 256>>>(gs->post_g.as<uint32_t>(), gs->post_c.as<double>(),
                                                                                             gs->n_post, ins, n_dpost, new_g, new_c);
    HIP_TRY(hipGetLastError());
    // 5. the tile tables of the new n_tiles
    uint32_t n_tab = 0;
    grow_append_flag_kernel<<<nt / 256 + 1, 256>>>(new_start, nt, n_tiles, flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(at(o_scan), scan_tb, flags, offs, (int)(nt + 1u)));
    HIP_TRY(hipMemcpy(&n_tab, offs + nt, 4, hipMemcpyDeviceToHost));
    if ((rc = reserve_spare(gs->tab2, 4ull * n_tab))) return rc;
    if (nt) grow_append_tabidx_kernel<<<(nt + 255) / 256, 256>>>(flags, offs, nt, n_tiles, gs->tab_idx2.as<uint32_t>(), tterm);
    if (n_tab) grow_append_tab_kernel<<<(n_tab + 255) / 256, 256>>>(tterm, n_tab, n_tiles, new_start, new_g, gs->tab2.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> start_host(nt + 1ull);
    HIP_TRY(hipMemcpy(start_host.data(), new_start, 4ull * (nt + 1ull), hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    // the new segment
    swap_buffers(gs->term_start, gs->term_start2);
    swap_buffers(gs->post_g, gs->post_g2);
    swap_buffers(gs->post_c, gs->post_c2);
    swap_buffers(gs->tab_idx, gs->tab_idx2);
    swap_buffers(gs->tab, gs->tab2);
    if (new_payload.p) swap_buffers(gs->payload, new_payload);
    gs->term_start_host.swap(start_host);
    gs->n_grow = n_new;
    gs->n_tiles = n_tiles;
    gs->n_post = n_post;
    return VBM25_OK;
}

static int device_growing_append_impl(vbm25_device_growing *gs, const vbm25_growing_desc *d) {
    if (!gs || !d) return set_error(VBM25_ERR_INVALID, "NULL argument");
    uint64_t e_first = 0, n_el = 0;
    if (int rc = growing_desc_check(gs->index, d, gs->n_grow, gs->n_post, &e_first, &n_el)) return rc;
    return device_growing_append_core(gs, d, e_first, n_el, hipMemcpyHostToDevice);
}

// vbm25_device_growing_append_documents: the delta is a cast's arrays in HBM.  Its keys are strictly ascending inside a document and
// its start is monotone by construction; the checks of growing_desc_check that read no element data apply.
static int device_growing_append_documents_impl(vbm25_device_growing *gs, const vbm25_documents *h) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return set_error(VBM25_ERR_DEVICE, "no HIP device: the growing segment has no host fallback");
    if (!gs || !h) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (h->device != gs->device) return set_error(VBM25_ERR_INVALID, "the documents are on device %d, the segment on device %d", h->device, gs->device);
    if (!h->has_payload) return set_error(VBM25_ERR_INVALID, "the documents were cast without payloads: a growing segment needs them");
    const vbm25_index *ix = gs->index;
    if (uint64_t(ix->n_docs) + gs->n_grow + h->n_docs > (1ull << 32))
        return set_error(VBM25_ERR_INVALID, "%u sealed + %llu growing documents exceed 2^32: the doc id ranges would collide", ix->n_docs,
                         (unsigned long long)gs->n_grow + h->n_docs);
    if (gs->n_post + h->n_elements >= (1ull << 31))
        return set_error(VBM25_ERR_UNSUPPORTED, "%llu growing elements: the device path takes fewer than 2^31", (unsigned long long)(gs->n_post + h->n_elements));
    // CAUTION: this desc's pointers are in HBM.  It exists only to be handed to device_growing_append_core with
    // hipMemcpyDeviceToDevice, which passes them to hipMemcpy and reads none on the host; nothing else may take it.
    vbm25_growing_desc d{};
    d.n_docs = h->n_docs;
    d.n_elements = h->n_elements;
    d.start = h->d_start.as<uint64_t>();
    d.key = h->d_key.as<uint8_t>();
    d.tf = h->d_tf.as<uint32_t>();
    d.fieldnorm = h->d_fieldnorm.as<uint8_t>();
    d.payload = h->d_payload.as<uint16_t>();
    d.deleted = nullptr;
    return device_growing_append_core(gs, &d, 0, h->n_elements, hipMemcpyDeviceToDevice);
}

static int device_growing_delete_impl(vbm25_device_growing *gs, const uint32_t *g, uint32_t n) {
    if (!gs || (!g && n)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    for (uint32_t i = 0; i < n; ++i)
        if (g[i] >= gs->n_grow) return set_error(VBM25_ERR_INVALID, "index %u: growing document %u of %u", i, g[i], gs->n_grow);
    if (!n || !gs->n_post) return VBM25_OK;
    if (int rc = use_device(gs->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (runs in flight read the old scores to their end)
    const size_t o_bits = (4ull * n + 255u) & ~size_t(255), bit_bytes = 4ull * ((gs->n_grow + 31u) / 32u);
    const int rc = reserve_spare(gs->stage, o_bits + bit_bytes);
    gs->count_bytes();
    if (rc) return rc;
    uint32_t *idx = gs->stage.as<uint32_t>(), *bits = reinterpret_cast<uint32_t *>(gs->stage.as<uint8_t>() + o_bits);
    HIP_TRY(hipMemcpy(idx, g, 4ull * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(bits, 0, bit_bytes));
    grow_delete_bits_kernel<<<uint32_t((uint64_t(n) + 255) / 256), 256>>>(idx, n, bits);
    grow_delete_kernel<<<(gs->n_post + 255) / 256, 256>>>(gs->post_g.as<uint32_t>(), gs->n_post, bits, gs->post_c.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return VBM25_OK;
}

// vbm25_device_growing_delete_tids (tid.hip): the deletion bitmap is already in HBM on the segment's device (bit g % 32 of word g / 32,
// what grow_delete_bits_kernel writes), the caller has waited for the device and the current device is the segment's.  Enqueues
// grow_delete_kernel; the caller synchronises.
int growing_delete_by_bits(vbm25_device_growing *gs, const uint32_t *bits) {
    if (!gs->n_post) return VBM25_OK;
    grow_delete_kernel<<<(gs->n_post + 255) / 256, 256>>>(gs->post_g.as<uint32_t>(), gs->n_post, bits, gs->post_c.as<double>());
    HIP_TRY(hipGetLastError());
    return VBM25_OK;
}

}  // namespace vbm25

using namespace vbm25;

extern "C" {

int vbm25_growing_upload(vbm25_index *ix, const vbm25_growing_desc *d, vbm25_device_growing **out) {
    return guarded([&] { return vbm25_growing_upload_impl(ix, d, out); });
}
void vbm25_device_growing_free(vbm25_device_growing *gs) {
    if (!gs) return;
    (void)hipSetDevice(gs->device);
    delete gs;
}
uint64_t vbm25_device_growing_bytes(const vbm25_device_growing *gs) { return gs ? gs->device_bytes : 0; }
uint32_t vbm25_device_growing_docs(const vbm25_device_growing *gs) { return gs ? gs->n_grow : 0; }
int vbm25_device_growing_append(vbm25_device_growing *gs, const vbm25_growing_desc *delta) {
    return guarded([&] { return device_growing_append_impl(gs, delta); });
}
int vbm25_device_growing_append_documents(vbm25_device_growing *gs, const vbm25_documents *documents) {
    return guarded([&] { return device_growing_append_documents_impl(gs, documents); });
}
int vbm25_device_growing_delete(vbm25_device_growing *gs, const uint32_t *g, uint32_t n) {
    return guarded([&] { return device_growing_delete_impl(gs, g, n); });
}

}  // extern "C"
