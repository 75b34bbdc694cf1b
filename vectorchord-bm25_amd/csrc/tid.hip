// tid.hip -- vbm25_tid_set: a set of ctids in HBM, and which documents of a payload plane it names.  bulkdelete.rs:20-112 calls
// callback(payload) for every growing and every sealed document and search.rs:122,230 filter(payload) the same way; what PostgreSQL
// holds in both cases is a set of TIDs (VACUUM's dead-TID store, the TID bitmap of a bitmap heap scan).  Here the set is sorted keys
// with a directory of evenly spaced keys, and the question is one kernel over a payload plane whose answer is one bit a document in
// the packing the filters and the deletion words use: a wave of 64 lanes answers exactly one uint64_t word with one ballot.
//   tid_pack_kernel    n x 3 uint16_t -> n 48-bit keys (tid_lane.h: tid_key)
//   (hipcub)           radix sort on the 48 bits, unique
//   tid_dir_kernel     the directory: dir_shape's entries, entry j = key dir_source(j, stride)
//   tid_match_kernel   wave w takes documents 64 w .. 64 w + 63: three u16 loads a lane (the wave's 384 bytes are contiguous),
//                      tid_contains with the directory staged in LDS once per workgroup, a ballot, and lane 0 writes the word:
//                      stored, stored and counted, or ORed into the word that is there with the new bits counted.  A wave adds
//                      its count with one atomic at its end.  Grid-stride over the words under the tid_grid cap.
//   tid_bytes_kernel   match words ORed into a plane of one deleted byte a document (the vacuum handle's growing flags)
// The consumers: the match calls, vbm25_filter_set_tids, vbm25_device_growing_delete_tids, vbm25_device_vacuum_bulkdelete.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "vbm25_internal.h"
#include "device_segment.h"
#include "host_objects.h"
#include "tid_lane.h"

struct vbm25_tid_set {
    int device = 0;
    uint64_t n_keys = 0;       // sorted, distinct
    uint32_t n_dir = 0, stride = 1;
    vbm25::DeviceBuffer keys;  // n_keys x 8
    vbm25::DeviceBuffer dir;   // n_dir x 8
};

namespace vbm25 {

using namespace tid;

namespace {

constexpr uint32_t WG = 256, WAVES = WG / 64, MAX_GRID = 2048;
enum MatchMode : uint32_t { STORE = 0, STORE_COUNT = 1, OR_COUNT = 2 };

// tid_grid and tid_dir of vbm25_tuning_set: tid_grid is read by each launch of the match kernel, tid_dir by each vbm25_tid_set_create
std::atomic<uint32_t> g_tid_grid{MAX_GRID}, g_tid_dir{DEFAULT_DIR_LOG2};

__global__ void __launch_bounds__(WG) tid_pack_kernel(const uint16_t *tids, uint64_t n, unsigned long long *keys) {
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * WG) keys[i] = tid_key(tids + 3 * i);
}

__global__ void __launch_bounds__(WG) tid_dir_kernel(const unsigned long long *keys, uint32_t n_dir, uint32_t stride, unsigned long long *dir) {
    const uint32_t j = blockIdx.x * WG + threadIdx.x;
    if (j < n_dir) dir[j] = keys[dir_source(j, stride)];
}

struct MatchArgs {
    const uint16_t *payload;            // n x 3
    uint32_t n;                         // documents of the plane
    const unsigned long long *dir;      // the set
    const unsigned long long *keys;
    uint64_t n_keys;
    uint32_t n_dir, stride;
    unsigned long long *words;          // ceil(n / 64)
    unsigned long long invert;          // 0 or ~0
    uint32_t mode;
    uint32_t *count;                    // STORE_COUNT: the set bits; OR_COUNT: the bits that were not set before (NULL with STORE)
};

__global__ void __launch_bounds__(WG) tid_match_kernel(MatchArgs a) {
    extern __shared__ unsigned long long s_dir[];
    for (uint32_t i = threadIdx.x; i < a.n_dir; i += WG) s_dir[i] = a.dir[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, n_words = (uint32_t)(((uint64_t)a.n + 63u) >> 6);
    uint32_t counted = 0;
    // whole waves take a word each: every lane of a wave is in every round, the ballot reads them all
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < n_words; w += (uint64_t)gridDim.x * WAVES) {
        const uint64_t d = (w << 6) + lane;
        bool hit = false;
        if (d < a.n) {
            const uint16_t *p = a.payload + 3 * d;
            const uint16_t p3[3] = {p[0], p[1], p[2]};
            hit = tid_contains(tid_key(p3), (const uint64_t *)s_dir, a.n_dir, (const uint64_t *)a.keys, a.n_keys, a.stride);
        }
        const uint64_t word = match_word(__ballot(hit), w << 6, a.n, a.invert);
        if (lane == 0) {  // (one lane's vector store)
            if (a.mode == OR_COUNT) {
                const uint64_t old = a.words[w];
                counted += new_bits(old, word);
                if (word & ~old) a.words[w] = old | word;
            } else {
                a.words[w] = word;
                counted += popcount64(word);
            }
        }
    }
    if (lane == 0 && counted && a.mode != STORE) atomicAdd(a.count, counted);
}

// words: ceil(n / 64) match words; deleted: n bytes, != 0 = deleted.  A matched document that was live is flagged and counted.
__global__ void __launch_bounds__(WG) tid_bytes_kernel(const unsigned long long *words, uint32_t n, uint8_t *deleted, uint32_t *count) {
    const uint64_t g = (uint64_t)blockIdx.x * WG + threadIdx.x;
    bool fresh = false;
    if (g < n && ((words[g >> 6] >> (g & 63u)) & 1ull) && deleted[g] == 0) {
        deleted[g] = 1;
        fresh = true;
    }
    const uint64_t m = __ballot(fresh);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(count, (uint32_t)__popcll(m));
}

int no_device(const char *what) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return set_error(VBM25_ERR_DEVICE, "no HIP device: %s", what);
    return VBM25_OK;
}

// the match of one payload plane against the set, enqueued on the null stream of the current device (the set's)
void match_launch(const vbm25_tid_set *s, const uint16_t *payload, uint32_t n, unsigned long long *words, bool invert, uint32_t mode,
                  uint32_t *count) {
    const uint32_t n_words = (uint32_t)(((uint64_t)n + 63u) / 64u);
    if (!n_words) return;
    MatchArgs a{payload, n, s->dir.as<unsigned long long>(), s->keys.as<unsigned long long>(), s->n_keys, s->n_dir, s->stride, words,
                invert ? ~0ull : 0ull, mode, count};
    const uint32_t cap = std::max(1u, g_tid_grid.load());
    tid_match_kernel<<<grid_for(n_words, WAVES, cap), WG, 8ull * std::max(1u, s->n_dir)>>>(a);
}

thread_local double g_match_ms = 0.0;  // the last vbm25_tid_set_match_index / _match_growing of this thread: its kernel between two events

int tid_set_create_impl(int device, const uint16_t *tids, uint64_t n, vbm25_tid_set **out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n > 0xffffffffull) return set_error(VBM25_ERR_UNSUPPORTED, "%llu TIDs: a set takes at most 2^32 - 1", (unsigned long long)n);
    if (n && !tids) return set_error(VBM25_ERR_INVALID, "tids is NULL");
    if (int rc = no_device("a TID set lives on the device")) return rc;
    if (int rc = use_device(device)) return rc;
    auto s = std::make_unique<vbm25_tid_set>();
    s->device = device;
    const uint32_t dir_log2 = g_tid_dir.load();
    int rc = 0;
    if (n) {
        DeviceBuffer raw, packed, sorted, tmp, d_count;
        if ((rc = raw.upload(tids, 6ull * n)) || (rc = packed.alloc(8ull * n)) || (rc = sorted.alloc(8ull * n)) || (rc = d_count.alloc(8)))
            return rc;
        tid_pack_kernel<<<grid_for(n, WG, 4096), WG>>>(raw.as<uint16_t>(), n, packed.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) {
            return hipcub::DeviceRadixSort::SortKeys(t, tb, packed.as<unsigned long long>(), sorted.as<unsigned long long>(), (uint64_t)n, 0, 48);
        }));
        // (the packed keys are done with: the distinct ones go where they were)
        HIP_TRY(with_cub_temp(tmp, [&](void *t, size_t &tb) {
            return hipcub::DeviceSelect::Unique(t, tb, sorted.as<unsigned long long>(), packed.as<unsigned long long>(),
                                                d_count.as<unsigned long long>(), (int64_t)n);
        }));
        unsigned long long n_unique = 0;
        HIP_TRY(hipMemcpy(&n_unique, d_count.p, 8, hipMemcpyDeviceToHost));
        s->n_keys = n_unique;
        if (n_unique == n) {
            std::swap(s->keys.p, packed.p);
            std::swap(s->keys.bytes, packed.bytes);
        } else {  // repeats: the set keeps what it needs
            if ((rc = s->keys.alloc(8ull * n_unique))) return rc;
            HIP_TRY(hipMemcpy(s->keys.p, packed.p, 8ull * n_unique, hipMemcpyDeviceToDevice));
        }
    } else if ((rc = s->keys.alloc(0))) {
        return rc;
    }
    const DirShape shape = dir_shape(s->n_keys, dir_log2);
    s->n_dir = shape.n_dir;
    s->stride = shape.stride;
    if ((rc = s->dir.alloc(8ull * s->n_dir))) return rc;
    if (s->n_dir)
        tid_dir_kernel<<<(s->n_dir + WG - 1) / WG, WG>>>(s->keys.as<unsigned long long>(), s->n_dir, s->stride, s->dir.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    *out = s.release();
    return VBM25_OK;
}

int tid_set_read_impl(const vbm25_tid_set *s, uint16_t *tids) {
    if (!s || (!tids && s->n_keys)) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (!s->n_keys) return VBM25_OK;
    if (int rc = use_device(s->device)) return rc;
    std::vector<uint64_t> keys(s->n_keys);
    HIP_TRY(hipMemcpy(keys.data(), s->keys.p, 8ull * s->n_keys, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < s->n_keys; ++i) {
        tids[3 * i] = uint16_t(keys[i] >> 32);
        tids[3 * i + 1] = uint16_t(keys[i] >> 16);
        tids[3 * i + 2] = uint16_t(keys[i]);
    }
    return VBM25_OK;
}

// one payload plane of `n` documents on `device` against the set: words and the count to the host
int match_plane(const vbm25_tid_set *s, int device, const char *what, const uint16_t *payload, uint32_t n, uint64_t *words, uint32_t *n_match) {
    if (s->device != device) return set_error(VBM25_ERR_INVALID, "the TID set is on device %d, the %s on device %d", s->device, what, device);
    if (n_match) *n_match = 0;
    const uint64_t n_words = ((uint64_t)n + 63u) / 64u;
    if (!n_words) return VBM25_OK;
    if (int rc = use_device(device)) return rc;
    DeviceBuffer d_words, d_count;
    int rc = 0;
    if ((rc = d_words.alloc(8ull * n_words)) || (rc = d_count.alloc(4))) return rc;
    HIP_TRY(hipMemsetAsync(d_count.p, 0, 4));
    Event ev[2];
    for (Event &e : ev) HIP_TRY(e.create());
    HIP_TRY(hipEventRecord(ev[0].e, nullptr));
    match_launch(s, payload, n, d_words.as<unsigned long long>(), false, STORE_COUNT, d_count.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1].e, nullptr));
    if (words) HIP_TRY(hipMemcpy(words, d_words.p, 8ull * n_words, hipMemcpyDeviceToHost));
    if (n_match) HIP_TRY(hipMemcpy(n_match, d_count.p, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0].e, ev[1].e));
    g_match_ms = ms;
    return VBM25_OK;
}

int tid_set_match_index_impl(const vbm25_tid_set *s, const vbm25_index *ix, uint64_t *words, uint32_t *n_match) {
    if (!s || !ix) return set_error(VBM25_ERR_INVALID, "NULL argument");
    return match_plane(s, ix->device, "index", ix->doc_payload.as<uint16_t>(), ix->n_docs, words, n_match);
}

int tid_set_match_growing_impl(const vbm25_tid_set *s, const vbm25_device_growing *gs, uint64_t *words, uint32_t *n_match) {
    if (!s || !gs) return set_error(VBM25_ERR_INVALID, "NULL argument");
    return match_plane(s, gs->device, "growing segment", gs->payload.as<uint16_t>(), gs->n_grow, words, n_match);
}

int filter_set_tids_impl(vbm25_filter *f, uint32_t i, const vbm25_tid_set *s, int invert, const vbm25_device_growing *gs) {
    if (!f || !s) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (i >= f->n_bitmaps) return set_error(VBM25_ERR_INVALID, "bitmap %u of a filter of %u", i, f->n_bitmaps);
    if (s->device != f->device) return set_error(VBM25_ERR_INVALID, "the TID set is on device %d, the filter on device %d", s->device, f->device);
    if (gs) {  // the pairing rules and codes of vbm25_batch_set_filter
        if (gs->index != f->index) return set_error(VBM25_ERR_INVALID, "the growing segment belongs to another index");
        if (!f->grow_serial) return set_error(VBM25_ERR_UNSUPPORTED, "a growing segment was given and the filter has no growing bitmaps");
        if (f->grow_serial != gs->serial)
            return set_error(VBM25_ERR_INVALID, "the filter's growing bitmaps belong to another upload than this segment");
        if (int rc = filter_growing_count_check(f, gs)) return rc;
    }
    if (int rc = use_device(f->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (runs in flight read the old bits to their end)
    match_launch(s, f->index->doc_payload.as<uint16_t>(), f->index->n_docs, f->bits.as<unsigned long long>() + size_t(i) * f->words, invert != 0,
                 STORE, nullptr);
    // (the growing words at or beyond ceil(n_grow / 64), up to the stride, are zero and stay so)
    if (gs) match_launch(s, gs->payload.as<uint16_t>(), gs->n_grow, f->grow_bits.as<unsigned long long>() + size_t(i) * f->grow_stride, invert != 0,
                         STORE, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return VBM25_OK;
}

int growing_delete_tids_impl(vbm25_device_growing *gs, const vbm25_tid_set *s, uint32_t *n_match) {
    if (!gs || !s) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (s->device != gs->device) return set_error(VBM25_ERR_INVALID, "the TID set is on device %d, the growing segment on device %d", s->device, gs->device);
    if (n_match) *n_match = 0;
    if (!gs->n_grow) return VBM25_OK;
    if (int rc = use_device(gs->device)) return rc;
    const uint64_t n_words = ((uint64_t)gs->n_grow + 63u) / 64u;
    DeviceBuffer d_words, d_count;
    int rc = 0;
    if ((rc = d_words.alloc(8ull * n_words)) || (rc = d_count.alloc(4))) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (runs in flight read the old scores to their end)
    HIP_TRY(hipMemsetAsync(d_count.p, 0, 4));
    match_launch(s, gs->payload.as<uint16_t>(), gs->n_grow, d_words.as<unsigned long long>(), false, STORE_COUNT, d_count.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    // bit g % 32 of the 32-bit word g / 32 is bit g % 64 of the 64-bit word g / 64: the bitmap grow_delete_bits_kernel writes
    if ((rc = growing_delete_by_bits(gs, d_words.as<uint32_t>()))) return rc;
    if (n_match) HIP_TRY(hipMemcpy(n_match, d_count.p, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return VBM25_OK;
}

int vacuum_bulkdelete_impl(vbm25_device_vacuum *dv, const vbm25_index *ix, const vbm25_tid_set *s, uint32_t *n_sealed_new, uint32_t *n_grow_new) {
    if (!dv || !ix || !s) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_sealed_new) *n_sealed_new = 0;
    if (n_grow_new) *n_grow_new = 0;
    if (ix->device != dv->device)
        return set_error(VBM25_ERR_INVALID, "the compaction inputs are on device %d, the index on device %d", dv->device, ix->device);
    if (ix->n_docs != dv->n_sealed)
        return set_error(VBM25_ERR_INVALID, "the compaction inputs are of %u sealed documents, the index holds %u", dv->n_sealed, ix->n_docs);
    if (s->device != dv->device)
        return set_error(VBM25_ERR_INVALID, "the TID set is on device %d, the compaction inputs on device %d", s->device, dv->device);
    if (int rc = use_device(dv->device)) return rc;
    // every allocation before the first word changes
    const uint64_t g_words = ((uint64_t)dv->n_grow + 63u) / 64u;
    DeviceBuffer d_gwords, d_count;
    int rc = 0;
    if ((rc = d_gwords.alloc(8ull * g_words)) || (rc = d_count.alloc(8))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemsetAsync(d_count.p, 0, 8));
    match_launch(s, ix->doc_payload.as<uint16_t>(), dv->n_sealed, dv->d_sealed_deleted.as<unsigned long long>(), false, OR_COUNT,
                 d_count.as<uint32_t>());
    if (dv->n_grow) {
        match_launch(s, dv->d_payload.as<uint16_t>(), dv->n_grow, d_gwords.as<unsigned long long>(), false, STORE, nullptr);
        tid_bytes_kernel<<<(dv->n_grow + WG - 1) / WG, WG>>>(d_gwords.as<unsigned long long>(), dv->n_grow, dv->d_deleted.as<uint8_t>(),
                                                             d_count.as<uint32_t>() + 1);
    }
    HIP_TRY(hipGetLastError());
    uint32_t fresh[2] = {0, 0};
    HIP_TRY(hipMemcpy(fresh, d_count.p, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    dv->n_sealed_deleted += fresh[0];
    dv->n_grow_deleted += fresh[1];
    if (n_sealed_new) *n_sealed_new = fresh[0];
    if (n_grow_new) *n_grow_new = fresh[1];
    return VBM25_OK;
}

}  // namespace

int tid_tuning_set(const char *name, long long value) {
    const std::string n(name);
    if (n == "tid_grid") g_tid_grid.store(uint32_t(std::min<long long>(std::max(1ll, value), MAX_GRID)));
    else if (n == "tid_dir") g_tid_dir.store(uint32_t(std::min<long long>(std::max(0ll, value), MAX_DIR_LOG2)));
    else return set_error(VBM25_ERR_INVALID, "unknown tuning switch %s", name);
    return VBM25_OK;
}
uint32_t tid_dir_now() { return g_tid_dir.load(); }
uint32_t tid_grid_now() { return std::max(1u, g_tid_grid.load()); }
void tid_set_view(const vbm25_tid_set *s, TidSetView *out) {
    *out = TidSetView{s->device, s->n_keys, s->n_dir, s->stride, s->keys.as<unsigned long long>(), s->dir.as<unsigned long long>()};
}
void tid_tuning_reset() {
    g_tid_grid.store(MAX_GRID);
    g_tid_dir.store(DEFAULT_DIR_LOG2);
}

}  // namespace vbm25

using namespace vbm25;

extern "C" {

int vbm25_tid_set_create(int device, const uint16_t *tids, uint64_t n, vbm25_tid_set **out) {
    const int rc = guarded([&] { return tid_set_create_impl(device, tids, n, out); });
    if (rc && out) *out = nullptr;
    return rc;
}
int vbm25_tid_set_info(const vbm25_tid_set *s, uint64_t *n_unique, int *device) {
    if (!s) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (n_unique) *n_unique = s->n_keys;
    if (device) *device = s->device;
    return VBM25_OK;
}
int vbm25_tid_set_read(const vbm25_tid_set *s, uint16_t *tids) {
    return guarded([&] { return tid_set_read_impl(s, tids); });
}
uint64_t vbm25_tid_set_device_bytes(const vbm25_tid_set *s) { return s ? s->keys.footprint() + s->dir.footprint() : 0; }
void vbm25_tid_set_free(vbm25_tid_set *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}
int vbm25_tid_set_match_index(const vbm25_tid_set *s, const vbm25_index *ix, uint64_t *words, uint32_t *n_match) {
    return guarded([&] { return tid_set_match_index_impl(s, ix, words, n_match); });
}
int vbm25_tid_set_match_growing(const vbm25_tid_set *s, const vbm25_device_growing *gs, uint64_t *words, uint32_t *n_match) {
    return guarded([&] { return tid_set_match_growing_impl(s, gs, words, n_match); });
}
int vbm25_filter_set_tids(vbm25_filter *f, uint32_t i, const vbm25_tid_set *s, int invert, const vbm25_device_growing *gs) {
    return guarded([&] { return filter_set_tids_impl(f, i, s, invert, gs); });
}
int vbm25_device_growing_delete_tids(vbm25_device_growing *gs, const vbm25_tid_set *s, uint32_t *n_match) {
    return guarded([&] { return growing_delete_tids_impl(gs, s, n_match); });
}
int vbm25_device_vacuum_bulkdelete(vbm25_device_vacuum *dv, const vbm25_index *ix, const vbm25_tid_set *s, uint32_t *n_sealed_new,
                                   uint32_t *n_grow_new) {
    return guarded([&] { return vacuum_bulkdelete_impl(dv, ix, s, n_sealed_new, n_grow_new); });
}

// The last vbm25_tid_set_match_index / _match_growing of this thread (tools/tid_cost.py; not part of the ABI): ms of tid_match_kernel between HIP events
int vbm25_debug_tid_match_ms(double *out) {
    if (!out) return set_error(VBM25_ERR_INVALID, "NULL argument");
    *out = g_match_ms;
    return VBM25_OK;
}

}  // extern "C"
