// hip_host.h -- the host plumbing around every kernel launch of libvbm25, once: the error macro, the owners of an HBM allocation, of
// pinned host memory, of a stream and of an event, the tally of what a handle took at create, launch-grid and layout arithmetic, and
// the hipcub calling convention.
// Host-side and HIP-only: every .hip translation unit includes it (device_segment.h does so for them) and defines none of this
// itself; the lane and parse headers that plain g++ compiles for the harnesses under tests/native/ must not.  Not part of the ABI.
#ifndef VBM25_HIP_HOST_H
#define VBM25_HIP_HOST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "vbm25_internal.h"

// In a function that returns the library's int codes: a failed HIP call becomes VBM25_ERR_DEVICE and the thread's error text
#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return vbm25::set_error(VBM25_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr,        \
                                    hipGetErrorString(e_), __FILE__, __LINE__);              \
    } while (0)

namespace vbm25 {

// The one owner of a hipMalloc.  `bytes` is the size asked for (capacity arithmetic relies on it); a zero-length request still
// allocates 16 bytes, so `p` is never NULL after a successful alloc.  alloc() on an array that holds memory leaks it: release() first.
struct HbmArray {
    void *p = nullptr;
    size_t bytes = 0;
    HbmArray() = default;
    HbmArray(const HbmArray &) = delete;
    HbmArray &operator=(const HbmArray &) = delete;
    ~HbmArray() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) {
        bytes = n;
        return hipMalloc(&p, n ? n : 16);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // what the allocation takes of the device: `bytes`, or the 16 of a zero-length request
    size_t footprint() const { return !p ? 0 : bytes ? bytes : 16; }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

struct PinnedHost {
    void *p = nullptr;
    PinnedHost() = default;
    PinnedHost(const PinnedHost &) = delete;
    PinnedHost &operator=(const PinnedHost &) = delete;
    ~PinnedHost() {
        if (p) (void)hipHostFree(p);
    }
    // (a zero-length request still allocates 16 bytes, as HbmArray's.)  alloc() on a block that holds memory leaks it.
    hipError_t alloc(size_t n) { return hipHostMalloc(&p, n ? n : 16, hipHostMallocDefault); }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    // a stream of the handle's or the call's own, which waits for no other: work on the null stream would wait for every stream of the device
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() { return hipEventCreate(&e); }  // (with timing)
};

// Waits for a stream when it goes out of scope.  Declared behind a call's buffers and its Stream, so destroyed before them: nothing is
// freed, and the stream is not destroyed, under a kernel or a copy in flight.  (s == NULL: nothing to wait for.)
struct Quiesce {
    hipStream_t s = nullptr;
    Quiesce() = default;
    explicit Quiesce(hipStream_t stream) : s(stream) {}
    Quiesce(const Quiesce &) = delete;
    Quiesce &operator=(const Quiesce &) = delete;
    ~Quiesce() {
        if (s) (void)hipStreamSynchronize(s);
    }
};

// What a handle that allocates nothing per call took at create: every allocation and creation of such a handle goes through its
// tally.  `allocations` is their number, `device_bytes` the footprint of the HBM arrays the handle keeps (kept = false: a temporary
// of create, counted as an allocation and freed before create returns).
struct ResourceTally {
    uint64_t allocations = 0, device_bytes = 0;
    hipError_t device_alloc(HbmArray &a, size_t n, bool kept = true) {
        ++allocations;
        const hipError_t e = a.alloc(n);
        if (e == hipSuccess && kept) device_bytes += a.footprint();
        return e;
    }
    hipError_t pinned_alloc(PinnedHost &h, size_t n) {
        ++allocations;
        return h.alloc(n);
    }
    hipError_t stream_create(Stream &st) {
        ++allocations;
        return st.create();
    }
    hipError_t event_create(Event &ev) {
        ++allocations;
        return ev.create();
    }
};

// the device time between two events of a stream, both reached (a collected slot's start and done)
inline hipError_t elapsed_ms(const Event &from, const Event &to, double *ms) {
    float f = 0;
    const hipError_t e = hipEventElapsedTime(&f, from.e, to.e);
    *ms = f;
    return e;
}

static_assert(!std::is_copy_constructible_v<HbmArray> && !std::is_copy_assignable_v<HbmArray>, "an owner is never copied");
static_assert(!std::is_copy_constructible_v<PinnedHost> && !std::is_copy_assignable_v<PinnedHost>, "an owner is never copied");
static_assert(!std::is_copy_constructible_v<Stream> && !std::is_copy_assignable_v<Stream>, "an owner is never copied");
static_assert(!std::is_copy_constructible_v<Event> && !std::is_copy_assignable_v<Event>, "an owner is never copied");
static_assert(!std::is_copy_constructible_v<Quiesce> && !std::is_copy_assignable_v<Quiesce>, "an owner is never copied");

// u32 -> u64 under a hipcub::TransformInputIterator: sums that a 32-bit scan would wrap
struct WidenU32 {
    __host__ __device__ unsigned long long operator()(uint32_t v) const { return v; }
};

// blocks for `units` of work at `per_block` a block: at least one, at most max_grid (the kernels stride the grid beyond it)
inline uint32_t grid_for(uint64_t units, uint32_t per_block, uint32_t max_grid) {
    return (uint32_t)std::min<uint64_t>(max_grid, std::max<uint64_t>(1, (units + per_block - 1) / per_block));
}
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline int use_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return VBM25_OK;
}

// The hipcub calling convention, the argument list written once: `call(tmp, bytes)` runs one hipcub device-wide function on its
// temporary storage.  Asked with NULL for the size; `tmp` (whatever it held is released first) allocated to it; then run.
template <class Call>
hipError_t with_cub_temp(HbmArray &tmp, Call &&call) {
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e != hipSuccess) return e;
    tmp.release();
    if ((e = tmp.alloc(bytes)) != hipSuccess) return e;
    return call(tmp.p, bytes);
}

}  // namespace vbm25

#endif
