// ring.h -- the cursor of a first-in-first-out ring of `depth` slots, once: which slot the next submit takes, which slot the next
// collect releases, how many are in flight.  Every pipelined handle (vbm25_stream, vbm25_resolver, vbm25_caster, vbm25_reranker)
// holds one beside its slots.  Plain C++ without HIP: tests/native/ring_cursor.cpp compiles it with g++ alone.  What a handle says
// when its ring is full or empty, and its last_collected, stay with the handle.
#ifndef VBM25_RING_H
#define VBM25_RING_H

#include <cstdint>

namespace vbm25 {

struct RingCursor {
    uint32_t depth = 0;  // slots; set once, at create
    uint32_t head = 0;   // the oldest slot in flight
    uint32_t count = 0;  // slots in flight
    bool full() const { return count == depth; }
    bool empty() const { return count == 0; }
    // the slot the next submit takes (asked for when not full)
    uint32_t tail() const {
        const uint32_t t = head + count;  // (head < depth and count <= depth <= 2^31: no wrap of the sum)
        return t >= depth ? t - depth : t;
    }
    // tail() is in flight now.  The caller has checked !full().
    void push() { ++count; }
    // the oldest slot leaves the ring: its index.  The caller has checked !empty().
    uint32_t pop() {
        const uint32_t released = head;
        head = head + 1 == depth ? 0 : head + 1;
        --count;
        return released;
    }
};

}  // namespace vbm25

#endif
