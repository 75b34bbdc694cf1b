// ring_cursor.cpp -- csrc/ring.h under AddressSanitizer + UBSan on the CPU: the cursor every pipelined handle keeps beside its slots,
// against a std::deque of the slot indices in flight.  A stand-alone program (tests/test_ring_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/ring_cursor.cpp -o ring_cursor && ./ring_cursor
// Every depth 1 .. 16, STEPS random steps each: a push when the ring is empty, a pop when it is full, otherwise either -- leaning to
// pushes and to pops in turns, so that the ring runs full and runs empty again and again.  A push must take the slot behind the one
// pushed before it (the slots are taken round and round), a pop must release the deque's front, and full(), empty(), count and head
// must agree with the deque after every step.  Each depth ends after its cursor has gone round at least 50 times.
#include <cstdint>
#include <cstdio>
#include <deque>
#include <random>

#include "../../vectorchord-bm25_amd/csrc/ring.h"

using vbm25::RingCursor;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            if (++failures > 20) return 1;                   \
        }                                                    \
    } while (0)

constexpr uint32_t STEPS = 4000;

static int run_depth(uint32_t depth, std::mt19937 &rng, uint64_t *cases) {
    RingCursor ring;
    ring.depth = depth;
    std::deque<uint32_t> in_flight;  // the model: slot indices, the oldest in front
    uint64_t pushes = 0, pops = 0, times_full = 0, times_empty = 0;
    CHECK(ring.empty() && !ring.full() && ring.tail() == 0, "depth %u: a fresh cursor", depth);
    for (uint32_t step = 0; step < STEPS; ++step) {
        const bool lean_push = (step / (4 * depth + 3)) % 2 == 0;
        const bool push = in_flight.empty() || (in_flight.size() < depth && rng() % 10 < (lean_push ? 7u : 3u));
        if (push) {
            const uint32_t slot = ring.tail();
            CHECK(slot == pushes % depth, "depth %u step %u: tail() is %u, the slot behind the last push is %u", depth, step, slot,
                  uint32_t(pushes % depth));
            ring.push();
            in_flight.push_back(slot);
            ++pushes;
        } else {
            CHECK(ring.head == in_flight.front(), "depth %u step %u: head is %u, the oldest in flight is %u", depth, step, ring.head, in_flight.front());
            const uint32_t released = ring.pop();
            CHECK(released == in_flight.front(), "depth %u step %u: pop() released %u, the oldest in flight is %u", depth, step, released,
                  in_flight.front());
            in_flight.pop_front();
            ++pops;
        }
        CHECK(ring.count == in_flight.size(), "depth %u step %u: count is %u, %zu are in flight", depth, step, ring.count, in_flight.size());
        CHECK(ring.full() == (in_flight.size() == depth), "depth %u step %u: full() with %zu in flight", depth, step, in_flight.size());
        CHECK(ring.empty() == in_flight.empty(), "depth %u step %u: empty() with %zu in flight", depth, step, in_flight.size());
        CHECK(ring.head < depth && ring.depth == depth, "depth %u step %u: head is %u", depth, step, ring.head);
        if (!in_flight.empty()) CHECK(ring.head == in_flight.front(), "depth %u step %u: head is %u, the oldest in flight is %u", depth, step, ring.head, in_flight.front());
        times_full += ring.full();
        times_empty += ring.empty();
        ++*cases;
    }
    CHECK(pops >= 50ull * depth, "depth %u: %llu pops, the cursor went round fewer than 50 times", depth, (unsigned long long)pops);
    CHECK(times_full >= 10 && times_empty >= 10, "depth %u: full %llu times, empty %llu times", depth, (unsigned long long)times_full,
          (unsigned long long)times_empty);
    return 0;
}

int main() {
    std::mt19937 rng(20260417u);
    uint64_t cases = 0;
    for (uint32_t depth = 1; depth <= 16; ++depth)
        if (run_depth(depth, rng, &cases)) return 1;
    std::printf("%llu cases\n", (unsigned long long)cases);
    if (failures) return 1;
    std::printf("fuzz done\n");
    return 0;
}
