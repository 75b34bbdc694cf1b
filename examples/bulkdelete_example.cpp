// bulkdelete_example.cpp -- a set of heap rows matched against payloads on the device, through the C++ host API: 150 sealed documents
// and 70 growing ones, a TID set of every fifth row of both plus rows the table never held, the sealed and the growing match words,
// a filter bitmap made from the set (plain and inverted) and the growing segment's delete by TID.
//   g++ -std=c++17 -Iinclude examples/bulkdelete_example.cpp -Lvectorchord-bm25_amd/csrc -lvbm25 -o /tmp/bulkdelete_example
// Prints the words; tests/test_cpp_tid_mirror.py compares them with the Python mirror's.
#include <cstdio>
#include <string>

#include "vbm25.hpp"

static const int N_SEALED = 150, N_GROW = 70;

// row r of the table: block r / 7, offset r % 7 + 1
static void ctid_of(int r, uint16_t (&ctid)[3]) {
    ctid[0] = 0, ctid[1] = uint16_t(r / 7), ctid[2] = uint16_t(r % 7 + 1);
}

static void add_document(vbm25::DocumentBatch &b, int r) {
    for (int j = 0; j < 1 + r % 4; ++j) b.add("t" + std::to_string((r * 3 + j) % 11), uint32_t(1 + j));
    uint16_t ctid[3];
    ctid_of(r, ctid);
    b.end_document(ctid);
}

static void print_words(const char *what, const std::vector<uint64_t> &w) {
    std::printf("%s", what);
    for (uint64_t x : w) std::printf(" %016llx", (unsigned long long)x);
    std::printf("\n");
}

int main() {
    try {
        vbm25::DocumentBatch sealed, growing;
        for (int r = 0; r < N_SEALED; ++r) add_document(sealed, r);
        for (int r = N_SEALED; r < N_SEALED + N_GROW; ++r) add_document(growing, r);
        vbm25::DeviceSegment segment = vbm25::DeviceSegment::from_documents(vbm25::Documents(0, nullptr, sealed), 1.2, 0.75);
        vbm25::Index index(segment.handle());
        vbm25::DeviceGrowing grow(index, vbm25::Documents(0, nullptr, growing).download());

        // the dead rows: every fifth, listed twice and backwards, and twenty the table never held
        std::vector<uint16_t> tids;
        for (int pass = 0; pass < 2; ++pass)
            for (int r = N_SEALED + N_GROW + 19; r >= 0; --r)
                if (r % 5 == 0 || r >= N_SEALED + N_GROW) {
                    uint16_t ctid[3];
                    ctid_of(r, ctid);
                    tids.insert(tids.end(), ctid, ctid + 3);
                }
        vbm25::TidSet set(tids);
        std::printf("set %llu distinct of %zu, device %d, %s\n", (unsigned long long)set.size(), tids.size() / 3, set.device(),
                    set.device_bytes() >= 8 * set.size() ? "bytes ok" : "BYTES SHORT");
        const std::vector<uint16_t> back = set.read();
        std::printf("first %u %u %u last %u %u %u\n", back[0], back[1], back[2], back[back.size() - 3], back[back.size() - 2], back[back.size() - 1]);

        uint32_t n_sealed = 0, n_grow = 0;
        print_words("sealed", set.match(index, N_SEALED, &n_sealed));
        print_words("growing", set.match(grow, &n_grow));
        std::printf("matched %u sealed %u growing\n", n_sealed, n_grow);

        vbm25::DocFilter filter(index, 2);
        filter.set_growing(&grow);
        filter.set_tids(0, set, false, &grow);
        filter.set_tids(1, set, true, &grow);
        for (uint32_t i = 0; i < 2; ++i) {
            print_words(i ? "filter 1 sealed" : "filter 0 sealed", filter.read(i, vbm25::DocFilter::words_per_bitmap(N_SEALED)));
            print_words(i ? "filter 1 growing" : "filter 0 growing", filter.read(i, vbm25::DocFilter::words_per_bitmap(N_GROW), true));
        }
        try {
            filter.set_tids(2, set);
        } catch (const vbm25::Error &e) {
            std::printf("refused: %s\n", e.what());
        }
        std::printf("deleted by TID: %u matched\n", grow.erase(set));
        return 0;
    } catch (const vbm25::Error &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
