// caster_example.cpp -- the Document step as a ring through the C++ host API: 100 short documents cast in chunks of 0, 1, 64 and 35
// through a vbm25::Caster of two slots, the chunks appended to one handle with Documents::extend, and the one-shot cast of all of them
// beside it.
//   g++ -std=c++17 -Iinclude examples/caster_example.cpp -Lvectorchord-bm25_amd/csrc -lvbm25 -o /tmp/caster_example
// Prints the extended handle's arrays; tests/test_cpp_caster_mirror.py compares them with the Python mirror's one-shot cast.
#include <cstdio>
#include <string>

#include "vbm25.hpp"

static void add_document(vbm25::DocumentBatch &b, int d) {
    // document d: d % 7 lexemes over 9 (every third one of the hashed kind), one of them twice when d is odd
    auto lexeme = [](int j) { return j % 3 ? "t" + std::to_string(j) : "a-lexeme-of-the-long-kind-" + std::to_string(j); };
    for (int j = 0; j < d % 7; ++j) b.add(lexeme((d * 5 + j * 2) % 9), uint32_t(1 + (d + j) % 3));
    if (d % 2 && d % 7) b.add(lexeme((d * 5) % 9), 4);
    const uint16_t ctid[3] = {0, uint16_t(d), 1};
    b.end_document(ctid);
}

int main() {
    try {
        vbm25::Seed seed{};
        for (size_t i = 0; i < seed.size(); ++i) seed[i] = uint8_t(7 + i);
        vbm25::DocumentBatch all;
        for (int d = 0; d < 100; ++d) add_document(all, d);
        vbm25::Documents one_shot(0, &seed, all);

        vbm25::Caster caster(0, &seed, 2, 64, 512, 16384);
        const uint64_t allocations = caster.allocations(), held = caster.device_bytes();
        vbm25::Documents whole = vbm25::Documents::empty(0, true);
        const int chunks[4] = {0, 1, 64, 35};
        int next = 0, submitted = 0, collected = 0;
        auto submit = [&] {
            vbm25::DocumentBatch b;
            for (int i = 0; i < chunks[submitted]; ++i) add_document(b, next++);
            if (!chunks[submitted]) b.payload.assign(3, 0);  // (0 documents with payloads: a non-NULL pointer)
            caster.submit(b);
            ++submitted;
        };
        submit();
        while (collected < 4) {
            if (submitted < 4) submit();  // (two in flight while there is more to cast)
            vbm25::Documents part = caster.collect();
            std::printf("chunk %d %u documents %llu elements, %d in flight\n", collected, part.docs(), (unsigned long long)part.elements(), caster.in_flight());
            whole.extend(part);
            ++collected;
        }
        std::printf("caster allocations %s, device bytes %s\n", caster.allocations() == allocations ? "unchanged" : "MOVED",
                    caster.device_bytes() == held && held > 0 ? "unchanged" : "MOVED");
        std::vector<uint32_t> len, len1;
        const vbm25::GrowingDocs got = whole.download(&len), want = one_shot.download(&len1);
        const bool same = got.start == want.start && got.tf == want.tf && got.fieldnorm == want.fieldnorm && got.payload == want.payload && len == len1 &&
                          got.key == want.key;
        std::printf("extended %u documents %llu elements: %s\n", whole.docs(), (unsigned long long)whole.elements(), same ? "equal" : "DIFFERENT");
        for (size_t d = 0; d < got.size(); ++d) {
            std::printf("doc %zu %u %u", d, unsigned(got.fieldnorm[d]), len[d]);
            for (uint64_t e = got.start[d]; e < got.start[d + 1]; ++e) {
                std::printf(" ");
                for (uint8_t byte : got.key[e]) std::printf("%02x", byte);
                std::printf(":%u", got.tf[e]);
            }
            std::printf("\n");
        }
        try {
            whole.extend(whole);
        } catch (const vbm25::Error &e) {
            std::printf("refused: %s\n", e.what());
        }
        return same ? 0 : 1;
    } catch (const vbm25::Error &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
