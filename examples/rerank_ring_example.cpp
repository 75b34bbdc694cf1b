// rerank_ring_example.cpp -- the rerank step as a pipelined ring through the C++ host API: lexeme queries and candidates go in as
// document indices, as ctids and as the cross product, three batches in flight on a vbm25::Reranker of three slots, and the 3 best
// rows a query come out first in first out.  The host never sees a term id.
//   g++ -std=c++17 -Iinclude examples/rerank_ring_example.cpp -Lvectorchord-bm25_amd/csrc -lvbm25 -o /tmp/rerank_ring_example
// Prints every score as a hexadecimal float; tests/test_cpp_reranker_mirror.py compares the rows with the Python mirror's.
#include <cstdio>
#include <string>

#include "vbm25.hpp"

int main() {
    try {
        vbm25::Seed seed{};
        for (size_t i = 0; i < seed.size(); ++i) seed[i] = uint8_t(7 + i);
        // the documents of examples/evaluate_example.cpp: 40 over 12 lexemes, document d at ctid (0, d, 1)
        auto lexeme = [](int j) { return j % 3 ? "t" + std::to_string(j) : "a-lexeme-of-the-long-kind-" + std::to_string(j); };
        vbm25::DocumentBatch batch;
        for (int d = 0; d < 40; ++d) {
            for (int j = 0; j < 12; ++j)
                if ((d + j) % (2 + j % 3) == 0) batch.add(lexeme(j), uint32_t(1 + (d * 7 + j) % 4));
            const uint16_t ctid[3] = {0, uint16_t(d), 1};
            batch.end_document(ctid);
        }
        vbm25::Documents sealed(0, &seed, batch);
        vbm25::DeviceSegment segment = vbm25::DeviceSegment::from_documents(sealed, 1.2, 0.75);
        vbm25::Index index(segment.handle());
        vbm25::Resolver resolver(index, &seed, 1, 8, 64, 4096);
        // the rows to rerank: the same documents and one more, which shares document 7's ctid
        batch.add("t1", 2);
        batch.add("not-in-the-index", 9);
        const uint16_t shared[3] = {0, 7, 1};
        batch.end_document(shared);
        vbm25::Documents rows(0, &seed, batch);
        vbm25::DocTerms bound = rows.bind(resolver);
        vbm25::Reranker ring(bound, resolver, 3, 8, 64, 4096, 1024, 16, &rows);
        const uint64_t made = ring.allocations();
        vbm25::LexemeBatch queries;
        for (const char *t : {"t1", "t2", "unknown"}) queries.add(t);
        queries.end_query();
        queries.add(lexeme(0));
        queries.add("t4");
        queries.end_query();
        queries.end_query();  // (a query without lexemes)
        const std::vector<uint64_t> q_cand{0, 3, 5, 6};
        ring.submit(queries, 3, q_cand, {40, 0, 7, 39, 39, 2});
        // the same lists as ctids; (0, 7, 1) names documents 7 and 40: the lower index; (9, 9, 9) names none
        ring.submit_tids(queries, 3, {0, 4, 6, 7}, {0, 7, 1, 0, 0, 1, 9, 9, 9, 0, 39, 1, 0, 39, 1, 0, 2, 1, 0, 2, 1});
        ring.submit(queries, 3);
        std::printf("in flight %d\n", ring.in_flight());
        std::vector<vbm25_rank> ranks;
        std::vector<uint32_t> n_ranks;
        for (const char *tag : {"ring listed", "ring tids", "ring cross"}) {
            const uint32_t k = ring.collect(ranks, n_ranks);
            for (size_t q = 0; q < n_ranks.size(); ++q)
                for (uint32_t i = 0; i < k; ++i)
                    std::printf("%s %zu %u %u %u %u %a\n", tag, q, i, n_ranks[q], ranks[q * k + i].pos, ranks[q * k + i].doc, ranks[q * k + i].score);
        }
        std::printf("allocations %s\n", ring.allocations() == made ? "unchanged" : "MOVED");
        try {
            ring.collect(ranks, n_ranks);
        } catch (const vbm25::Error &e) {
            std::printf("empty ring: error %d\n", e.code);
        }
    } catch (const vbm25::Error &e) {
        std::printf("error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
