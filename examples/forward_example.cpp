// forward_example.cpp -- the rerank stack on an index's own documents through the C++ host API: an index arrives without its tsvectors
// (here: built on the device, its documents dropped), Index::bind makes the forward index from what the index holds in HBM, and a
// vbm25::Reranker made with vbm25::from_index reranks ctids of the indexed table -- the hybrid-search step behind a vector index.
//   g++ -std=c++17 -Iinclude examples/forward_example.cpp -Lvectorchord-bm25_amd/csrc -lvbm25 -o /tmp/forward_example
// Prints the forward index and every score as a hexadecimal float; tests/test_cpp_forward_mirror.py compares them with the Python mirror's.
#include <cstdio>
#include <memory>
#include <string>

#include "vbm25.hpp"

int main() {
    try {
        vbm25::Seed seed{};
        for (size_t i = 0; i < seed.size(); ++i) seed[i] = uint8_t(7 + i);
        // the documents of examples/rerank_ring_example.cpp: 40 over 12 lexemes, document d at ctid (0, d, 1)
        auto lexeme = [](int j) { return j % 3 ? "t" + std::to_string(j) : "a-lexeme-of-the-long-kind-" + std::to_string(j); };
        std::unique_ptr<vbm25::Index> index;
        {
            vbm25::DocumentBatch batch;
            for (int d = 0; d < 40; ++d) {
                for (int j = 0; j < 12; ++j)
                    if ((d + j) % (2 + j % 3) == 0) batch.add(lexeme(j), uint32_t(1 + (d * 7 + j) % 4));
                const uint16_t ctid[3] = {0, uint16_t(d), 1};
                batch.end_document(ctid);
            }
            vbm25::Documents sealed(0, &seed, batch);
            vbm25::DeviceSegment segment = vbm25::DeviceSegment::from_documents(sealed, 1.2, 0.75);
            index = std::make_unique<vbm25::Index>(segment.handle());
        }  // the documents and the segment are gone: the index is all there is
        vbm25::Resolver resolver(*index, &seed, 1, 8, 64, 4096);
        vbm25::DocTerms bound = index->bind();
        std::vector<uint64_t> start;
        std::vector<uint32_t> term, tf;
        bound.download(start, term, tf);
        std::printf("forward %u documents %llu postings\n", bound.docs(), (unsigned long long)bound.known());
        for (uint32_t d = 0; d < bound.docs(); ++d) {
            std::printf("doc %u:", d);
            for (uint64_t i = start[d]; i < start[d + 1]; ++i) std::printf(" %u:%u", term[i], tf[i]);
            std::printf("\n");
        }
        vbm25::Reranker ring(bound, resolver, vbm25::from_index, 2, 8, 64, 4096, 1024, 16);
        vbm25::LexemeBatch queries;
        for (const char *t : {"t1", "t2", "unknown"}) queries.add(t);
        queries.end_query();
        queries.add(lexeme(0));
        queries.add("t4");
        queries.end_query();
        queries.end_query();  // (a query without lexemes)
        // ctids of the table: (9, 9, 9) names no row and keeps its position
        ring.submit_tids(queries, 3, {0, 4, 6, 7}, {0, 7, 1, 0, 0, 1, 9, 9, 9, 0, 39, 1, 0, 39, 1, 0, 2, 1, 0, 2, 1});
        ring.submit(queries, 3);
        std::vector<vbm25_rank> ranks;
        std::vector<uint32_t> n_ranks;
        for (const char *tag : {"ring tids", "ring cross"}) {
            const uint32_t k = ring.collect(ranks, n_ranks);
            for (size_t q = 0; q < n_ranks.size(); ++q)
                for (uint32_t i = 0; i < k; ++i)
                    std::printf("%s %zu %u %u %u %u %a\n", tag, q, i, n_ranks[q], ranks[q * k + i].pos, ranks[q * k + i].doc, ranks[q * k + i].score);
        }
        // a handle bound from documents has no ctids of an index
        try {
            vbm25::DocumentBatch one;
            one.add("t1", 1);
            const uint16_t ctid[3] = {0, 1, 1};
            one.end_document(ctid);
            vbm25::Documents rows(0, &seed, one);
            vbm25::DocTerms from_rows = rows.bind(resolver);
            vbm25::Reranker refused(from_rows, resolver, vbm25::from_index, 2, 8, 64, 4096, 1024, 16);
        } catch (const vbm25::Error &e) {
            std::printf("documents-bound handle: error %d\n", e.code);
        }
    } catch (const vbm25::Error &e) {
        std::printf("error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
