// live_rerank_example.cpp -- the rerank stack follows a live table through the C++ host API: an index built from documents, its forward
// index (Index::bind) and a vbm25::Reranker made with vbm25::from_index; then three rounds of INSERTs -- each delta is cast once,
// appended to the growing segment (what the search reads) and to the bound handle (DocTerms::append), the reranker's ctid directory
// takes the new rows (Reranker::sync), and the rows are reranked by ctid.  Nothing is bound, cast or sorted a second time.
//   g++ -std=c++17 -Iinclude examples/live_rerank_example.cpp -Lvectorchord-bm25_amd/csrc -lvbm25 -o /tmp/live_rerank_example
// Prints the rows of the new documents, the scores as hexadecimal floats; tests/test_cpp_live_rerank_mirror.py compares them with the
// Python mirror's.
#include <cstdio>
#include <memory>
#include <string>

#include "vbm25.hpp"

int main() {
    try {
        vbm25::Seed seed{};
        for (size_t i = 0; i < seed.size(); ++i) seed[i] = uint8_t(7 + i);
        // the documents of examples/forward_example.cpp, continued: document d over 12 lexemes at ctid (0, d, 1)
        auto lexeme = [](int j) { return j % 3 ? "t" + std::to_string(j) : "a-lexeme-of-the-long-kind-" + std::to_string(j); };
        auto rows = [&](int first, int end) {
            vbm25::DocumentBatch batch;
            for (int d = first; d < end; ++d) {
                for (int j = 0; j < 12; ++j)
                    if ((d + j) % (2 + j % 3) == 0) batch.add(lexeme(j), uint32_t(1 + (d * 7 + j) % 4));
                const uint16_t ctid[3] = {0, uint16_t(d), 1};
                batch.end_document(ctid);
            }
            return batch;
        };
        const int n_sealed = 40;
        vbm25::Documents sealed(0, &seed, rows(0, n_sealed));
        vbm25::DeviceSegment segment = vbm25::DeviceSegment::from_documents(sealed, 1.2, 0.75);
        vbm25::Index index(segment.handle());
        vbm25::Resolver resolver(index, &seed, 1, 8, 64, 4096);
        vbm25::DocTerms bound = index.bind();
        vbm25::Reranker ring(bound, resolver, vbm25::from_index, 2, 8, 64, 4096, 1024, 16);
        std::unique_ptr<vbm25::DeviceGrowing> growing;
        vbm25::LexemeBatch queries;
        for (const char *t : {"t1", "t2", "unknown"}) queries.add(t);
        queries.end_query();
        queries.add(lexeme(0));
        queries.add("t4");
        queries.end_query();
        std::vector<vbm25_rank> ranks;
        std::vector<uint32_t> n_ranks;
        const int cuts[4] = {40, 41, 50, 70};  // three rounds of INSERTs: 1, 9 and 20 rows
        for (int round = 0; round < 3; ++round) {
            const int first = cuts[round], end = cuts[round + 1];
            vbm25::Documents delta(0, &seed, rows(first, end));
            if (growing) growing->append(delta);
            else growing = std::make_unique<vbm25::DeviceGrowing>(index, delta.download());
            bound.append(delta, resolver);
            ring.sync();
            std::printf("round %d: %u documents, %u sealed, %u growing, directory %u\n", round, bound.docs(), bound.base_docs(), growing->docs(),
                        ring.directory_docs());
            // every query reranks the new rows and one sealed row, by ctid; (9, 9, 9) names no row and keeps its position
            std::vector<uint16_t> tids;
            for (int d = first; d < end; ++d) tids.insert(tids.end(), {0, uint16_t(d), 1});
            tids.insert(tids.end(), {9, 9, 9, 0, 7, 1});
            const uint64_t n = uint64_t(end - first) + 2;
            std::vector<uint16_t> both(tids);
            both.insert(both.end(), tids.begin(), tids.end());
            ring.submit_tids(queries, 4, {0, n, 2 * n}, both);
            const uint32_t k = ring.collect(ranks, n_ranks);
            for (size_t q = 0; q < n_ranks.size(); ++q)
                for (uint32_t i = 0; i < k; ++i)
                    std::printf("row %d %zu %u %u %u %u %a\n", round, q, i, n_ranks[q], ranks[q * k + i].pos, ranks[q * k + i].doc, ranks[q * k + i].score);
        }
    } catch (const vbm25::Error &e) {
        std::printf("error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
