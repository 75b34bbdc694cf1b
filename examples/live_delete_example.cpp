// live_delete_example.cpp -- a DELETE reaches the rerank stack through the C++ host API: an index built from documents, its forward index
// (Index::bind) and a vbm25::Reranker made with vbm25::from_index; the rows are reranked by ctid; then a row is deleted
// (DocTerms::erase with a vbm25::TidSet, the set the growing segment's and the filters' deletes take) and drops out of the rerank; then
// its ctid is inserted again -- PostgreSQL hands a dead tuple's ctid out again -- appended (DocTerms::append) and synced
// (Reranker::sync), and the ctid names the new row.  Nothing is bound, cast or sorted a second time.
//   g++ -std=c++17 -Iinclude examples/live_delete_example.cpp -Lvectorchord-bm25_amd/csrc -lvbm25 -o /tmp/live_delete_example
// Prints the rows of each step, the scores as hexadecimal floats; tests/test_cpp_live_delete_mirror.py compares them with the Python
// mirror's.
#include <cstdio>
#include <string>

#include "vbm25.hpp"

int main() {
    try {
        vbm25::Seed seed{};
        for (size_t i = 0; i < seed.size(); ++i) seed[i] = uint8_t(7 + i);
        // the documents of examples/live_rerank_example.cpp: document d over 12 lexemes; `at` is the row's ctid (0, at, 1)
        auto lexeme = [](int j) { return j % 3 ? "t" + std::to_string(j) : "a-lexeme-of-the-long-kind-" + std::to_string(j); };
        auto rows = [&](int first, int end, int at) {
            vbm25::DocumentBatch batch;
            for (int d = first; d < end; ++d) {
                for (int j = 0; j < 12; ++j)
                    if ((d + j) % (2 + j % 3) == 0) batch.add(lexeme(j), uint32_t(1 + (d * 7 + j) % 4));
                const uint16_t ctid[3] = {0, uint16_t(at + d - first), 1};
                batch.end_document(ctid);
            }
            return batch;
        };
        const int n_sealed = 40, victim = 7;
        vbm25::Documents sealed(0, &seed, rows(0, n_sealed, 0));
        vbm25::DeviceSegment segment = vbm25::DeviceSegment::from_documents(sealed, 1.2, 0.75);
        vbm25::Index index(segment.handle());
        vbm25::Resolver resolver(index, &seed, 1, 8, 64, 4096);
        vbm25::DocTerms bound = index.bind();
        vbm25::Reranker ring(bound, resolver, vbm25::from_index, 2, 8, 64, 4096, 1024, 16);
        vbm25::LexemeBatch queries;
        for (const char *t : {"t1", "t2", "unknown"}) queries.add(t);
        queries.end_query();
        queries.add(lexeme(0));
        queries.add("t4");
        queries.end_query();
        // both queries rerank rows 5 .. 9 by ctid; (9, 9, 9) names no row and keeps its position
        std::vector<uint16_t> tids;
        for (int d = 5; d < 10; ++d) tids.insert(tids.end(), {0, uint16_t(d), 1});
        tids.insert(tids.end(), {9, 9, 9});
        const uint64_t n = tids.size() / 3;
        std::vector<uint16_t> both(tids);
        both.insert(both.end(), tids.begin(), tids.end());
        std::vector<vbm25_rank> ranks;
        std::vector<uint32_t> n_ranks;
        auto rerank = [&](const char *step) {
            ring.submit_tids(queries, 8, {0, n, 2 * n}, both);
            const uint32_t k = ring.collect(ranks, n_ranks);
            std::printf("%s: %u documents, %u dead, directory %u\n", step, bound.docs(), bound.dead_docs(), ring.directory_docs());
            for (size_t q = 0; q < n_ranks.size(); ++q)
                for (uint32_t i = 0; i < k; ++i)
                    std::printf("row %s %zu %u %u %u %u %a\n", step, q, i, n_ranks[q], ranks[q * k + i].pos, ranks[q * k + i].doc, ranks[q * k + i].score);
        };
        rerank("bound");
        // DELETE of row 7, by its ctid
        vbm25::TidSet gone(std::vector<uint16_t>{0, uint16_t(victim), 1});
        const uint32_t n_new = bound.erase(gone);
        std::printf("deleted %u, word 0 of the bitmap %llx\n", n_new, (unsigned long long)bound.read_dead()[0]);
        rerank("deleted");
        // INSERT: document 40 arrives at the dead row's ctid
        vbm25::Documents delta(0, &seed, rows(n_sealed, n_sealed + 1, victim));
        bound.append(delta, resolver);
        rerank("appended");  // (not yet synced: the directory does not know the row)
        ring.sync();
        rerank("synced");
        // the same row again by its index: nobody was alive
        const uint32_t again[2] = {uint32_t(victim), uint32_t(victim)};
        std::printf("deleted again %u, dead %u\n", bound.erase(again, 2), bound.dead_docs());
    } catch (const vbm25::Error &e) {
        std::printf("error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
