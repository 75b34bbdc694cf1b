// evaluate_lane.h -- the per-lane functions of the `<&>` operator on bound documents (evaluate.hip): bm25::evaluate (evaluate.rs:22-74)
// for ONE (query, document) pair in term-id space.  __host__ __device__, and plain C++ as well: the scoring kernel of evaluate.hip is
// a loop over score_step, and tests/native/fuzz_evaluate.cpp compiles the same text with g++ under AddressSanitizer against
// std::lower_bound and a plain merge walk.
//
//   bisect_run   the first position of a document's ascending id run that holds an id >= the probe, and whether it holds the probe.
//                A position is read only while lo < hi: an empty run (a document without known elements, a lane without a candidate)
//                reads nothing, whatever its bounds are.
//   term_score   idf * tf() of one posting: Cache::evaluate's expression (bm25.rs:291-295, 355-358) as vbm25_evaluate_batch writes it
//   score_step   one query term against one document: the bisection from the cursor the previous term left (query ids ascend, so
//                every later term lies behind it), the posting's tf, the add.  Absent terms add nothing.
//   pair_score   the whole query against one document: score_step per term in query order, ids >= n_terms skipped -- the sum order is
//                the query's key order by construction
#ifndef VBM25_EVALUATE_LANE_H
#define VBM25_EVALUATE_LANE_H

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EVL_HD __host__ __device__ __forceinline__
#else
#define EVL_HD inline __attribute__((always_inline))
#endif

namespace vbm25 {
namespace evl {

// run = term[lo .. hi), strictly ascending.  Returns the first p in [lo, hi] with p == hi or term[p] >= id; found = (p < hi and
// term[p] == id).
EVL_HD uint32_t bisect_run(const uint32_t *term, uint32_t lo, uint32_t hi, uint32_t id, bool &found) {
    found = false;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t v = term[mid];
        if (v < id) {
            lo = mid + 1;
        } else {
            hi = mid;
            found = v == id;  // (the last move of hi decides: lo ends on it)
            if (found) lo = mid;
        }
    }
    return lo;
}

EVL_HD double term_score(double idf, uint32_t tf_count, double k1p1, double s1) {
    const double tf = double(tf_count);
    const double tfv = (tf * k1p1) / (tf + s1);
    return idf * tfv;
}

// cursor: in/out, the run's first position that may still hold an id >= this term's
EVL_HD void score_step(const uint32_t *term, const uint32_t *tf, uint32_t &cursor, uint32_t hi, uint32_t id, double idf, double k1p1, double s1,
                       double &result) {
    bool found;
    cursor = bisect_run(term, cursor, hi, id, found);
    if (found) result += term_score(idf, tf[cursor], k1p1, s1);
}

EVL_HD double pair_score(const uint32_t *term, const uint32_t *tf, uint32_t lo, uint32_t hi, const uint32_t *q_ids, uint32_t n_q, uint32_t n_terms,
                         const double *term_idf, double k1p1, double s1) {
    double result = 0.0;
    uint32_t cursor = lo;
    for (uint32_t i = 0; i < n_q; ++i) {
        const uint32_t id = q_ids[i];
        if (id >= n_terms) continue;
        score_step(term, tf, cursor, hi, id, term_idf[id], k1p1, s1, result);
    }
    return result;
}

}  // namespace evl
}  // namespace vbm25

#endif
