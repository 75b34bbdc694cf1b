// scan_sparse_big_launch.h -- what search.hip sees of scan_sparse_big.hip.  Included by both.
#ifndef VBM25_SCAN_SPARSE_BIG_LAUNCH_H
#define VBM25_SCAN_SPARSE_BIG_LAUNCH_H

#include "device_types.h"

namespace vbm25 {

// stats: four counters the kernel adds to (items taken, items given up, slow-path tiles, cuts), zeroed by plan_kernel
hipError_t scan_sparse_big_launch(const DevIndex &ix, const DevBatch &bt, uint32_t *stats, uint32_t grid, hipStream_t st);
uint32_t scan_sparse_big_max_terms();  // indexed terms per query
uint32_t scan_sparse_big_grid();       // persistent workgroups of a full grid: two per CU

}  // namespace vbm25

#endif
