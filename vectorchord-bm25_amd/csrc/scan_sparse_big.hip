// scan_sparse_big.hip -- translation unit of scan_sparse_big_kernel (scan_sparse_big.h) and the launcher search.hip calls.  A unit of
// its own: the kernel is compiled without packed f32 instructions (Makefile: UNIT_FLAGS), and nothing of it changes the code of the
// other scan kernels' units.
#include <hip/hip_runtime.h>

#include "vbm25_internal.h"
#include "scan_sparse_big.h"
#include "scan_sparse_big_launch.h"

namespace vbm25 {

hipError_t scan_sparse_big_launch(const DevIndex &ix, const DevBatch &bt, uint32_t *stats, uint32_t grid, hipStream_t st) {
    if (bt.k <= (uint32_t)REG_K || bt.k > dlist::MAX_K || bt.lpi != 1u || !ix.post_id16 || !ix.win_off || !ix.term_win || !ix.post_tfn)
        return hipErrorInvalidValue;
    scan_sparse_big_kernel<<<grid ? grid : 1u, SBWG, 0, st>>>(ix, bt, stats);
    return hipGetLastError();
}
uint32_t scan_sparse_big_max_terms() { return sbig::MAX_T; }
uint32_t scan_sparse_big_grid() { return SB_GRID; }

}  // namespace vbm25
