// Internal launcher interface of kernel K17 (pgh_rank_trim.hip), beside pgh_kernels.h.  Not installed.
#pragma once
#include "pgh_kernels.h"

namespace pgh {

// MODE_RANK_TRIMMED (the definition is in include/pgh_api.h): out = ckpt - the mean of sort(values)[b : n - b],
// per param.  K17 launch_rank_trim (pgh_rank_trim.hip): one pass over HBM with K9's tile, row sources and tiers
// and K15's row mapping (wave w holds the fold positions 64 w .. 64 w + 63 in register order -- a block of the
// definition's sum).  Both boundary keys, L of rank b and H of rank n - 1 - b, come out of one 32-step bisection
// whose two counts per lane travel packed in one word; one more packed sweep counts the values up to L and below
// H; the values strictly between them are added in f64, a block per wave, the blocks left to right, and the
// boundary values go in as two products.  1 <= b, 2 b + 1 <= n_rows <= MEDIAN_NCHIP.
constexpr int MODE_RANK_TRIMMED = 9;
struct RankTrimArgs {
    const float* diffs;      // the slab at row 0 (a table) or at the first row
    SlabMap map;             // map.off = shard param of local column 0
    int n_rows;
    int b;                   // values dropped per side
    int64_t p;               // params of the launch
    const int32_t* d_rows;   // the launcher's: Rows::d_rows on its way to the kernel
    const float* ckpt;       // [p]
    float* out;              // [p]
};
hipError_t launch_rank_trim(const RankTrimArgs& a, const Rows& rows, hipStream_t s);
bool valid_map(const SlabMap& m, int64_t p);  // the geometry a kernel may rely on (pgh_kernels.hip)

}  // namespace pgh
