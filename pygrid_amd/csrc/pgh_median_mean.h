// Internal launcher interface of kernel K15 (pgh_median_mean.hip), beside pgh_kernels.h.  Not installed.
#pragma once
#include "pgh_kernels.h"

namespace pgh {

// MODE_MEAN_AROUND_MEDIAN (the definition is in include/pgh_api.h): out = ckpt - the mean of the `keep` values
// nearest the median, per param.  K15 launch_median_mean (pgh_median_mean.hip): one pass over HBM with K9's tile,
// row sources and tiers, wave w holding the fold positions 64 w .. 64 w + 63 in register order -- a block of the
// definition's sum.  The median as in K9; the distance key e = bits(x - m) & 0x7fffffff derived from the one
// register array wherever it is read; the keep-th smallest e by a 31-step bisection; ties at it kept in fold
// order through per-wave tie counts in LDS; the kept values added in f64, a block per wave, the blocks left to
// right.  1 <= keep <= n_rows <= MEDIAN_NCHIP.
constexpr int MODE_MEAN_AROUND_MEDIAN = 8;
struct MedianMeanArgs {
    const float* diffs;      // the slab at row 0 (a table) or at the first row
    SlabMap map;             // map.off = shard param of local column 0
    int n_rows;
    int keep;                // n_rows - the drop count
    int64_t p;               // params of the launch
    const int32_t* d_rows;   // the launcher's: Rows::d_rows on its way to the kernel
    const float* ckpt;       // [p]
    float* out;              // [p]
};
hipError_t launch_median_mean(const MedianMeanArgs& a, const Rows& rows, hipStream_t s);
bool valid_map(const SlabMap& m, int64_t p);  // the geometry a kernel may rely on (pgh_kernels.hip)

}  // namespace pgh
