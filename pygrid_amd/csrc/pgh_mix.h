// Internal launcher interface of kernel K19 (pgh_mix.hip), beside pgh_gram.h.  Not installed.
#pragma once
#include "pgh_kernels.h"

namespace pgh {

// K19: the row mix Y = W X on the matrix cores (the definition is in include/pgh_api.h).  For destination list
// position i < m and param q < p:  out[d_dst[i]][q] = (float) sum over k < n, in increasing k, of
// w[i * n + k] * (double)x[d_src[k]][q], accumulated in f64 by v_mfma_f64_16x16x4_f64 from +0.0, four k at a
// time, no split over k.  d_src and d_dst are device tables of slab rows; the two lists share no row (the
// caller's check: the kernel reads the sources while it writes the destinations).  The output is cut into blocks
// of MIX_RB list positions by MIX_CB params, one workgroup each, the row block fastest in the grid; a workgroup
// walks all n sources in steps of MIX_KSTEP.  The accumulation order of an element depends on (n, k) alone.
constexpr int MIX_RB = 128;
constexpr int MIX_CB = 128;
constexpr int MIX_KSTEP = 16;
struct MixArgs {
    float* slab;             // the slab at row 0: sources read, destinations written
    SlabMap map;             // map.off = 0
    int64_t p;               // params in the shard
    const int32_t* d_src;    // [n] slab rows of the sources, list order
    int n;                   // 1 .. PAIRDIST_MAX_ROWS
    const int32_t* d_dst;    // [m] slab rows of the destinations
    int m;                   // 1 .. PAIRDIST_MAX_ROWS
    const double* w;         // [m][n] row-major, device
};
hipError_t launch_mix_rows(const MixArgs& a, hipStream_t s);
bool valid_map(const SlabMap& m, int64_t p);  // the geometry a kernel may rely on (pgh_kernels.hip)

}  // namespace pgh
