// Internal launcher interface of kernel K16 (pgh_gram.hip), beside pgh_kernels.h.  Not installed.
#pragma once
#include "pgh_kernels.h"

namespace pgh {

// K16: the Gram matrix of the listed rows on the matrix cores (the definition is in include/pgh_api.h):
// G[a][b] = sum over i < p of (double)d_a[i] * (double)d_b[i] for list indices a, b of the n listed rows, every
// product exact, accumulated in f64 by v_mfma_f64_16x16x4_f64.  List index k is slab row d_rows[k] (a device table
// of n entries) or, without a table, row0 + k.  The output is cut into blocks of GRAM_RB list positions; block
// pair q = (A, B), B >= A, counted A-major (A = 0: B = 0, 1, ..; A = 1: B = 1, 2, ..).  The params are cut into
// chunks of chunk_tiles whole SUMSQ_TILE tiles.  A workgroup owns one (chunk, block pair): it walks its params
// in steps of GRAM_KSTEP and writes its GRAM_RB x GRAM_RB partial block to part[(chunk * nbp + (q - bp0))][i][j]
// (places at or past n, and in a diagonal pair the 16 x 16 tiles below the diagonal, are not written).  One
// launch takes the block pairs [bp0, bp0 + nbp) over every chunk and then folds each of their entries over the
// chunks in chunk order into gram[a * n + b] and gram[b * n + a]: the caller sizes `part` for nbp block pairs and
// batches them.  The accumulation order of an entry depends on (p, n, a, b) alone.
constexpr int GRAM_RB = 128;
constexpr int GRAM_KSTEP = 32;
constexpr int GRAM_TARGET_WGS = 4096;
inline int gram_blocks(int n) { return (n + GRAM_RB - 1) / GRAM_RB; }
inline int gram_block_pairs(int n) { return gram_blocks(n) * (gram_blocks(n) + 1) / 2; }
// Tiles per chunk, a function of (p, n) alone: about GRAM_TARGET_WGS workgroups over all block pairs, so the
// partials of all of them stay near GRAM_TARGET_WGS blocks (512 MiB) whatever n and the model.
inline int64_t gram_chunk_tiles(int64_t ntiles, int n) {
    const int64_t ct = ntiles * gram_block_pairs(n) / GRAM_TARGET_WGS;
    return ct < 1 ? 1 : ct;
}
struct GramArgs {
    const float* slab;       // the slab at row 0
    SlabMap map;             // map.off = 0
    int64_t p;               // params in the shard
    const int32_t* d_rows;   // [n] slab rows in list order, or null: row0 + k
    int row0;
    int n;                   // rows in the list, 1 .. PAIRDIST_MAX_ROWS
    int bp0, nbp;            // the launch's block pairs
    int64_t chunk_tiles;     // gram_chunk_tiles(ntiles, n)
    int nchunks;             // ceil(ntiles / chunk_tiles)
    double* part;            // [nchunks][nbp][GRAM_RB * GRAM_RB]
    double* gram;            // [n][n]
    const double* sums;      // K20 alone: K7's sums by slab row, the row scales (gram_row_exp); null for K16
};
hipError_t launch_row_gram(const GramArgs& a, hipStream_t s);
// What both Gram kernels (K16; K20, pgh_gram_bf16.hip) share: the check of a launch's arguments, and the fold of
// the launch's partial blocks over the chunks in chunk order into both triangles of `gram`.  With a.sums the
// folded entry is scaled by 2^(e_a + e_b) first (K20's row scales); without, it is stored as it is.
hipError_t check_row_gram(const GramArgs& a);
hipError_t launch_row_gram_fold(const GramArgs& a, hipStream_t s);
bool valid_map(const SlabMap& m, int64_t p);  // the geometry a kernel may rely on (pgh_kernels.hip)

#ifdef __HIP__
// slab row of list position k (SRC 2: through the device table)
template <int SRC>
__device__ __forceinline__ size_t gram_row_at(const GramArgs& a, int k) {
    if constexpr (SRC == 2) return (size_t)(uint32_t)a.d_rows[k];
    else return (size_t)(a.row0 + k);
}

// block pair q of nblk blocks -> (A, B), A-major (uniform: a short scalar loop)
__device__ __forceinline__ void gram_pair(int q, int nblk, int* A, int* B) {
    int x = 0;
    while (q >= nblk - x) {
        q -= nblk - x;
        ++x;
    }
    *A = x;
    *B = x + q;
}

// K20's row scale: the integer e with 2^e <= sqrt(s) < 2^(e + 1) from the exponent field of the f64 sum of
// squares s (floor of half the unbiased exponent); 0 where s is 0 or not finite.  (A sum of squares of f32 values
// is never subnormal in f64: an exponent field of 0 is the zero.)
__device__ __forceinline__ int gram_row_exp(double s) {
    const int be = (int)(((uint64_t)__double_as_longlong(s) >> 52) & 0x7ffu);
    return be == 0 || be == 0x7ff ? 0 : (be - 1023) >> 1;
}
#endif

}  // namespace pgh
