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
};
hipError_t launch_row_gram(const GramArgs& a, hipStream_t s);
bool valid_map(const SlabMap& m, int64_t p);  // the geometry a kernel may rely on (pgh_kernels.hip)

}  // namespace pgh
