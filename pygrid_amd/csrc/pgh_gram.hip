// gfx950 (CDNA4, MI355X) kernel K16 of the cycle-close aggregation path.
//
// K16 k_row_gram  the Gram matrix G = X X^T of the listed slab rows in f64 on the matrix cores (Multi-Krum's
//       "gram" distances, cosine similarities; the definition is in include/pgh_api.h, the design in DESIGN.md
//       section 5); k_row_gram_fold finishes each entry over the chunks of the params and mirrors the triangle.
//
// A translation unit of its own, beside pgh_kernels.hip.  The product of two f32 values is exact in f64, so an
// entry is a sum of p exactly represented terms; only the accumulation rounds, and its order is fixed below.
//
// Work split.  The n x n output is cut into blocks of GRAM_RB = 128 list positions, only the block pairs (A, B)
// with B >= A are computed, and the params into chunks of whole 4,096-param tiles (pgh_gram.h).  A workgroup
// of 256 lanes owns one (chunk, block pair); the block pair runs fastest in the grid, so the workgroups that
// read one chunk's rows are neighbours in dispatch order and the re-reads come from L2 / Infinity Cache.
// Data path.  Per step of GRAM_KSTEP = 32 params the workgroup brings 128 A rows' and 128 B rows' segments
// (a diagonal pair: A alone) to LDS: lane l loads the 16-byte column l & 7 of rows (l >> 3) + 32 q, q = 0 .. 3,
// so eight lanes read one row's 128 contiguous bytes.  Params past p are masked to +0.0 before they reach LDS
// (the address clamps to the row's last column as in K7).  Two LDS buffers: the next step's global loads are
// issued before this step's MFMAs and stored behind them, one barrier per step.  The LDS row stride is 36
// floats, off the bank period.  Wave w owns the 64 x 64 sub-block (w >> 1, w & 1) as 4 x 4 MFMA tiles of
// 16 x 16: 64 f64 accumulators per lane.  Lane (r = l & 15, kk = l >> 4) of a wave reads the 16-byte column kk
// of row r of each of its four A and four B tiles from LDS (two reads of each per step), widens each float once
// and issues v_mfma_f64_16x16x4_f64 with element e of the column as its k = kk operand, e = 0 .. 3: the MFMA
// sums the four lanes' columns, so a step adds the params in the order e, kk within each half of the step.
// A wave whose sub-block lies past n, or below the diagonal of a diagonal pair, computes nothing; tiles past n
// and tiles below the diagonal are not stored.
// Result layout of the MFMA: register v of lane l holds entry (4 v + (l >> 4), l & 15) of the tile.
#include "pgh_gram.h"

namespace pgh {
namespace {

constexpr int BLOCK = 256;
constexpr int GRAM_LD = GRAM_KSTEP + 4;  // LDS row stride in floats: 144 bytes, a multiple of 16 and not of 128
constexpr int GRAM_BLK = GRAM_RB * GRAM_RB;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

static_assert(GRAM_RB == 128 && GRAM_KSTEP == 32 && BLOCK == 256, "K16: 4 waves of 64 x 64, 8 lanes a row, 4 rows a lane");
static_assert(SUMSQ_TILE % GRAM_KSTEP == 0, "K16: a chunk is whole steps");

template <int SRC>
__global__ __launch_bounds__(BLOCK) void k_row_gram(GramArgs a) {
    __shared__ __attribute__((aligned(16))) float sA[2][GRAM_RB][GRAM_LD];
    __shared__ __attribute__((aligned(16))) float sB[2][GRAM_RB][GRAM_LD];
    const int lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(lane >> 6);
    const int bpl = (int)(blockIdx.x % (unsigned)a.nbp), chunk = (int)(blockIdx.x / (unsigned)a.nbp);
    int A, B;
    gram_pair(a.bp0 + bpl, (a.n + GRAM_RB - 1) / GRAM_RB, &A, &B);
    const bool diag = A == B;
    const int na = min(GRAM_RB, a.n - A * GRAM_RB), nb = min(GRAM_RB, a.n - B * GRAM_RB);  // >= 1

    // ---- the global loads: 16-byte column lc of rows lr + 32 q; a short block repeats its last row ----
    const int lr = lane >> 3, lc = (lane & 7) * 4;
    const float* rowA[4];
    const float* rowB[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        rowA[q] = a.slab + gram_row_at<SRC>(a, A * GRAM_RB + min(lr + 32 * q, na - 1)) * (size_t)a.map.ld;
        rowB[q] = a.slab + gram_row_at<SRC>(a, B * GRAM_RB + min(lr + 32 * q, nb - 1)) * (size_t)a.map.ld;
    }
    const int64_t kbeg = (int64_t)chunk * a.chunk_tiles * SUMSQ_TILE;
    const int64_t kend = min(a.p, kbeg + a.chunk_tiles * SUMSQ_TILE);
    const int ns = (int)((kend - kbeg + GRAM_KSTEP - 1) / GRAM_KSTEP);  // >= 1: kbeg < p
    const int64_t last4 = (a.p - 1) & ~int64_t(3);
    f32x4 ga[4], gb[4];
    auto fetch = [&](int s) {
        const int64_t idx = kbeg + (int64_t)s * GRAM_KSTEP + lc;
        const int64_t off = a.map.at(min(idx, last4));
#pragma unroll
        for (int q = 0; q < 4; ++q) ga[q] = *reinterpret_cast<const f32x4*>(rowA[q] + off);
        if (!diag) {
#pragma unroll
            for (int q = 0; q < 4; ++q) gb[q] = *reinterpret_cast<const f32x4*>(rowB[q] + off);
        }
        if (idx + 4 > a.p) {  // the shard's last column or past it: masked to +0.0, whatever the padding holds
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (idx + e >= a.p) {
                        ga[q][e] = 0.f;
                        gb[q][e] = 0.f;
                    }
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(&sA[buf][lr + 32 * q][lc]) = ga[q];
        if (!diag) {
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(&sB[buf][lr + 32 * q][lc]) = gb[q];
        }
    };

    // ---- the wave's 4 x 4 MFMA tiles and which of them it computes ----
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 15, kk = (lane & 63) >> 4;
    unsigned live = 0;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
            const int r0 = wr * 64 + ti * 16, c0 = wc * 64 + tj * 16;
            if (r0 < na && c0 < nb && (!diag || c0 >= r0)) live |= 1u << (ti * 4 + tj);
        }
    live = (unsigned)__builtin_amdgcn_readfirstlane((int)live);
    f64x4 acc[4][4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f64x4{0.0, 0.0, 0.0, 0.0};

    auto compute = [&](int buf) {
        const float* pa = &sA[buf][wr * 64 + li][kk * 4];
        const float* pb = diag ? &sA[buf][wc * 64 + li][kk * 4] : &sB[buf][wc * 64 + li][kk * 4];
#pragma unroll
        for (int h = 0; h < GRAM_KSTEP / 16; ++h) {
            f32x4 af[4], bf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = *reinterpret_cast<const f32x4*>(pa + t * 16 * GRAM_LD + h * 16);
                bf[t] = *reinterpret_cast<const f32x4*>(pb + t * 16 * GRAM_LD + h * 16);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double ad[4], bd[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    ad[t] = (double)af[t][e];
                    bd[t] = (double)bf[t][e];
                }
#pragma unroll
                for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                    for (int tj = 0; tj < 4; ++tj)
                        acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[ti], bd[tj], acc[ti][tj], 0, 0, 0);
            }
        }
    };

    // ---- the steps: buffer s & 1 holds step s; step s + 1 is loaded ahead of the MFMAs and stored behind them ----
    fetch(0);
    stash(0);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
        const bool more = s + 1 < ns;  // (uniform)
        if (more) fetch(s + 1);
        if (live) compute(s & 1);  // (a wave with any tile to store computes all 16: no branch between the MFMAs)
        if (more) stash((s + 1) & 1);
        __syncthreads();
    }

    // ---- the partial block: register v of lane (li, kk) is entry (4 v + kk, li) of its tile ----
    double* part = a.part + ((size_t)chunk * (size_t)a.nbp + (size_t)bpl) * GRAM_BLK;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
            if (!((live >> (ti * 4 + tj)) & 1u)) continue;
            const int j = wc * 64 + tj * 16 + li;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = wr * 64 + ti * 16 + 4 * v + kk;
                if (i < na && j < nb) part[i * GRAM_RB + j] = acc[ti][tj][v];
            }
        }
}

// Every entry of the launch's block pairs with b >= a: its chunk partials left to right, one lane an entry (the
// lanes of a wave read 64 consecutive doubles of each chunk), written to both triangles.
__global__ __launch_bounds__(BLOCK) void k_row_gram_fold(GramArgs a) {
    constexpr int WGS = GRAM_BLK / BLOCK;  // workgroups a block
    const int bpl = (int)(blockIdx.x / WGS), e = (int)(blockIdx.x % WGS) * BLOCK + (int)threadIdx.x;
    int A, B;
    gram_pair(a.bp0 + bpl, (a.n + GRAM_RB - 1) / GRAM_RB, &A, &B);
    const int ia = A * GRAM_RB + e / GRAM_RB, ib = B * GRAM_RB + e % GRAM_RB;
    if (ia >= a.n || ib >= a.n || ib < ia) return;
    const double* p = a.part + (size_t)bpl * GRAM_BLK + (size_t)e;
    const size_t stride = (size_t)a.nbp * GRAM_BLK;
    double acc = p[0];
    for (int c = 1; c < a.nchunks; ++c) acc += p[(size_t)c * stride];
    if (a.sums) {  // K20: the entry of the scaled rows back to the rows' own scale (exact unless it overflows)
        const size_t ra = a.d_rows ? gram_row_at<2>(a, ia) : gram_row_at<0>(a, ia), rb = a.d_rows ? gram_row_at<2>(a, ib) : gram_row_at<0>(a, ib);
        acc = ldexp(acc, gram_row_exp(a.sums[ra]) + gram_row_exp(a.sums[rb]));
    }
    a.gram[(size_t)ia * (size_t)a.n + (size_t)ib] = acc;
    a.gram[(size_t)ib * (size_t)a.n + (size_t)ia] = acc;
}

}  // namespace

hipError_t check_row_gram(const GramArgs& a) {
    const int64_t ntiles = (a.p + SUMSQ_TILE - 1) / SUMSQ_TILE;
    if (a.p <= 0 || a.n < 1 || a.n > PAIRDIST_MAX_ROWS || a.row0 < 0 || (a.d_rows && a.row0) || a.map.off != 0 || !valid_map(a.map, a.p) ||
        a.bp0 < 0 || a.nbp < 1 || a.bp0 + a.nbp > gram_block_pairs(a.n) || a.chunk_tiles != gram_chunk_tiles(ntiles, a.n) ||
        (int64_t)a.nchunks != (ntiles + a.chunk_tiles - 1) / a.chunk_tiles)
        return hipErrorInvalidValue;
    if (!a.slab || !a.part || !a.gram || (reinterpret_cast<uintptr_t>(a.slab) & 15)) return hipErrorInvalidValue;
    const int64_t grid = (int64_t)a.nchunks * a.nbp;
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launch_row_gram_fold(const GramArgs& a, hipStream_t s) {
    k_row_gram_fold<<<(unsigned)(a.nbp * (GRAM_BLK / BLOCK)), BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_row_gram(const GramArgs& a, hipStream_t s) {
    if (check_row_gram(a) != hipSuccess || a.sums) return hipErrorInvalidValue;  // (K16 scales nothing)
    const int64_t grid = (int64_t)a.nchunks * a.nbp;
    if (a.d_rows) k_row_gram<2><<<(unsigned)grid, BLOCK, 0, s>>>(a);
    else k_row_gram<0><<<(unsigned)grid, BLOCK, 0, s>>>(a);
    return launch_row_gram_fold(a, s);
}

}  // namespace pgh
