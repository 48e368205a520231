// gfx950 (CDNA4, MI355X) kernel K19 of the cycle-close aggregation path.
//
// K19 k_mix_rows  the row mix Y = W X of the listed slab rows in f64 on the matrix cores: nearest-neighbour
//       mixing ahead of a robust rule, and any other linear pre-aggregation (the definition is in
//       include/pgh_api.h, the design in DESIGN.md section 5).
//
// A translation unit of its own, beside pgh_gram.hip.  W is f64 and X f32: a product is rounded once, by the
// MFMA, as is every addition; the order of both is fixed below.
//
// Work split.  The m x p output is cut into blocks of MIX_RB = 128 destination list positions by MIX_CB = 128
// params.  A workgroup of 256 lanes owns one block and walks all n source rows: no split over k, no partial sums.
// The row block runs fastest in the grid, so the ceil(m / 128) workgroups that read one column block of X are
// neighbours in dispatch order and the re-reads of X come from L2 / Infinity Cache.
// Data path.  Per step of MIX_KSTEP = 16 source rows the workgroup brings to LDS
//   - the step's rows of X for its 128 params, as f32: lane l loads the 16-byte column l & 31 of rows
//     (l >> 5) + 8 q, q = 0, 1, so 32 lanes read one row's 512 contiguous bytes (through SlabMap::at: a column
//     block is 128-aligned and never straddles a slab block).  Rows at or past n and params at or past p are
//     masked to +0.0 before they reach LDS (the addresses clamp to the last row and the row's last column);
//   - the 128 x 16 slice of W, as f64: lane l loads column l & 15 of rows (l >> 4) + 16 q, q = 0 .. 7, so 16
//     lanes read 128 contiguous bytes of a W row.  Places at or past m or n are +0.0 and not loaded.
// Two LDS buffers: the next step's global loads are issued before this step's MFMAs and stored behind them, one
// barrier per step.  The LDS row strides are off the bank period: X 144 floats (the four rows a wave reads at
// once start 16 banks apart), W 18 doubles (a half-wave's 16 rows x 2 columns cover the 64 banks once).  The
// source row table is copied to LDS once, so a step's row addresses cost no dependent global load.
// Wave w owns the 64 x 64 sub-block (w >> 1, w & 1) as 4 x 4 MFMA tiles of 16 x 16: 64 f64 accumulators per
// lane.  For the k group j of a step (source rows 4 j .. 4 j + 3) lane (r = l & 15, kk = l >> 4) of a wave reads
// W[row tile's row r][4 j + kk] and, widened once, X[4 j + kk][column tile's column r] for each of its four row
// and four column tiles and issues v_mfma_f64_16x16x4_f64: one MFMA adds four consecutive k to the accumulator,
// the groups follow in increasing k.  Tiles wholly past m or past p are neither computed nor stored.
// Result layout of the MFMA: register v of lane l holds entry (4 v + (l >> 4), l & 15) of the tile, so the 16
// lanes of one row write 64 contiguous bytes of a destination row: stored directly, rounded once to f32.
#include "pgh_mix.h"

namespace pgh {
namespace {

constexpr int BLOCK = 256;
constexpr int MIX_XLD = MIX_CB + 16;    // LDS row stride of X in floats: 576 bytes, a multiple of 16
constexpr int MIX_WLD = MIX_KSTEP + 2;  // LDS row stride of W in doubles: 144 bytes

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

static_assert(MIX_RB == 128 && MIX_CB == 128 && MIX_KSTEP == 16 && BLOCK == 256, "K19: 4 waves of 64 x 64; 32 lanes an X row, 16 a W row");

// (two workgroups a CU, as K16 runs: one's barrier and loads hide behind the other's MFMAs)
__global__ __launch_bounds__(BLOCK, 2) void k_mix_rows(MixArgs a) {
    __shared__ __attribute__((aligned(16))) float sX[2][MIX_KSTEP][MIX_XLD];
    __shared__ __attribute__((aligned(16))) double sW[2][MIX_RB][MIX_WLD];
    __shared__ int32_t sSrc[PAIRDIST_MAX_ROWS];
    const int lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(lane >> 6);
    const int nrb = (a.m + MIX_RB - 1) / MIX_RB;
    const int rb = (int)(blockIdx.x % (unsigned)nrb);
    const int64_t q0 = (int64_t)(blockIdx.x / (unsigned)nrb) * MIX_CB;
    const int i0 = rb * MIX_RB;
    const int mi = min(MIX_RB, a.m - i0);                    // >= 1
    const int pc = (int)min((int64_t)MIX_CB, a.p - q0);      // >= 1
    const int ns = (a.n + MIX_KSTEP - 1) / MIX_KSTEP;        // >= 1

    for (int k = lane; k < a.n; k += BLOCK) sSrc[k] = a.d_src[k];
    __syncthreads();

    // ---- the global loads ----
    const int xr = lane >> 5, xc = (lane & 31) * 4;
    const int64_t last4 = (a.p - 1) & ~int64_t(3);
    const int64_t xoff = a.map.at(min(q0 + xc, last4));
    const int wk = lane & 15, wr0 = lane >> 4;
    f32x4 gx[2];
    double gw[8];
    auto fetch = [&](int s) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = s * MIX_KSTEP + xr + 8 * q;
            const float* row = a.slab + (size_t)(uint32_t)sSrc[min(k, a.n - 1)] * (size_t)a.map.ld;
            gx[q] = *reinterpret_cast<const f32x4*>(row + xoff);
            if (k >= a.n) gx[q] = f32x4{0.f, 0.f, 0.f, 0.f};  // past the list: masked, whatever the last row holds
        }
        if (xc + 4 > pc) {  // the shard's last column or past it: masked to +0.0, whatever the padding holds
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (xc + e >= pc) gx[q][e] = 0.f;
        }
        const int k = s * MIX_KSTEP + wk;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = wr0 + 16 * q;
            gw[q] = (i < mi && k < a.n) ? a.w[(size_t)(i0 + i) * (size_t)a.n + (size_t)k] : 0.0;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 2; ++q) *reinterpret_cast<f32x4*>(&sX[buf][xr + 8 * q][xc]) = gx[q];
#pragma unroll
        for (int q = 0; q < 8; ++q) sW[buf][wr0 + 16 * q][wk] = gw[q];
    };

    // ---- the wave's 4 x 4 MFMA tiles: the first nti row tiles and ntj column tiles hold something to store ----
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 15, kk = (lane & 63) >> 4;
    const int nti = __builtin_amdgcn_readfirstlane(max(0, min(4, (mi - wr * 64 + 15) / 16)));
    const int ntj = __builtin_amdgcn_readfirstlane(max(0, min(4, (pc - wc * 64 + 15) / 16)));
    const bool live = nti > 0 && ntj > 0;
    f64x4 acc[4][4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f64x4{0.0, 0.0, 0.0, 0.0};

    auto compute = [&](int buf) {
        const double* pw = &sW[buf][wr * 64 + li][kk];
        const float* px = &sX[buf][kk][wc * 64 + li];
#pragma unroll
        for (int j = 0; j < MIX_KSTEP / 4; ++j) {
            double ad[4], bd[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                ad[t] = pw[t * 16 * MIX_WLD + 4 * j];
                bd[t] = (double)px[4 * j * MIX_XLD + t * 16];
            }
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int tj = 0; tj < 4; ++tj)
                    if (ti < nti && tj < ntj)  // (uniform)
                        acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[ti], bd[tj], acc[ti][tj], 0, 0, 0);
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
        if (live) compute(s & 1);
        if (more) stash((s + 1) & 1);
        __syncthreads();
    }

    // ---- the store: register v of lane (li, kk) is entry (4 v + kk, li) of its tile ----
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
            if (!(ti < nti && tj < ntj)) continue;
            const int c = wc * 64 + tj * 16 + li;
            if (c >= pc) continue;
            const int64_t off = a.map.at(q0 + c);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = wr * 64 + ti * 16 + 4 * v + kk;
                if (i < mi) a.slab[(size_t)(uint32_t)a.d_dst[i0 + i] * (size_t)a.map.ld + off] = __double2float_rn(acc[ti][tj][v]);
            }
        }
}

}  // namespace

hipError_t launch_mix_rows(const MixArgs& a, hipStream_t s) {
    if (a.p <= 0 || a.n < 1 || a.n > PAIRDIST_MAX_ROWS || a.m < 1 || a.m > PAIRDIST_MAX_ROWS || a.map.off != 0 || !valid_map(a.map, a.p))
        return hipErrorInvalidValue;
    if (!a.slab || !a.d_src || !a.d_dst || !a.w || (reinterpret_cast<uintptr_t>(a.slab) & 15)) return hipErrorInvalidValue;
    const int64_t grid = ((a.p + MIX_CB - 1) / MIX_CB) * (int64_t)((a.m + MIX_RB - 1) / MIX_RB);
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    k_mix_rows<<<(unsigned)grid, BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace pgh
