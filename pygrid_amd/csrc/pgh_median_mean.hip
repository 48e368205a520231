// gfx950 (CDNA4, MI355X) kernel K15 of the cycle-close aggregation path.
//
// K15 k_median_mean  per param, the mean of the keep = N - drop values nearest the median (Bulyan's second
//       stage, MeaMed; build-owned: PGH_MEAN_AROUND_MEDIAN, the definition is in include/pgh_api.h, the
//       design in DESIGN.md section 5)
//
// A translation unit of its own, beside pgh_kernels.hip: it is compiled without the packed fp32 instructions
// (build.py), which the subtraction x - m per key and bit would otherwise be paired into; every step of the
// definition is one rounded scalar operation (__fsub_rn, __dadd_rn, __ddiv_rn; -ffp-contract=off, f32 denormals
// kept).
//
// K9's tile -- 64 consecutive columns, lane l of every wave owning column l, the rows on chip in registers, all
// loads of a lane issued before the first use, the same three row sources and the same tiers by N -- with
// another row mapping: wave w holds the fold positions 64 w .. 64 w + 63 in register order, so a wave is a
// block of the definition's sum and a wave-wide load is still 256 contiguous bytes of one row.
//   A  the median m by K9's bisection on u = key ^ 0x80000000: 32 steps, the W counts of a column meeting in
//      one of three 64-word LDS buffers used in turn (one barrier per step), then the upper middle of an even N.
//   B  the registers go back from u to the rows' bits, and the distance key e = bits(x - m) & 0x7fffffff is
//      derived from them wherever it is needed in the 16-wave tier (v_sub, v_lshl_or: 128 VGPRs per lane, room
//      for one array of 64 words, not two) and kept in a second array in the smaller ones.  E, the keep-th smallest e, by a 31-step bisection with the same
//      count exchange; places past N carry bit 31 in e, which no threshold reaches.  Then c_lt = #{e < E}
//      and the ties #{e == E} of every wave go to LDS; a wave takes the ties of the waves before it off the
//      quota keep - c_lt and walks its registers in order, keeping ties while quota is left.
//   C  every lane left-folds (double)x over its kept registers in order from +0.0; the W block sums meet in
//      LDS (W x 64 doubles), wave 0 folds them left to right, divides, rounds and stores ckpt - mean.
// Per float: 32 x 2 ops (A) + 31 x 4 (B) + about 20; per lane and step two LDS operations on top.  W = 1 (up to
// 64 rows): a lane holds its whole column, no LDS and no barrier, four independent tiles per 256-thread workgroup.
#include "pgh_median_mean.h"

namespace pgh {
namespace {

constexpr int BLOCK = 256;

template <int SRC>
__device__ __forceinline__ size_t mam_row_at(const Rows rows, int r) {
    if constexpr (SRC == 1) return (size_t)(uint32_t)rows.tab->rows[r];
    else if constexpr (SRC == 2) return (size_t)(uint32_t)rows.d_rows[r];
    else return (size_t)r;
}

// u = key(bits) ^ 0x80000000 (unsigned order = the key's signed order) and back
__device__ __forceinline__ uint32_t mam_ukey(uint32_t b) { return b ^ (uint32_t)(((int)b >> 31) | (int)0x80000000); }
__device__ __forceinline__ uint32_t mam_bits(uint32_t u) { return u ^ (uint32_t)(~((int)u >> 31) | (int)0x80000000); }
// The distance key of a row's bits, kept as e2 = e << 1 (the shift drops the sign as the definition's mask does
// and keeps the order; one v_lshl_or with the padding): pad = 0xffffffff for a place past N, which then lies past
// every threshold -- thresholds are even.
__device__ __forceinline__ uint32_t mam_dist(uint32_t bits, float m, uint32_t pad) {
    return (__float_as_uint(__fsub_rn(__uint_as_float(bits), m)) << 1) | pad;
}

template <int W, int KPL, int SRC>
__device__ __forceinline__ void median_mean_tile(const MedianMeanArgs& a, const Rows rows) {
    __shared__ uint32_t s_cnt[3][64];
    __shared__ uint32_t s_min[64];
    __shared__ uint32_t s_tie[W][64];
    __shared__ double s_sum[W][64];
    const int lane = threadIdx.x & 63;
    const int w = W == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t q = W == 1 ? (int64_t)blockIdx.x * blockDim.x + threadIdx.x : (int64_t)blockIdx.x * 64 + lane;
    const bool live = q < a.p;
    const int n = a.n_rows;
    const int nv = min(max(n - 64 * w, 0), KPL);  // this wave's block: fold positions 64 w .. 64 w + nv - 1
    const int64_t ld = a.map.ld;
    const uint32_t* col = reinterpret_cast<const uint32_t*>(a.diffs) + a.map.at(live ? q : 0);
    uint32_t k[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        k[j] = 0x7fffffffu;  // bits of the largest key
        if (j < nv && live) k[j] = __builtin_nontemporal_load(col + mam_row_at<SRC>(rows, 64 * w + j) * ld);
    }
    if constexpr (W > 1) {
        if (w == 0) {
            s_cnt[0][lane] = s_cnt[1][lane] = s_cnt[2][lane] = 0;
            s_min[lane] = 0xffffffffu;
        }
        __syncthreads();
    }
    int buf = 0;  // s_cnt[buf]: all zero here; s_cnt[buf + 2 (mod 3)] was read a barrier ago
    // the W counts of a column, summed: every lane of the column gets the same total (one barrier)
    auto meet = [&](uint32_t c) -> uint32_t {
        if constexpr (W > 1) {
            __hip_atomic_fetch_add(&s_cnt[buf][lane], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            c = s_cnt[buf][lane];
            const int old = buf == 0 ? 2 : buf - 1;
            if (w == 0) s_cnt[old][lane] = 0;  // every wave read it before this step's barrier
            buf = buf == 2 ? 0 : buf + 1;
        }
        return c;
    };

    // ---- A: the median (K9's bisection) ----
#pragma unroll
    for (int j = 0; j < KPL; ++j) k[j] = mam_ukey(k[j]);
    const uint32_t rank = (uint32_t)(n - 1) >> 1;
    uint32_t pre = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t T = pre | (1u << bit);
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < KPL; ++j) c += k[j] < T ? 1u : 0u;
        if (meet(c) <= rank) pre = T;
    }
    const bool even = !(n & 1);
    uint32_t upper = pre;
    if (even) {  // (uniform)
        uint32_t c = 0, mn = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            c += k[j] <= pre ? 1u : 0u;
            mn = k[j] > pre ? min(mn, k[j]) : mn;
        }
        if constexpr (W > 1) __hip_atomic_fetch_min(&s_min[lane], mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        c = meet(c);
        if constexpr (W > 1) mn = s_min[lane];
        upper = c >= (uint32_t)(n / 2 + 1) ? pre : mn;
    }
    const float lo = __uint_as_float(mam_bits(pre)), hi = __uint_as_float(mam_bits(upper));
    const float m = even ? __fadd_rn(__fmul_rn(0.5f, lo), __fmul_rn(0.5f, hi)) : lo;

    // ---- B: the distance threshold E, the keep-th smallest e ----
#pragma unroll
    for (int j = 0; j < KPL; ++j) k[j] = mam_bits(k[j]);
    // The 16-wave tier has 128 VGPRs per lane: room for the rows, not for their distances beside them, so it
    // derives e2 from the row wherever it reads it (mv: m behind an empty asm before each use, so that the
    // subtractions stay where they are written).  The smaller tiers keep e2 in a second array.
    constexpr bool DERIVE = W * KPL > 512;
    uint32_t e[DERIVE ? 1 : KPL];
    float mv = m;
    if constexpr (!DERIVE) {
#pragma unroll
        for (int j = 0; j < KPL; ++j) e[j] = mam_dist(k[j], m, j < nv ? 0u : 0xffffffffu);
    }
    auto dist = [&](int j) -> uint32_t {
        if constexpr (DERIVE) return mam_dist(k[j], mv, j < nv ? 0u : 0xffffffffu);
        else return e[j];
    };
    const uint32_t keep = (uint32_t)a.keep;
    uint32_t E = 0;  // (E2 = E << 1: bits 31 .. 1)
#pragma unroll 1
    for (int bit = 31; bit >= 1; --bit) {
        if constexpr (DERIVE) asm volatile("" : "+v"(mv));
        const uint32_t T = E | (1u << bit);
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < KPL; ++j) c += dist(j) < T ? 1u : 0u;
        if (meet(c) < keep) E = T;
    }
    if constexpr (DERIVE) asm volatile("" : "+v"(mv));
    uint32_t c_lt = 0, ties = 0;
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const uint32_t d = dist(j);
        c_lt += d < E ? 1u : 0u;
        ties += d == E ? 1u : 0u;
    }
    uint32_t before = 0;  // the ties at E in the blocks before this one: they come first in (e, k)
    if constexpr (W > 1) s_tie[w][lane] = ties;
    c_lt = meet(c_lt);
    if constexpr (W > 1) {
#pragma unroll
        for (int v = 0; v < W - 1; ++v) before += v < w ? s_tie[v][lane] : 0u;
    }
    const uint32_t quota = keep - c_lt;  // ties to keep in the whole column, >= 1
    uint32_t left = quota > before ? quota - before : 0u;

    // ---- C: the block's f64 sum over its kept places in order, the blocks' sums left to right ----
    if constexpr (DERIVE) asm volatile("" : "+v"(mv));
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const uint32_t d = dist(j);
        const bool tie = d == E && left > 0u;
        left -= tie ? 1u : 0u;
        if (d < E || tie) s = __dadd_rn(s, (double)__uint_as_float(k[j]));
    }
    if constexpr (W > 1) {
        s_sum[w][lane] = s;
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int g = 1; g < W; ++g) s = __dadd_rn(s, s_sum[g][lane]);
        }
    }
    if (w == 0 && live) a.out[q] = __fsub_rn(a.ckpt[q], __double2float_rn(__ddiv_rn(s, (double)keep)));
}

template <int W, int KPL, int SRC>
__global__ __launch_bounds__(W == 1 ? BLOCK : 64 * W) void k_median_mean(MedianMeanArgs a) {
    median_mean_tile<W, KPL, SRC>(a, Rows{nullptr, a.d_rows});
}
template <int W, int KPL>
__global__ __launch_bounds__(W == 1 ? BLOCK : 64 * W) void k_median_mean_tab(MedianMeanArgs a, RowTab tab) {
    median_mean_tile<W, KPL, 1>(a, Rows{&tab});
}

template <int W, int KPL>
hipError_t go_median_mean(const MedianMeanArgs& k, const RowTab* t, hipStream_t s) {
    constexpr int TB = W == 1 ? BLOCK : 64 * W;
    const int64_t tiles = (k.p + (W == 1 ? BLOCK : 64) - 1) / (W == 1 ? BLOCK : 64);
    const unsigned grid = (unsigned)tiles;
    if (t) k_median_mean_tab<W, KPL><<<grid, TB, 0, s>>>(k, *t);
    else if (k.d_rows) k_median_mean<W, KPL, 2><<<grid, TB, 0, s>>>(k);
    else k_median_mean<W, KPL, 0><<<grid, TB, 0, s>>>(k);
    return hipGetLastError();
}

}  // namespace

// K15's tiers are K9's (waves per tile x keys per lane).
hipError_t launch_median_mean(const MedianMeanArgs& a, const Rows& rows, hipStream_t s) {
    if ((rows.tab && rows.d_rows) || (rows.tab && a.n_rows > ROWTAB_MAX) || rows.row0 != 0) return hipErrorInvalidValue;
    if (a.p <= 0 || a.n_rows < 1 || a.n_rows > MEDIAN_NCHIP || a.keep < 1 || a.keep > a.n_rows) return hipErrorInvalidValue;
    if (!valid_map(a.map, a.p) || !a.diffs || (reinterpret_cast<uintptr_t>(a.diffs) & 15) || !a.ckpt || !a.out) return hipErrorInvalidValue;
    MedianMeanArgs k = a;
    k.d_rows = rows.d_rows;
    const RowTab* t = rows.tab;
    if (a.n_rows <= 8) return go_median_mean<1, 8>(k, t, s);
    if (a.n_rows <= 16) return go_median_mean<1, 16>(k, t, s);
    if (a.n_rows <= 32) return go_median_mean<1, 32>(k, t, s);
    if (a.n_rows <= 64) return go_median_mean<1, 64>(k, t, s);
    if (a.n_rows <= 128) return go_median_mean<2, 64>(k, t, s);
    if (a.n_rows <= 256) return go_median_mean<4, 64>(k, t, s);
    if (a.n_rows <= 512) return go_median_mean<8, 64>(k, t, s);
    return go_median_mean<MEDIAN_WAVES, 64>(k, t, s);
}

}  // namespace pgh
