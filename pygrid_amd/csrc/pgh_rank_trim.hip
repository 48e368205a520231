// gfx950 (CDNA4, MI355X) kernel K17 of the cycle-close aggregation path.
//
// K17 k_rank_trim  per param, the mean of sort(values)[b : N - b] for any b with N >= 2 b + 1 (the coordinate-wise
//       trimmed mean by rank; build-owned: PGH_RANK_TRIMMED_MEAN, the definition is in include/pgh_api.h, the
//       design in DESIGN.md section 5)
//
// A translation unit of its own, beside pgh_kernels.hip and pgh_median_mean.hip.  Every f64 step of the
// definition is one rounded operation (__dadd_rn, __dmul_rn, __ddiv_rn; -ffp-contract=off).
//
// K9's tile -- 64 consecutive columns, lane l of every wave owning column l, the rows on chip in registers, all
// loads of a lane issued before the first use, the same three row sources and the same tiers by N -- with K15's
// row mapping: wave w holds the fold positions 64 w .. 64 w + 63 in register order, so a wave is a block of the
// definition's sum and a wave-wide load is still 256 contiguous bytes of one row.
//   A  both boundary keys in one bisection on u = key ^ 0x80000000: two prefixes, preL (rank b) and preH (rank
//      N - 1 - b), each with its own threshold per bit.  A lane counts its keys below either threshold and packs
//      the two counts into one word, cL | cH << 16 -- a column's totals are at most 1,024, so the halves never
//      carry into each other -- and the W words of a column meet in one of three 64-word LDS buffers used in
//      turn: one LDS add per lane and one barrier per step serve both selections.  Each half then takes its own
//      branch.  Places past N hold the largest u, which no threshold exceeds.
//   B  one more packed sweep: #{u <= L} over the live places only (a row may hold the padding's bit pattern,
//      0x7fffffff) and #{u < H}.  From them the multiplicities kL and kH of the boundary values in the kept
//      multiset: equal keys are identical bits, so which of several equal rows is kept never matters and no tie
//      walk is needed.
//   C  every lane left-folds (double)x over its registers strictly between L and H in order from +0.0; the W
//      block sums meet in LDS (W x 64 doubles), wave 0 folds them left to right, adds kL * unkey(L) and
//      kH * unkey(H) -- exact products --, divides, rounds and stores ckpt - mean.
// Per float: 32 x 4 ops (A) + about 15; per lane and step two LDS operations on top.  Only the one array of 64
// keys is live.  W = 1 (up to 64 rows): a lane holds its whole column, no LDS and no barrier, four independent
// tiles per 256-thread workgroup.
#include "pgh_rank_trim.h"

namespace pgh {
namespace {

constexpr int BLOCK = 256;

template <int SRC>
__device__ __forceinline__ size_t rt_row_at(const Rows rows, int r) {
    if constexpr (SRC == 1) return (size_t)(uint32_t)rows.tab->rows[r];
    else if constexpr (SRC == 2) return (size_t)(uint32_t)rows.d_rows[r];
    else return (size_t)r;
}

// u = key(bits) ^ 0x80000000 (unsigned order = the key's signed order) and back
__device__ __forceinline__ uint32_t rt_ukey(uint32_t b) { return b ^ (uint32_t)(((int)b >> 31) | (int)0x80000000); }
__device__ __forceinline__ uint32_t rt_bits(uint32_t u) { return u ^ (uint32_t)(~((int)u >> 31) | (int)0x80000000); }
__device__ __forceinline__ double rt_value(uint32_t u) { return (double)__uint_as_float(rt_bits(u)); }

template <int W, int KPL, int SRC>
__device__ __forceinline__ void rank_trim_tile(const RankTrimArgs& a, const Rows rows) {
    __shared__ uint32_t s_cnt[3][64];
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
        if (j < nv && live) k[j] = __builtin_nontemporal_load(col + rt_row_at<SRC>(rows, 64 * w + j) * ld);
    }
    if constexpr (W > 1) {
        if (w == 0) s_cnt[0][lane] = s_cnt[1][lane] = s_cnt[2][lane] = 0;
        __syncthreads();
    }
    int buf = 0;  // s_cnt[buf]: all zero here; s_cnt[buf + 2 (mod 3)] was read a barrier ago
    // the W packed counts of a column, summed: every lane of the column gets the same totals (one barrier)
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

    // ---- A: L = s[b] and H = s[n - 1 - b] in one bisection ----
#pragma unroll
    for (int j = 0; j < KPL; ++j) k[j] = rt_ukey(k[j]);
    const uint32_t b = (uint32_t)a.b;
    const uint32_t rankL = b, rankH = (uint32_t)(n - 1) - b;
    uint32_t preL = 0, preH = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t TL = preL | (1u << bit), TH = preH | (1u << bit);
        uint32_t cl = 0, ch = 0;
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            cl += k[j] < TL ? 1u : 0u;
            ch += k[j] < TH ? 1u : 0u;
        }
        const uint32_t c = meet(cl | (ch << 16));
        if ((c & 0xffffu) <= rankL) preL = TL;
        if ((c >> 16) <= rankH) preH = TH;
    }
    const uint32_t L = preL, H = preH;

    // ---- B: the boundary values' multiplicities in the kept multiset ----
    uint32_t cle = 0, clt = 0;
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        cle += (j < nv && k[j] <= L) ? 1u : 0u;  // live places only: a row may hold the padding's bits
        clt += k[j] < H ? 1u : 0u;               // (the padding lies below no H)
    }
    const uint32_t c = meet(cle | (clt << 16));
    const uint32_t keep = (uint32_t)n - 2u * b;
    const uint32_t kL = L < H ? (c & 0xffffu) - b : keep;
    const uint32_t kH = L < H ? ((uint32_t)n - b) - (c >> 16) : 0u;

    // ---- C: the block's f64 sum over its interior places in order, the blocks' sums left to right ----
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < KPL; ++j)
        if (k[j] > L && k[j] < H) s = __dadd_rn(s, rt_value(k[j]));
    if constexpr (W > 1) {
        s_sum[w][lane] = s;
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int g = 1; g < W; ++g) s = __dadd_rn(s, s_sum[g][lane]);
        }
    }
    if (w == 0 && live) {
        s = __dadd_rn(s, __dmul_rn((double)kL, rt_value(L)));
        if (kH > 0u) s = __dadd_rn(s, __dmul_rn((double)kH, rt_value(H)));
        a.out[q] = __fsub_rn(a.ckpt[q], __double2float_rn(__ddiv_rn(s, (double)keep)));
    }
}

template <int W, int KPL, int SRC>
__global__ __launch_bounds__(W == 1 ? BLOCK : 64 * W) void k_rank_trim(RankTrimArgs a) {
    rank_trim_tile<W, KPL, SRC>(a, Rows{nullptr, a.d_rows});
}
template <int W, int KPL>
__global__ __launch_bounds__(W == 1 ? BLOCK : 64 * W) void k_rank_trim_tab(RankTrimArgs a, RowTab tab) {
    rank_trim_tile<W, KPL, 1>(a, Rows{&tab});
}

template <int W, int KPL>
hipError_t go_rank_trim(const RankTrimArgs& k, const RowTab* t, hipStream_t s) {
    constexpr int TB = W == 1 ? BLOCK : 64 * W;
    const int64_t tiles = (k.p + (W == 1 ? BLOCK : 64) - 1) / (W == 1 ? BLOCK : 64);
    const unsigned grid = (unsigned)tiles;
    if (t) k_rank_trim_tab<W, KPL><<<grid, TB, 0, s>>>(k, *t);
    else if (k.d_rows) k_rank_trim<W, KPL, 2><<<grid, TB, 0, s>>>(k);
    else k_rank_trim<W, KPL, 0><<<grid, TB, 0, s>>>(k);
    return hipGetLastError();
}

}  // namespace

// K17's tiers are K9's (waves per tile x keys per lane).
hipError_t launch_rank_trim(const RankTrimArgs& a, const Rows& rows, hipStream_t s) {
    if ((rows.tab && rows.d_rows) || (rows.tab && a.n_rows > ROWTAB_MAX) || rows.row0 != 0) return hipErrorInvalidValue;
    if (a.p <= 0 || a.b < 1 || a.n_rows > MEDIAN_NCHIP || a.n_rows < 2 * (int64_t)a.b + 1) return hipErrorInvalidValue;
    if (!valid_map(a.map, a.p) || !a.diffs || (reinterpret_cast<uintptr_t>(a.diffs) & 15) || !a.ckpt || !a.out) return hipErrorInvalidValue;
    RankTrimArgs k = a;
    k.d_rows = rows.d_rows;
    const RowTab* t = rows.tab;
    if (a.n_rows <= 8) return go_rank_trim<1, 8>(k, t, s);
    if (a.n_rows <= 16) return go_rank_trim<1, 16>(k, t, s);
    if (a.n_rows <= 32) return go_rank_trim<1, 32>(k, t, s);
    if (a.n_rows <= 64) return go_rank_trim<1, 64>(k, t, s);
    if (a.n_rows <= 128) return go_rank_trim<2, 64>(k, t, s);
    if (a.n_rows <= 256) return go_rank_trim<4, 64>(k, t, s);
    if (a.n_rows <= 512) return go_rank_trim<8, 64>(k, t, s);
    return go_rank_trim<MEDIAN_WAVES, 64>(k, t, s);
}

}  // namespace pgh
