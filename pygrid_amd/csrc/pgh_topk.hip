// gfx950 (CDNA4, MI355X) kernel K18 of the cycle-close aggregation path.
//
// K18 k_topk_hist / k_topk_pick / k_topk_apply  top-k sparsification of the averaged update behind a FINAL fold
//       (SparseFed; build-owned: pgh_set_topk, the definition is in include/pgh_api.h, the design in DESIGN.md
//       section 5)
//
// A translation unit of its own, beside pgh_kernels.hip.  The k-th largest of P magnitude keys is found by a
// three-digit MSB-first radix select -- 11, 10 and 10 bits of the 31-bit key -- whose every count is an integer,
// so neither the launch shape nor the order in which workgroups merge their histograms can change a bit of it.
//   hist<D>  a workgroup sweeps 1,024 params at a time, one 16-byte column per lane, grid-stride past 8,192
//            workgroups.  Each key under the prefix chosen so far goes into the workgroup's LDS histogram with one
//            LDS add (no return value), the ragged last column element by element; lanes past p count nothing.  At
//            the end the non-zero bins go to the global histogram with one vector atomic add each -- at most 2,048
//            per workgroup, against 4 x 1,024 keys per sweep.  hist<0> also forms u = g + e from the delta plane
//            (g = -d, exact) and the committed error memory and stores it; the later passes read u alone.
//   pick<D>  one workgroup: lane t owns the BINS / 256 consecutive bins t * PER .., a 256-wide suffix scan of the
//            lanes' totals in LDS gives each lane the count above its bins, and the one lane whose bins straddle
//            the rank writes {prefix, remaining rank, #greater, #equal} to the state block.  Every lane clears its
//            own bins for the next digit.
//   apply    tau from the state block; keep = key >= tau; out = ckpt - s (or d = -s ahead of K10), e' = u - s.
// No kernel keeps anything in scratch; the largest, hist<0>, holds 8 KiB of LDS.
#include "pgh_topk.h"

#include <algorithm>

namespace pgh {
namespace {

constexpr int BLOCK = 256;
static_assert(TOPK_WG_PARAMS == 4 * BLOCK, "one 16-byte column per lane");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// [p]-sized planes may end mid-column: the last column goes scalar.
__device__ __forceinline__ u32x4 ldu4_tail(const float* base, int64_t i, int64_t p) {
    const uint32_t* b = reinterpret_cast<const uint32_t*>(base);
    if (i + 4 <= p) return *reinterpret_cast<const u32x4*>(b + i);
    u32x4 v = {0u, 0u, 0u, 0u};
    for (int e = 0; e < 4; ++e)
        if (i + e < p) v[e] = b[i + e];
    return v;
}

__device__ __forceinline__ void stu4_tail(float* base, int64_t i, int64_t p, u32x4 v) {
    uint32_t* b = reinterpret_cast<uint32_t*>(base);
    if (i + 4 <= p) { *reinterpret_cast<u32x4*>(b + i) = v; return; }
    for (int e = 0; e < 4; ++e)
        if (i + e < p) b[i + e] = v[e];
}

template <int DIGIT>
__global__ __launch_bounds__(BLOCK) void k_topk_hist(TopkArgs a) {
    constexpr int BINS = DIGIT == 0 ? TOPK_BINS : 1024;
    __shared__ uint32_t s_h[BINS];
    for (int b = threadIdx.x; b < BINS; b += BLOCK) s_h[b] = 0u;
    __syncthreads();
    const uint32_t prefix = DIGIT == 0 ? 0u : a.blk->prefix;  // (uniform: the pick before this launch wrote it)
    const int64_t ncol = (a.p + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < ncol; q += (int64_t)gridDim.x * BLOCK) {
        const int64_t i = 4 * q;
        u32x4 w;
        if constexpr (DIGIT == 0) {
            const u32x4 d = ldu4_tail(a.d, i, a.p);
            w = d ^ 0x80000000u;  // g = -d, exact
            if (a.e) {
                const u32x4 e = ldu4_tail(a.e, i, a.p);
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = __float_as_uint(__uint_as_float(w[j]) + __uint_as_float(e[j]));
            }
            stu4_tail(a.u, i, a.p, w);
        } else {
            w = ldu4_tail(a.u, i, a.p);
        }
        const int live = (int)std::min<int64_t>(4, a.p - i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t key = w[j] & 0x7fffffffu;
            bool mine = j < live;
            uint32_t bin;
            if constexpr (DIGIT == 0) {
                bin = key >> 20;
            } else if constexpr (DIGIT == 1) {
                mine = mine && (key >> 20) == prefix;
                bin = (key >> 10) & 1023u;
            } else {
                mine = mine && (key >> 10) == prefix;
                bin = key & 1023u;
            }
            if (mine) atomicAdd(&s_h[bin], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < BINS; b += BLOCK) {
        const uint32_t n = s_h[b];
        if (n) atomicAdd(&a.blk->hist[b], n);
    }
}

template <int DIGIT>
__global__ __launch_bounds__(BLOCK) void k_topk_pick(TopkBlock* blk, uint32_t k) {
    constexpr int BINS = DIGIT == 0 ? TOPK_BINS : 1024;
    constexpr int PER = BINS / BLOCK;
    constexpr int BITS = DIGIT == 0 ? 11 : 10;
    __shared__ uint64_t s_sum[BLOCK];
    const int t = threadIdx.x;
    uint32_t h[PER];
    uint64_t own = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        h[j] = blk->hist[t * PER + j];
        own += h[j];
    }
    const uint64_t rank = DIGIT == 0 ? (uint64_t)k : (uint64_t)blk->rank;
    const uint32_t prefix = DIGIT == 0 ? 0u : blk->prefix;
    const uint64_t n_gt = DIGIT == 0 ? 0ull : blk->n_gt;
    // inclusive suffix scan over the lanes' totals: v = the count in this lane's bins and every bin above them
    uint64_t v = own;
    s_sum[t] = v;
    __syncthreads();  // (also: every lane has read the state before the one below writes it)
    for (int off = 1; off < BLOCK; off <<= 1) {
        const uint64_t add = t + off < BLOCK ? s_sum[t + off] : 0ull;
        __syncthreads();
        v += add;
        s_sum[t] = v;
        __syncthreads();
    }
    uint64_t above = v - own;
#pragma unroll
    for (int j = PER - 1; j >= 0; --j) {
        if (above < rank && above + h[j] >= rank) {  // exactly one bin of one lane, for 1 <= rank <= the total
            blk->prefix = (prefix << BITS) | (uint32_t)(t * PER + j);
            blk->rank = (uint32_t)(rank - above);
            blk->n_eq = h[j];
            blk->n_gt = n_gt + above;
        }
        above += h[j];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) blk->hist[t * PER + j] = 0u;
}

__global__ __launch_bounds__(BLOCK) void k_topk_apply(TopkArgs a) {
    const uint32_t tau = a.blk->prefix;
    const int64_t ncol = (a.p + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < ncol; q += (int64_t)gridDim.x * BLOCK) {
        const int64_t i = 4 * q;
        const u32x4 u = ldu4_tail(a.u, i, a.p);
        u32x4 ck = {0u, 0u, 0u, 0u};
        if (a.ckpt) ck = ldu4_tail(a.ckpt, i, a.p);
        u32x4 o, e2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool keep = (u[j] & 0x7fffffffu) >= tau;
            const uint32_t s = keep ? u[j] : 0u;
            e2[j] = keep ? 0u : u[j];
            o[j] = a.ckpt ? __float_as_uint(__uint_as_float(ck[j]) - __uint_as_float(s)) : s ^ 0x80000000u;
        }
        stu4_tail(a.out, i, a.p, o);
        if (a.e2) stu4_tail(a.e2, i, a.p, e2);
    }
}

__global__ __launch_bounds__(BLOCK) void k_topk_clear(uint32_t* w, int n) {
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) w[i] = 0u;
}

bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

unsigned sweep_grid(int64_t p) {
    const int64_t ncol = (p + 3) >> 2;
    return (unsigned)std::min<int64_t>((ncol + BLOCK - 1) / BLOCK, TOPK_MAX_WGS);
}

}  // namespace

hipError_t launch_topk_hist(const TopkArgs& a, int digit, hipStream_t s) {
    if (a.p <= 0 || a.p > 0xffffffffll || !a.u || !a.blk || digit < 0 || digit > 2 || (digit == 0 && !a.d))
        return hipErrorInvalidValue;
    if (!aligned16({a.d, a.e, a.u, a.blk})) return hipErrorInvalidValue;
    const unsigned g = sweep_grid(a.p);
    switch (digit) {
    case 0: k_topk_hist<0><<<g, BLOCK, 0, s>>>(a); break;
    case 1: k_topk_hist<1><<<g, BLOCK, 0, s>>>(a); break;
    default: k_topk_hist<2><<<g, BLOCK, 0, s>>>(a); break;
    }
    return hipGetLastError();
}

hipError_t launch_topk_pick(const TopkArgs& a, int digit, hipStream_t s) {
    if (!a.blk || digit < 0 || digit > 2 || (digit == 0 && (a.k < 1 || (int64_t)a.k > a.p))) return hipErrorInvalidValue;
    switch (digit) {
    case 0: k_topk_pick<0><<<1, BLOCK, 0, s>>>(a.blk, a.k); break;
    case 1: k_topk_pick<1><<<1, BLOCK, 0, s>>>(a.blk, 0u); break;
    default: k_topk_pick<2><<<1, BLOCK, 0, s>>>(a.blk, 0u); break;
    }
    return hipGetLastError();
}

hipError_t launch_topk_apply(const TopkArgs& a, hipStream_t s) {
    if (a.p <= 0 || !a.u || !a.out || !a.blk) return hipErrorInvalidValue;
    if (!aligned16({a.u, a.ckpt, a.out, a.e2, a.blk})) return hipErrorInvalidValue;
    k_topk_apply<<<sweep_grid(a.p), BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_topk_clear(TopkBlock* blk, hipStream_t s) {
    if (!blk) return hipErrorInvalidValue;
    static_assert(sizeof(TopkBlock) % 4 == 0, "cleared word by word");
    k_topk_clear<<<(sizeof(TopkBlock) / 4 + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(reinterpret_cast<uint32_t*>(blk),
                                                                              (int)(sizeof(TopkBlock) / 4));
    return hipGetLastError();
}

}  // namespace pgh
