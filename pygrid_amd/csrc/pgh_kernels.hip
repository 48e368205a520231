// gfx950 (CDNA4, MI355X) kernels for the PyGrid cycle-close aggregation path.
//
// K1  k_fedavg<MODE_MEAN>      out = ckpt - (((d0 + d1) + d2) + ...) / N
//       restates cycle_manager.py:276-296 (reduce(th.add) -> th.div(., N) -> subtract)
//     k_fedavg<MODE_WEIGHTED>  out = ckpt - (sum_c w_c*d_c) / (sum_c w_c)   (build-owned)
// K2  k_fedavg<MODE_ITERATIVE> a = d0; a = (a*k + d_k)/(k+1); out = ckpt - a
//       restates cycle_manager.py:266-269 + 01-Create-plan.ipynb:450-454
// K3  k_secagg                 Z_2^64 wrap-sum over [clients*parties][P] int64 + fixed-point
//       decode float32(int64)/10^prec (PySyft 0.2.9 semantics)
// K8  k_fedavg_trim            per param, the mean without the b largest and b smallest values
//       (build-owned: PGH_TRIMMED_MEAN, a register-resident selection network)
// K9  k_median / k_median_pass per param, the median of the N values: a bisection on the key, the
//       rows of a 64-column tile on chip (K9) or one pass over the slab per bit (K9p)
//       (build-owned: PGH_MEDIAN)
// K7  k_row_sumsq              sumsq_c = sum_i (double)d_c[i]^2 along a client's row, in one fixed
//       order (build-owned: the norms of PGH_CLIPPED_MEAN)
// K10 k_server_opt             the server optimizer's step behind a FINAL fold: FedAvgM, FedAdagrad,
//       FedAdam, FedYogi on g = the cycle's average (build-owned: pgh_set_server_opt)
// K11 k_dp_noise              Gaussian noise on the clipped average behind a FINAL fold, ahead of K10:
//       Philox4x32-10, Marsaglia's polar method, a libm-free logarithm (build-owned: pgh_set_dp_noise,
//       DESIGN.md section 5); k_dp_normals returns the sampler's normals alone
// K12 k_row_distsq             K7's sum over d_c[i] - v[i]: every row's squared distance to a moving point,
//       a tile of the point held in registers over a chunk of rows; one tile body with K7, row_sq_tile
// K13 k_row_pairdist           K12's sum for every pair of the listed rows (Multi-Krum): a block of anchor rows'
//       tile held in registers while the later rows stream past; k_row_pairdist_fold finishes each pair
//       (build-owned: PGH_GEOMETRIC_MEDIAN)
// K14 k_row_dot                K7's sum over d_c[i] * g0[i]: every row's inner product with a fixed vector (the
//       trust root), K12's shape and tile body (build-owned: PGH_TRUSTED_MEAN)
//
// Design (DESIGN.md "Kernels"): every kernel is a single streaming pass over the slab held in
// HBM, column-blocked (SlabMap in pgh_kernels.h: blocks of ld columns, each block all rows,
// so a lane's walk down the client rows stays inside one compact block).  Parallelism is over
// the PARAMETER axis only: one lane owns a column (1 or 4 fp32, 1 or 2 int64) and walks the
// client rows in index order, so the fp32 fold order is exactly the reference's left fold
// (bit-exact, no tree/shuffle reordering).  U rows are issued before they are consumed to keep
// U loads per lane in flight.  No LDS: there is no reuse to stage, and no MFMA: this is a
// 0.25 flop/byte reduction, bound by HBM bandwidth.  (K9, the median, is the exception: it holds
// the rows of a tile on chip, a column's rows shared by the waves of a workgroup past 64 rows, whose
// per-bit counts meet in 1 KiB of LDS.)
//
// Build flags matter for parity: -ffp-contract=off (no a*k+d -> FMA), no fast-math, f32
// denormals kept, IEEE (correctly rounded) f32 division.
#include "pgh_kernels.h"

#include <algorithm>

namespace pgh {
namespace {

constexpr int BLOCK = 256;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t sm64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t row_key(uint64_t seed, uint64_t stream, uint64_t row) {
    return sm64(sm64(seed ^ (stream << 48)) ^ (row * 0xD1B54A32D192ED03ull));
}

__device__ __forceinline__ float bits_to_f32(uint64_t b, float scale) {
    const uint32_t s = (uint32_t)(b & 0xFFFF) + (uint32_t)((b >> 16) & 0xFFFF) +
                       (uint32_t)((b >> 32) & 0xFFFF) + (uint32_t)(b >> 48);
    return (float)((int32_t)s - 131070) * scale;  // exact convert, one rounded multiply
}

template <bool NT>
__device__ __forceinline__ f32x4 ld4(const float* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    else return *reinterpret_cast<const f32x4*>(p);
}

template <bool NT>
__device__ __forceinline__ u64x2 ld2u(const int64_t* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(p));
    else return *reinterpret_cast<const u64x2*>(p);
}

// [p]-sized vectors (acc, ckpt, out) may end mid-column: the last column goes scalar.
__device__ __forceinline__ f32x4 ld4_tail(const float* base, int64_t q, int64_t p) {
    const int64_t i = 4 * q;
    if (i + 4 <= p) return *reinterpret_cast<const f32x4*>(base + i);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < 4; ++e)
        if (i + e < p) v[e] = base[i + e];
    return v;
}

__device__ __forceinline__ void st4_tail(float* base, int64_t q, int64_t p, f32x4 v) {
    const int64_t i = 4 * q;
    if (i + 4 <= p) { *reinterpret_cast<f32x4*>(base + i) = v; return; }
    for (int e = 0; e < 4; ++e)
        if (i + e < p) base[i + e] = v[e];
}

// Lane element: VEC = 4 (one 16-byte column of 4 params, the default) or VEC = 1 (one param per
// lane: 4x the lanes, for shards too small to fill 256 CUs with 16-byte columns).
template <int VEC> struct Lane;
template <> struct Lane<4> {
    using T = f32x4;
    template <bool NT> static __device__ __forceinline__ T load(const float* p) { return ld4<NT>(p); }
    static __device__ __forceinline__ T load_tail(const float* b, int64_t q, int64_t p) { return ld4_tail(b, q, p); }
    static __device__ __forceinline__ void store_tail(float* b, int64_t q, int64_t p, T v) { st4_tail(b, q, p, v); }
};
template <> struct Lane<1> {
    using T = float;
    template <bool NT> static __device__ __forceinline__ T load(const float* p) {
        if constexpr (NT) return __builtin_nontemporal_load(p);
        else return *p;
    }
    static __device__ __forceinline__ T load_tail(const float* b, int64_t q, int64_t p) { return q < p ? b[q] : 0.f; }
    static __device__ __forceinline__ void store_tail(float* b, int64_t q, int64_t p, T v) { if (q < p) b[q] = v; }
};

template <int MODE, class T>
__device__ __forceinline__ T fold(T acc, T v, const float* w, int r) {
    if constexpr (MODE == MODE_MEAN) {
        return acc + v;                                   // th.add, cycle_manager.py:286
    } else {
        return acc + v * w[r];                            // MODE_WEIGHTED: product rounded, then add
    }
}

// Iterative plan step k (01-Create-plan.ipynb:453): t = avg * k + d (two roundings: no FMA under
// -ffp-contract=off), avg = t / (k + 1) with k and k + 1 promoted to f32 like th.tensor([k]).
// The IEEE division is replaced by (float)((double)t * rec), rec = RN_f64(1 / y), y = (float)(k+1):
// the double product is within ~2^-52 of t / y, which for a normal quotient is never an f32
// rounding midpoint and never within ~2^-49 of one, so the final rounding agrees bit for bit
// (tests/native/recip_div_check.c: 2e9 operand pairs against IEEE division).  A lane whose
// quotient could be below 2^-125 (0 < |t| < 2^-125 * y) sets `tiny`; the caller then redoes the
// batch with real divisions.  rec comes from a per-client table (scalar loads: k is uniform).
__device__ __forceinline__ float iter_step(float acc, float v, float kf, double rec, uint32_t thr, bool& tiny) {
    const float t = acc * kf + v;
    const uint32_t ut = __float_as_uint(t) & 0x7fffffffu;
    tiny |= (ut - 1u) < thr;  // thr = bits(2^-125 * y) - 1
    return (float)((double)t * rec);
}
__device__ __forceinline__ f32x4 iter_step(f32x4 acc, f32x4 v, float kf, double rec, uint32_t thr, bool& tiny) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = iter_step(acc[e], v[e], kf, rec, thr, tiny);
    return o;
}

// Slab row of the launch's row r (Rows in pgh_kernels.h; wave-uniform, so a table entry is a scalar
// load): SRC 0 contiguous from row0, 1 the RowTab (report-time folds of scattered slots: the kernarg
// segment), 2 the device table.  The device functions hand Rows on by value: behind a reference the
// deepest iterative row-table fold (U = 64) kept its RowTab in scratch.
template <int SRC>
__device__ __forceinline__ size_t row_at(const Rows rows, int r) {
    if constexpr (SRC == 1) return (size_t)(uint32_t)rows.tab->rows[r];
    else if constexpr (SRC == 2) return (size_t)(uint32_t)rows.d_rows[r];
    else return (size_t)(rows.row0 + r);
}

// Fold rows r .. r + nv - 1 (nv <= U, already loaded in v) into acc, in order.  nv is U for full
// batches (the guards fold away) and the wave-uniform remainder for the last one.
template <int MODE, int U, int W, class T>
__device__ __forceinline__ void fold_rows(T (&acc)[W], const T (&v)[U][W], const FedavgArgs& a, int r, int nv) {
    if constexpr (MODE != MODE_ITERATIVE) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u < nv)
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] = fold<MODE>(acc[w], v[u][w], a.weights, r + u);
    } else {
        T acc0[W];
#pragma unroll
        for (int w = 0; w < W; ++w) acc0[w] = acc[w];
        bool tiny = false;
        const uint32_t k0 = (uint32_t)(a.client0 + r);  // client indices < 2^31
#pragma unroll
        for (int u0 = 0; u0 < U; u0 += 8) {
            double rec[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (u0 + j < U && u0 + j < nv) rec[j] = a.recips[r + u0 + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (u0 + j >= U || u0 + j >= nv) break;
                const uint32_t k = k0 + (uint32_t)(u0 + j);
                const float kf = (float)k, y = (float)(k + 1u);
                const uint32_t thr = __float_as_uint(0x1p-125f * y) - 1u;
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] = iter_step(acc[w], v[u0 + j][w], kf, rec[j], thr, tiny);
            }
        }
        if (tiny) {  // rare: a quotient near f32's subnormal range -- redo these rows dividing for real
#pragma unroll
            for (int w = 0; w < W; ++w) acc[w] = acc0[w];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u >= nv) break;
                const uint32_t k = k0 + (uint32_t)u;
                const float kf = (float)k, y = (float)(k + 1u);
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] = (acc[w] * kf + v[u][w]) / y;
            }
        }
    }
}

// W columns per lane (q0, q0 + qstep, ...: each load instruction of a wave still reads one
// contiguous span), all rows of the chunk, in order.  VEC consecutive params per column.
template <int MODE, int U, int W, bool NT, int VEC, int SRC>
__device__ __forceinline__ void fedavg_columns(const FedavgArgs& a, const Rows rows, int64_t q0, int64_t qstep) {
    using L = Lane<VEC>;
    using T = typename L::T;
    const int n = a.n_rows;
    const int64_t ld = a.map.ld;
    const float* col[W];
#pragma unroll
    for (int w = 0; w < W; ++w) col[w] = a.diffs + a.map.at(VEC * (q0 + w * qstep));
    T acc[W];
    int r;
    if (a.flags & FL_FIRST) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            acc[w] = L::template load<NT>(col[w] + row_at<SRC>(rows, 0) * ld);  // fold starts at d0, not 0
            if constexpr (MODE == MODE_WEIGHTED) acc[w] = acc[w] * a.weights[0];
        }
        r = 1;
    } else {
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = L::load_tail(a.acc, q0 + w * qstep, a.p);
        r = 0;
    }
    for (; r + U <= n; r += U) {
        T v[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int w = 0; w < W; ++w)
                v[u][w] = L::template load<NT>(col[w] + row_at<SRC>(rows, r + u) * ld);
        fold_rows<MODE, U, W>(acc, v, a, r, U);
    }
    if (r < n) {  // the last partial batch, its loads in flight together
        const int nv = n - r;
        T v[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u < nv)
#pragma unroll
                for (int w = 0; w < W; ++w) v[u][w] = L::template load<NT>(col[w] + row_at<SRC>(rows, r + u) * ld);
        fold_rows<MODE, U, W>(acc, v, a, r, nv);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int64_t q = q0 + w * qstep;
        if (a.flags & FL_FINAL) {
            const T avg = (MODE == MODE_ITERATIVE) ? acc[w] : acc[w] / a.divisor;  // th.div, :288
            L::store_tail(a.out, q, a.p, L::load_tail(a.ckpt, q, a.p) - avg);     // :293-296
        } else {
            L::store_tail(a.acc, q, a.p, acc[w]);
        }
    }
}

// Software-pipelined column walk (variants 21/22): the loads of row batch i + 1 are issued before
// batch i is folded, so a lane keeps between U and 2U rows in flight instead of draining to zero
// between batches.  Two named buffers (no register copies that would wait on the new loads); the
// fold of one batch and the loads of the next sit in one basic block, so the wait counts only
// cover the batch being folded.  Same fold order as fedavg_columns: bit-identical.
template <int MODE, int U, bool NT, int VEC>
__device__ __forceinline__ void fedavg_columns_pipe(const FedavgArgs& a, int64_t q) {
    using L = Lane<VEC>;
    using T = typename L::T;
    const int n = a.n_rows;
    const int64_t ld = a.map.ld;
    const float* col = a.diffs + a.map.at(VEC * q);
    T acc[1];
    int r;
    if (a.flags & FL_FIRST) {
        acc[0] = L::template load<NT>(col);
        if constexpr (MODE == MODE_WEIGHTED) acc[0] = acc[0] * a.weights[0];
        r = 1;
    } else {
        acc[0] = L::load_tail(a.acc, q, a.p);
        r = 0;
    }
    T A[U][1], B[U][1];
    if (r + U <= n) {
#pragma unroll
        for (int u = 0; u < U; ++u) A[u][0] = L::template load<NT>(col + (size_t)(r + u) * ld);
        for (;;) {
            if (r + 2 * U <= n) {
#pragma unroll
                for (int u = 0; u < U; ++u) B[u][0] = L::template load<NT>(col + (size_t)(r + U + u) * ld);
                fold_rows<MODE, U, 1>(acc, A, a, r, U);
                r += U;
            } else {
                fold_rows<MODE, U, 1>(acc, A, a, r, U);
                r += U;
                break;
            }
            if (r + 2 * U <= n) {
#pragma unroll
                for (int u = 0; u < U; ++u) A[u][0] = L::template load<NT>(col + (size_t)(r + U + u) * ld);
                fold_rows<MODE, U, 1>(acc, B, a, r, U);
                r += U;
            } else {
                fold_rows<MODE, U, 1>(acc, B, a, r, U);
                r += U;
                break;
            }
        }
    }
    if (r < n) {  // the last partial batch, its loads in flight together
        const int nv = n - r;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u < nv) A[u][0] = L::template load<NT>(col + (size_t)(r + u) * ld);
        fold_rows<MODE, U, 1>(acc, A, a, r, nv);
    }
    if (a.flags & FL_FINAL) {
        const T avg = (MODE == MODE_ITERATIVE) ? acc[0] : acc[0] / a.divisor;  // th.div, :288
        L::store_tail(a.out, q, a.p, L::load_tail(a.ckpt, q, a.p) - avg);     // :293-296
    } else {
        L::store_tail(a.acc, q, a.p, acc[0]);
    }
}

template <int MODE, int U, bool NT, int TB, int VEC>
__global__ __launch_bounds__(TB) void k_fedavg_pipe(FedavgArgs a, int64_t ncol) {
    for (int64_t q = (int64_t)blockIdx.x * TB + threadIdx.x; q < ncol; q += (int64_t)gridDim.x * TB)
        fedavg_columns_pipe<MODE, U, NT, VEC>(a, q);
}

// Workgroup -> tile order.  Workgroups are dealt round robin over the 8 XCDs (wg % 8); XMAP gives
// each XCD a contiguous eighth of the tiles instead (A/B variant 23: does DRAM page locality
// across XCDs matter for a read-once stream?).
template <bool XMAP>
__device__ __forceinline__ int64_t tile_of_wg() {
    if constexpr (!XMAP) return blockIdx.x;
    const int64_t g = gridDim.x, per = g / 8, b = blockIdx.x;
    return b < per * 8 ? (b % 8) * per + b / 8 : b;
}

// Grid-stride over tiles of TB x W columns; a partial last tile goes one column per lane.
template <int MODE, int U, int W, bool NT, int TB, int VEC, int SRC, bool XMAP = false>
__device__ __forceinline__ void fedavg_tiles(const FedavgArgs& a, const Rows rows, int64_t ncol) {
    const int64_t tile = (int64_t)TB * W;
    for (int64_t t0 = tile_of_wg<XMAP>() * tile; t0 < ncol; t0 += (int64_t)gridDim.x * tile) {
        const int64_t q0 = t0 + threadIdx.x;
        if (t0 + tile <= ncol) {
            fedavg_columns<MODE, U, W, NT, VEC, SRC>(a, rows, q0, TB);
        } else {
            for (int64_t q = q0; q < ncol && q < t0 + tile; q += TB)
                fedavg_columns<MODE, U, 1, NT, VEC, SRC>(a, rows, q, TB);
        }
    }
}

template <int MODE, int U, int W, bool NT, int TB, int VEC, bool XMAP = false>
__global__ __launch_bounds__(TB) void k_fedavg(FedavgArgs a, int64_t ncol) {
    fedavg_tiles<MODE, U, W, NT, TB, VEC, 0, XMAP>(a, Rows{}, ncol);
}

// The same fold over the slab rows listed in `tab` (report-time aggregation, pgh_fold_slots).
template <int MODE, int U, int W, bool NT, int TB, int VEC>
__global__ __launch_bounds__(TB) void k_fedavg_rows(FedavgArgs a, int64_t ncol, RowTab tab) {
    fedavg_tiles<MODE, U, W, NT, TB, VEC, 1>(a, Rows{&tab}, ncol);
}

// K8: coordinate-wise trimmed mean (MODE_TRIMMED; the definition is in include/pgh_api.h).  The same
// walk as fedavg_columns -- one lane down the client rows of its column, U non-temporal loads in
// flight -- with a selection network in registers beside the stream: per param B keys `lo` (the B
// smallest so far), B keys `hi` (the B largest of what lo evicted) and the f32 sum of what hi
// evicted.  Keys are int32 (v_min_i32 / v_max_i32 / v_med3_i32), converted on load and back on
// eviction (op count: trim_step).  No LDS and no second pass.
__device__ __forceinline__ int trim_key(int b) { return b ^ ((b >> 31) & 0x7fffffff); }  // its own inverse

__device__ __forceinline__ float lane_get(float v, int) { return v; }
__device__ __forceinline__ float lane_get(const f32x4& v, int e) { return v[e]; }
__device__ __forceinline__ void lane_put(float& v, int, float x) { v = x; }
__device__ __forceinline__ void lane_put(f32x4& v, int e, float x) { v[e] = x; }

template <int B, int VEC>
struct TrimState {
    int lo[B][VEC], hi[B][VEC];
    float acc[VEC];
};

// The median of three as min / max (hipcc selects v_med3_i32 for this shape).
__device__ __forceinline__ int med3i(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }

// One row.  k = its fold index, the same in every lane.  The definition's compare-exchange chain
// (t = max(lo[j], e); lo[j] = min(lo[j], e); e = t) is an insertion into a list that stays sorted
// (lo ascending, hi descending; the sentinels and a state read back from HBM are sorted too), so
// entry j of the new list is the median of its two old neighbours and the new key, and the evicted
// key the max (min) of the old last entry and the new key: the same values bit for bit -- keys are
// totally ordered and equal keys are equal bits -- in B + 1 independent ops instead of a chain of 2B.
// Per float: 3 (key) + (B + 1) + (B + 1) + 3 (unkey) + 1 (add) = 2B + 9 VALU ops.
// STEADY: k > 2B is known, so the fill phase's branches (k < B: lo still filling; k < 2B: hi still
// filling; k == 2B: the sum starts at the first kept value, not at 0, so that -0 survives) are
// compiled out.
template <int B, int VEC, bool STEADY, class T>
__device__ __forceinline__ void trim_step(TrimState<B, VEC>& s, const T& v, int64_t k) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        int x = trim_key(__float_as_int(lane_get(v, e)));
        const int up = max(s.lo[B - 1][e], x);  // the largest of lo and x leaves lo
#pragma unroll
        for (int j = B - 1; j > 0; --j) s.lo[j][e] = med3i(s.lo[j - 1][e], s.lo[j][e], x);
        s.lo[0][e] = min(s.lo[0][e], x);
        if (!STEADY && k < B) continue;
        const int down = min(s.hi[B - 1][e], up);  // the smallest of hi and it leaves hi: a kept value
#pragma unroll
        for (int j = B - 1; j > 0; --j) s.hi[j][e] = med3i(s.hi[j - 1][e], s.hi[j][e], up);
        s.hi[0][e] = max(s.hi[0][e], up);
        if (!STEADY && k < 2 * B) continue;
        const float kept = __int_as_float(trim_key(down));
        s.acc[e] = (!STEADY && k == 2 * B) ? kept : s.acc[e] + kept;
    }
}

// A state plane is indexed like acc: [p] words from the launch's column 0, the last column ragged.
template <int VEC>
__device__ __forceinline__ void trim_plane_load(const int32_t* plane, int64_t q, int64_t p, int (&dst)[VEC]) {
    const auto v = Lane<VEC>::load_tail(reinterpret_cast<const float*>(plane), q, p);
#pragma unroll
    for (int e = 0; e < VEC; ++e) dst[e] = __float_as_int(lane_get(v, e));
}
template <int VEC>
__device__ __forceinline__ void trim_plane_store(int32_t* plane, int64_t q, int64_t p, const int (&src)[VEC]) {
    typename Lane<VEC>::T v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) lane_put(v, e, __int_as_float(src[e]));
    Lane<VEC>::store_tail(reinterpret_cast<float*>(plane), q, p, v);
}

template <int B, int U, int VEC, int SRC>
__device__ __forceinline__ void trim_column(const FedavgArgs& a, const Rows rows, int64_t q) {
    using L = Lane<VEC>;
    using T = typename L::T;
    const int n = a.n_rows;
    const int64_t ld = a.map.ld;
    const float* col = a.diffs + a.map.at(VEC * q);
    TrimState<B, VEC> s;
    if (a.flags & FL_FIRST) {
#pragma unroll
        for (int j = 0; j < B; ++j)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                s.lo[j][e] = 0x7fffffff;
                s.hi[j][e] = (int)0x80000000;
            }
#pragma unroll
        for (int e = 0; e < VEC; ++e) s.acc[e] = 0.f;  // replaced at k == 2B
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j) {
            trim_plane_load<VEC>(a.tstate + (int64_t)j * a.tplane, q, a.p, s.lo[j]);
            trim_plane_load<VEC>(a.tstate + (int64_t)(B + j) * a.tplane, q, a.p, s.hi[j]);
        }
        const T v = L::load_tail(a.acc, q, a.p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s.acc[e] = lane_get(v, e);
    }
    // Full batches past the fill phase take the branch-free step; the batches of the fill phase
    // (k <= 2B: a prologue of at most ceil((2B + 1) / U) + 1 batches) and the last partial one take
    // the general step, whose branches are wave-uniform.
    for (int r = 0; r < n;) {
        const int nv = min(U, n - r);
        const int64_t k0 = a.client0 + r;
        T v[U];
        if (nv == U && k0 > 2 * B) {
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = L::template load<true>(col + row_at<SRC>(rows, r + u) * ld);
#pragma unroll
            for (int u = 0; u < U; ++u) trim_step<B, VEC, true>(s, v[u], k0 + u);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < nv) v[u] = L::template load<true>(col + row_at<SRC>(rows, r + u) * ld);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < nv) trim_step<B, VEC, false>(s, v[u], k0 + u);
        }
        r += nv;
    }
    if (a.flags & FL_FINAL) {
        T avg;
#pragma unroll
        for (int e = 0; e < VEC; ++e) lane_put(avg, e, s.acc[e] / a.divisor);
        L::store_tail(a.out, q, a.p, L::load_tail(a.ckpt, q, a.p) - avg);
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j) {
            trim_plane_store<VEC>(a.tstate + (int64_t)j * a.tplane, q, a.p, s.lo[j]);
            trim_plane_store<VEC>(a.tstate + (int64_t)(B + j) * a.tplane, q, a.p, s.hi[j]);
        }
        T v;
#pragma unroll
        for (int e = 0; e < VEC; ++e) lane_put(v, e, s.acc[e]);
        L::store_tail(a.acc, q, a.p, v);
    }
}

template <int B, int U, int TB, int VEC>
__global__ __launch_bounds__(TB) void k_fedavg_trim(FedavgArgs a, int64_t ncol) {
    const int64_t q = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (q < ncol) trim_column<B, U, VEC, 0>(a, Rows{}, q);
}

template <int B, int U, int TB, int VEC>
__global__ __launch_bounds__(TB) void k_fedavg_trim_rows(FedavgArgs a, int64_t ncol, RowTab tab) {
    const int64_t q = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (q < ncol) trim_column<B, U, VEC, 1>(a, Rows{&tab}, q);
}

// K9 / K9p: coordinate-wise median (MODE_MEDIAN; the definition is in include/pgh_api.h, the
// bisection in pgh_kernels.h).  Values are compared as u = key ^ 0x80000000, unsigned.
__device__ __forceinline__ uint32_t med_ukey(uint32_t b) { return b ^ (uint32_t)(((int)b >> 31) | (int)0x80000000); }
__device__ __forceinline__ float med_value(uint32_t u) { return __int_as_float(trim_key((int)(u ^ 0x80000000u))); }
// m = lower for an odd n, 0.5f * lower + 0.5f * upper (two rounded products, one rounded sum) for an even one
__device__ __forceinline__ float med_mid(uint32_t lower, uint32_t upper, bool even) {
    const float a = med_value(lower);
    return even ? __fadd_rn(__fmul_rn(0.5f, a), __fmul_rn(0.5f, med_value(upper))) : a;
}

// K9.  A tile = 64 consecutive columns; lane l of a wave owns column l of its tile, so a wave-wide
// load reads 256 contiguous bytes of one row.  The rows of a tile are split over the W waves of a
// workgroup (wave w holds rows w, w + W, ...: KPL keys per lane in registers), all KPL loads of a
// lane issued before the first use.  Places past n_rows hold the largest u, which no rank below
// n_rows reaches; lanes past p hold only those and store nothing (the slab's padding columns are
// never read).
// Per bit every lane counts its keys below T (v_cmp_lt_u32 + v_addc per key); with W > 1 the W
// counts of a column meet in LDS -- one ds_add per lane into one of three 64-word buffers used in
// turn (wave 0 clears the one of the bit before, so a bit costs one barrier), one read back -- and
// every lane of the column takes the same branch.  Per float: 3 (key) + 32 x 2 ops; per lane and
// bit two LDS operations on top.  W = 1 (up to 64 rows): a lane holds its whole column, no LDS and no
// barrier, four independent tiles per 256-thread workgroup.
template <int W, int KPL, int SRC>
__device__ __forceinline__ void median_tile(const MedianArgs& a, const Rows rows) {
    __shared__ uint32_t s_cnt[3][64];
    __shared__ uint32_t s_min[64];
    const int lane = threadIdx.x & 63;
    const int w = W == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t q = W == 1 ? (int64_t)blockIdx.x * blockDim.x + threadIdx.x : (int64_t)blockIdx.x * 64 + lane;
    const bool live = q < a.p;
    const int n = a.n_rows;
    const int64_t ld = a.map.ld;
    const uint32_t* col = reinterpret_cast<const uint32_t*>(a.diffs) + a.map.at(live ? q : 0);
    uint32_t k[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int r = w + W * j;
        k[j] = 0x7fffffffu;  // bits of the largest key
        if (r < n && live) k[j] = __builtin_nontemporal_load(col + row_at<SRC>(rows, r) * ld);
    }
    if constexpr (W > 1) {
        if (w == 0) {
            s_cnt[0][lane] = s_cnt[1][lane] = s_cnt[2][lane] = 0;
            s_min[lane] = 0xffffffffu;
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < KPL; ++j) k[j] = med_ukey(k[j]);
    const uint32_t rank = (uint32_t)(n - 1) >> 1;
    uint32_t pre = 0;
    int buf = 0;  // s_cnt[buf]: all zero here; s_cnt[buf + 2 (mod 3)] was read a barrier ago
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t T = pre | (1u << bit);
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < KPL; ++j) c += k[j] < T ? 1u : 0u;
        if constexpr (W > 1) {
            __hip_atomic_fetch_add(&s_cnt[buf][lane], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            c = s_cnt[buf][lane];
            const int old = buf == 0 ? 2 : buf - 1;
            if (w == 0) s_cnt[old][lane] = 0;  // every wave read it before this bit's barrier
            buf = buf == 2 ? 0 : buf + 1;
        }
        if (c <= rank) pre = T;
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
        if constexpr (W > 1) {
            __hip_atomic_fetch_add(&s_cnt[buf][lane], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(&s_min[lane], mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            c = s_cnt[buf][lane];
            mn = s_min[lane];
        }
        upper = c >= (uint32_t)(n / 2 + 1) ? pre : mn;
    }
    if (w == 0 && live) a.out[q] = a.ckpt[q] - med_mid(pre, upper, even);
}

template <int W, int KPL, int SRC>
__global__ __launch_bounds__(W == 1 ? BLOCK : 64 * W) void k_median(MedianArgs a) {
    median_tile<W, KPL, SRC>(a, Rows{nullptr, a.d_rows});
}
template <int W, int KPL>
__global__ __launch_bounds__(W == 1 ? BLOCK : 64 * W) void k_median_tab(MedianArgs a, RowTab tab) {
    median_tile<W, KPL, 1>(a, Rows{&tab});
}

// K9p: one step of the same bisection with the prefix in HBM: the K1 walk (one lane down its
// column, U loads in flight) counting instead of adding.  3 (key) + 2 ops per float and pass.
template <int SRC, int U>
__device__ __forceinline__ void median_pass(const MedianArgs& a, const Rows rows, int bit) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.p) return;
    const int n = a.n_rows;
    const int64_t ld = a.map.ld;
    const uint32_t* col = reinterpret_cast<const uint32_t*>(a.diffs) + a.map.at(q);
    const uint32_t pre = bit == 31 ? 0u : a.prefix[q];
    const bool upper_pass = bit < 0;
    const uint32_t T = upper_pass ? pre : pre | (1u << bit);
    uint32_t c = 0, mn = 0xffffffffu;
    for (int r = 0; r < n; r += U) {
        const int nv = min(U, n - r);
        uint32_t x[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u < nv) x[u] = __builtin_nontemporal_load(col + row_at<SRC>(rows, r + u) * ld);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u < nv) {
                const uint32_t key = med_ukey(x[u]);
                if (upper_pass) {
                    c += key <= T ? 1u : 0u;
                    mn = key > T ? min(mn, key) : mn;
                } else {
                    c += key < T ? 1u : 0u;
                }
            }
    }
    const bool even = !(n & 1);
    if (upper_pass) {
        a.out[q] = a.ckpt[q] - med_mid(pre, c >= (uint32_t)(n / 2 + 1) ? pre : mn, true);
        return;
    }
    const uint32_t next = c <= ((uint32_t)(n - 1) >> 1) ? T : pre;
    if (bit == 0 && !even) a.out[q] = a.ckpt[q] - med_mid(next, next, false);
    else a.prefix[q] = next;
}

template <int SRC>
__global__ __launch_bounds__(BLOCK) void k_median_pass(MedianArgs a, int bit) {
    median_pass<SRC, 16>(a, Rows{nullptr, a.d_rows}, bit);
}
__global__ __launch_bounds__(BLOCK) void k_median_pass_tab(MedianArgs a, int bit, RowTab tab) {
    median_pass<1, 16>(a, Rows{&tab}, bit);
}

// Z_2^64 lane element: VEC = 2 (16-byte column of 2 int64) or 1 (one int64 per lane).
template <int VEC> struct Lane64;
template <> struct Lane64<2> {
    using T = u64x2;
    template <bool NT> static __device__ __forceinline__ T load(const int64_t* p) { return ld2u<NT>(p); }
};
template <> struct Lane64<1> {
    using T = unsigned long long;
    template <bool NT> static __device__ __forceinline__ T load(const int64_t* p) {
        const T* q = reinterpret_cast<const T*>(p);
        if constexpr (NT) return __builtin_nontemporal_load(q);
        else return *q;
    }
};

template <int VEC>
__device__ __forceinline__ unsigned long long lane_elem(const typename Lane64<VEC>::T& v, int e) {
    if constexpr (VEC == 1) return v;
    else return v[e];
}

template <int VEC>
__device__ __forceinline__ void lane_set(typename Lane64<VEC>::T& v, int e, unsigned long long x) {
    if constexpr (VEC == 1) v = x;
    else v[e] = x;
}

template <int U, bool NT, int TB, int VEC>
__global__ __launch_bounds__(TB) void k_secagg(SecaggArgs a, int64_t ncol) {
    using L = Lane64<VEC>;
    using T = typename L::T;
    const int64_t stride = (int64_t)gridDim.x * TB;
    const int64_t ld = a.map.ld;
    for (int64_t q = (int64_t)blockIdx.x * TB + threadIdx.x; q < ncol; q += stride) {
        const int64_t i = VEC * q;
        const int64_t* col = a.shares + a.map.at(i);
        const int ne = (int)(i + VEC <= a.p ? VEC : a.p - i);  // valid elements of this column
        T acc{};
        if (!(a.flags & FL_FIRST))
            for (int e = 0; e < ne; ++e) lane_set<VEC>(acc, e, a.acc[i + e]);
        int r = 0;
        for (; r + U <= a.n_rows; r += U) {
            T v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = L::template load<NT>(col + (size_t)(r + u) * ld);
#pragma unroll
            for (int u = 0; u < U; ++u) acc += v[u];  // wraps mod 2^64
        }
        if (r < a.n_rows) {  // last partial batch, its loads in flight together
            const int nv = a.n_rows - r;
            T v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < nv) v[u] = L::template load<NT>(col + (size_t)(r + u) * ld);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < nv) acc += v[u];
        }
        for (int e = 0; e < ne; ++e) {
            const unsigned long long x = lane_elem<VEC>(acc, e);
            if (a.flags & FL_FINAL) {
                if (a.sum_out) a.sum_out[i + e] = (int64_t)x;
                if (a.dec_out) a.dec_out[i + e] = (float)(int64_t)x / a.divisor;  // float_prec decode
            } else {
                a.acc[i + e] = x;
            }
        }
    }
}

// Page-locked report ingest (pgh_ingest_state): one workgroup per chunk of a float payload that
// sits at an arbitrary byte offset of the DMA'd message.  After a head that brings the slab column
// to a multiple of 4, each lane moves 4 floats: one 16-byte load of the 4 dwords around them (plus
// the dword after, for an unaligned payload) funnel-shifted out (v_alignbyte), one 16-byte store
// into the blocked slab row (blocks are multiples of 64 columns, so 4 aligned columns never straddle
// one).  Bound by HBM like a copy: 4 B read + 4 B written per param, the message read once.
__global__ __launch_bounds__(BLOCK) void k_gather_f32(const uint8_t* bytes, const GChunk* tab, float* row,
                                                      SlabMap m) {
    const GChunk ch = tab[blockIdx.x];
    const int head = (int)min((int64_t)ch.n, (4 - (ch.dst & 3)) & 3);
    const int body = (ch.n - head) & ~3;
    const uint32_t sh = (uint32_t)(ch.src & 3);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(bytes + (ch.src & ~int64_t(3)));
    auto one = [&](int t) {
        const uint32_t lo = w[t];
        const uint32_t v = sh ? __builtin_amdgcn_alignbyte(w[t + 1], lo, sh) : lo;
        row[m.at(ch.dst + t)] = __uint_as_float(v);
    };
    if ((int)threadIdx.x < head) one((int)threadIdx.x);
    const int tail0 = head + body;
    if ((int)threadIdx.x < ch.n - tail0) one(tail0 + (int)threadIdx.x);
    for (int q = (int)threadIdx.x * 4; q < body; q += BLOCK * 4) {
        const int t = head + q;
        uint4 a;
        __builtin_memcpy(&a, w + t, 16);  // 4-byte aligned: a dwordx4 load (unaligned access is legal)
        float4 o;
        if (sh) {
            const uint32_t e = w[t + 4];
            o.x = __uint_as_float(__builtin_amdgcn_alignbyte(a.y, a.x, sh));
            o.y = __uint_as_float(__builtin_amdgcn_alignbyte(a.z, a.y, sh));
            o.z = __uint_as_float(__builtin_amdgcn_alignbyte(a.w, a.z, sh));
            o.w = __uint_as_float(__builtin_amdgcn_alignbyte(e, a.w, sh));
        } else {
            o = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w));
        }
        *reinterpret_cast<float4*>(row + m.at(ch.dst + t)) = o;
    }
}

// Decode of an already-summed Z_2^64 vector (client-sharded secagg: the per-rank share sums are
// reduce-scattered, then each rank decodes its param shard).  Same expression as k_secagg's
// FINAL epilogue, compiled with the same flags: bit-identical to the single-GPU decode.
__global__ __launch_bounds__(BLOCK) void k_secagg_decode(const int64_t* sum, float* dec, int64_t n, float divisor) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK)
        dec[i] = (float)sum[i] / divisor;
}

// K10 (pgh_kernels.h).  Every operation is one rounded f32 operation (-ffp-contract=off: no FMA); `/`
// and __builtin_sqrtf are the correctly rounded ones under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt (__fsqrt_rn is the native, approximate square root in
// this toolchain unless OCML's rounded operations are switched on, so it is not used).
template <int KIND>
__device__ __forceinline__ void server_opt_step(const ServerOptArgs& a, float d, float ck, float m, float v, float& out,
                                                float& m2, float& v2) {
    const float g = __uint_as_float(__float_as_uint(d) ^ 0x80000000u);
    if constexpr (KIND == 1) {
        m2 = a.beta1 * m + g;
        v2 = v;
        out = ck - a.lr * m2;
    } else {
        m2 = a.beta1 * m + a.c1 * g;
        const float q = g * g;
        if constexpr (KIND == 2) {
            v2 = v + q;
        } else if constexpr (KIND == 3) {
            v2 = a.beta2 * v + a.c2 * q;
        } else {
            const float sgn = v > q ? 1.0f : v < q ? -1.0f : 0.0f;
            v2 = v - (a.c2 * q) * sgn;
        }
        out = ck - (a.lr * m2) / (__builtin_sqrtf(v2) + a.tau);
    }
}

template <int KIND>
__global__ __launch_bounds__(BLOCK) void k_server_opt(ServerOptArgs a) {
    constexpr bool ADAPTIVE = KIND != 1;
    const int64_t ncol = (a.p + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < ncol; q += (int64_t)gridDim.x * BLOCK) {
        const int64_t i = 4 * q;
        f32x4 d, ck, m, v = {0.f, 0.f, 0.f, 0.f};
        if (i + 4 <= a.p) {
            d = ld4<true>(a.d + i);
            ck = ld4<false>(a.ckpt + i);
            m = ld4<false>(a.m + i);
            if constexpr (ADAPTIVE) v = ld4<false>(a.v + i);
        } else {
            d = ld4_tail(a.d, q, a.p);
            ck = ld4_tail(a.ckpt, q, a.p);
            m = ld4_tail(a.m, q, a.p);
            if constexpr (ADAPTIVE) v = ld4_tail(a.v, q, a.p);
        }
        f32x4 o, m2, v2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float oe, me, ve;
            server_opt_step<KIND>(a, d[e], ck[e], m[e], v[e], oe, me, ve);
            o[e] = oe;
            m2[e] = me;
            v2[e] = ve;
        }
        st4_tail(a.out, q, a.p, o);
        st4_tail(a.m2, q, a.p, m2);
        if constexpr (ADAPTIVE) st4_tail(a.v2, q, a.p, v2);
    }
}

// K11 (pgh_kernels.h; the sampler is defined operation by operation in include/pgh_api.h and restated
// for the host in pgh_host.cpp).  Every f64 operation is rounded on its own (-ffp-contract=off); `/` and
// __builtin_sqrt on doubles are the correctly rounded expansions (v_div_scale / v_div_fmas / v_div_fixup,
// v_rsq_f64 with its refinement and fix-up), not the OCML *_rn entry points (see K10 above).
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&x)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

__device__ __forceinline__ double dp_uniform(uint32_t lo, uint32_t hi) {
    const int64_t q = (int64_t)(((uint64_t)hi << 32) | lo) >> 11;  // arithmetic: 53 signed bits
    return ((double)q + 0.5) * 0x1p-52;                             // exact, symmetric, never 0
}

__device__ __forceinline__ double dp_plog(double s) {
    const uint64_t b = (uint64_t)__double_as_longlong(s);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    uint64_t mb = b & 0xfffffffffffffull;
    const bool big = mb >= 0x6a09e667f3bcdull;
    e += big ? 1 : 0;
    mb |= big ? 0x3fe0000000000000ull : 0x3ff0000000000000ull;
    const double m = __longlong_as_double((long long)mb);
    const double f = m - 1.0, t = f / (2.0 + f), w = t * t;
    double R = 1.479819860511658591e-01;
    R = R * w + 1.531383769920937332e-01;
    R = R * w + 1.818357216161805012e-01;
    R = R * w + 2.222219843214978396e-01;
    R = R * w + 2.857142874366239149e-01;
    R = R * w + 3.999999999940941908e-01;
    R = R * w + 6.666666666666735130e-01;
    R = R * w;
    return (double)e * 0x1.62e42fefa39efp-1 + (f - t * (f - R));
}

// The two standard normals of pair `pair`: the first of at most DP_ATTEMPTS polar attempts inside the
// unit circle (acceptance pi / 4 per attempt, so lanes of a wave retry for 1.3 rounds on average and the
// loop is bounded whatever the generator returns); +0.0 twice when every attempt was rejected.
__device__ __forceinline__ void dp_pair_normals(uint32_t k0, uint32_t k1, uint32_t round, uint64_t pair, double& z0,
                                                double& z1) {
    z0 = 0.0;
    z1 = 0.0;
    for (uint32_t at = 0; at < (uint32_t)DP_ATTEMPTS; ++at) {
        uint32_t x[4];
        philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), round, at, k0, k1, x);
        const double v1 = dp_uniform(x[0], x[1]), v2 = dp_uniform(x[2], x[3]);
        const double s = v1 * v1 + v2 * v2;
        if (s < 1.0) {
            const double f = __builtin_sqrt((-2.0 * dp_plog(s)) / s);
            z0 = v1 * f;
            z1 = v2 * f;
            break;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_dp_noise(DpNoiseArgs a) {
    const int64_t ncol = (a.p + 3) >> 2;
    const uint32_t k0 = (uint32_t)a.key, k1 = (uint32_t)(a.key >> 32);
    const bool to_out = a.ckpt != nullptr;
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < ncol; q += (int64_t)gridDim.x * BLOCK) {
        const int64_t i = 4 * q;
        const bool whole = i + 4 <= a.p;
        f32x4 d, ck = {0.f, 0.f, 0.f, 0.f};
        if (whole) {
            d = ld4<false>(a.d + i);
            if (to_out) ck = ld4<false>(a.ckpt + i);
        } else {
            d = ld4_tail(a.d, q, a.p);
            if (to_out) ck = ld4_tail(a.ckpt, q, a.p);
        }
        const uint64_t pair = (uint64_t)(a.i0 + i) >> 1;  // i0 + i is a multiple of 4: two whole pairs
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        dp_pair_normals(k0, k1, a.round, pair, z[0], z[1]);
        if (i + 2 < a.p) dp_pair_normals(k0, k1, a.round, pair + 1, z[2], z[3]);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float g = __uint_as_float(__float_as_uint(d[e]) ^ 0x80000000u);
            const float n = (float)(a.sigma * z[e]);  // one f64 product, one rounding to f32
            const float gn = g + n;
            o[e] = to_out ? ck[e] - gn : __uint_as_float(__float_as_uint(gn) ^ 0x80000000u);
        }
        st4_tail(a.out, q, a.p, o);
    }
}

// One lane per pair; the pairs that hold out[0] and out[n - 1] may lie half outside [i0, i0 + n).
__global__ __launch_bounds__(BLOCK) void k_dp_normals(uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out) {
    const int64_t pair0 = i0 >> 1, npairs = ((i0 + n - 1) >> 1) - pair0 + 1;
    for (int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (int64_t)gridDim.x * BLOCK) {
        double z0, z1;
        dp_pair_normals((uint32_t)key, (uint32_t)(key >> 32), round, (uint64_t)(pair0 + t), z0, z1);
        const int64_t k = 2 * (pair0 + t) - i0;  // -1 for the first pair of an odd i0
        if (k >= 0 && k < n) out[k] = z0;
        if (k + 1 >= 0 && k + 1 < n) out[k + 1] = z1;
    }
}

// KIND 0: one splitmix64 word per param -> Irwin-Hall(4 x u16).  KIND 1 ("fast", config 4's
// on-device data source): one word per 4 consecutive params (global index g >> 2), param g takes
// u16 number g & 3 of it, centred, times 2 * scale (same sigma ~ 1e-2): a quarter of the integer
// work, so the fill is bound by its HBM writes instead of the 64-bit multiplies (r01af).
// NT: non-temporal stores (the rows are read back by a fold only after the whole chunk is written:
// nothing to keep in L2 / MALL).
template <int KIND, bool NT>
__global__ __launch_bounds__(BLOCK) void k_synth_f32(float* out, SlabMap m, int64_t ncols, int n_rows, int64_t p,
                                                     uint64_t seed, uint64_t stream_id, int64_t row0, int64_t idx0,
                                                     float scale) {
    for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const uint64_t key = row_key(seed, stream_id, (uint64_t)(row0 + r));
        float* row = out + (size_t)r * m.ld;
        for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < ncols / 4; q += (int64_t)gridDim.x * BLOCK) {
            f32x4 v;
            if constexpr (KIND == 0) {
                const uint64_t k0 = key + (uint64_t)(idx0 + 4 * q);
                if (4 * q + 4 <= p) {  // branch-free: four independent hash chains interleave
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = bits_to_f32(sm64(k0 + (uint64_t)e), scale);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        v[e] = (4 * q + e < p) ? bits_to_f32(sm64(k0 + (uint64_t)e), scale) : 0.f;
                }
            } else {
                const float s2 = 2.0f * scale;  // exact
                const int64_t g0 = idx0 + 4 * q;
                if ((g0 & 3) == 0) {  // the four params share one word
                    const uint64_t h = sm64(key + (uint64_t)(g0 >> 2));
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        v[e] = (4 * q + e < p) ? (float)((int32_t)((h >> (16 * e)) & 0xFFFF) - 32768) * s2 : 0.f;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int64_t g = g0 + e;
                        const uint64_t h = sm64(key + (uint64_t)(g >> 2));
                        v[e] = (4 * q + e < p) ? (float)((int32_t)((h >> (16 * (g & 3))) & 0xFFFF) - 32768) * s2 : 0.f;
                    }
                }
            }
            f32x4* dst = reinterpret_cast<f32x4*>(row + m.at(4 * q));  // 4 params never straddle a block
            if constexpr (NT) __builtin_nontemporal_store(v, dst);
            else *dst = v;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_synth_shares(int64_t* out, SlabMap m, int64_t ncols, int n_parties,
                                                        int64_t p, uint64_t seed, int64_t client0, int64_t idx0,
                                                        float enc_scale) {
    const int64_t c = blockIdx.y;
    const uint64_t kx = row_key(seed, STREAM_SECRET, (uint64_t)(client0 + c));
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < ncols; i += (int64_t)gridDim.x * BLOCK) {
        int64_t* dst = out + (size_t)(c * n_parties) * m.ld + m.at(i);
        if (i >= p) {
            for (int s = 0; s < n_parties; ++s) dst[(size_t)s * m.ld] = 0;
            continue;
        }
        const uint64_t g = (uint64_t)(idx0 + i);
        const float x = bits_to_f32(sm64(kx + g), DIFF_SCALE);
        const float y = x * enc_scale;                  // fix_prec: x * base**prec in f32
        const uint64_t enc = (uint64_t)(int64_t)y;      // .long(): truncation toward zero
        uint64_t acc = 0;
        for (int s = 0; s < n_parties - 1; ++s) {
            const uint64_t sh = sm64(row_key(seed, STREAM_SHARE, (uint64_t)((client0 + c) * n_parties + s)) + g);
            dst[(size_t)s * m.ld] = (int64_t)sh;
            acc += sh;
        }
        dst[(size_t)(n_parties - 1) * m.ld] = (int64_t)(enc - acc);
    }
}

// Packed varints -> int64 (TensorData.contents_int64 of secagg share States): K4 below.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Inclusive prefix sum over a wave64 in DPP moves (row shifts inside each 16-lane row, then the
// row totals broadcast into the rows after them): no LDS round trips, unlike __shfl_up's
// ds_bpermute chain.
__device__ __forceinline__ int wave_inclusive_sum(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return x;
}

// The value whose bytes are win[s .. e] (s >= e - 9, win[-16 .. 1039] readable), from the 12 bytes
// at s (three funnel shifts of the four aligned dwords around it).  The 7-bit groups are summed
// whole bytes at a time in byte dot products: raw = sum_i b_i 128^i over bytes b_0 .. b_9, i.e.
// sum_i (v_i + 128 c_i) 128^i with v_i the 7-bit group and c_i the continuation bit.  c_i = 1 for
// every byte before the last (e), so raw = value + K(len) + (multiples of 2^(7 len) from the bytes
// past e), with K(len) = sum_{j=1}^{len-1} 2^(7j); subtracting K(10) differs from K(len) only by
// multiples of 2^(7 len) too, so value = (raw - K(10)) mod 2^(7 len) (all 64 bits at len 10).
__device__ __forceinline__ uint64_t varint_at(const uint8_t* win, int s, int e) {
    const uint32_t* wd = reinterpret_cast<const uint32_t*>(win + (s & ~3));
    const uint32_t d0 = wd[0], d1 = wd[1], d2 = wd[2], d3 = wd[3];
    const uint32_t sh = (uint32_t)(s & 3);
    const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, sh);  // bytes 0-3 of the value
    const uint32_t w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);  // 4-7
    const uint32_t w2 = __builtin_amdgcn_alignbyte(d3, d2, sh);  // 8-11
    constexpr uint32_t LO = 0x00008001u, HI = 0x80010000u;       // byte weights (1, 128, 0, 0), (0, 0, 1, 128)
    // b0 + 128 b1 + 2^14 (b2 + 128 b3) < 2^30: no wrap
    const uint32_t a = __builtin_amdgcn_udot4(w0, LO, 0u, false) + (__builtin_amdgcn_udot4(w0, HI, 0u, false) << 14);
    const uint32_t b = __builtin_amdgcn_udot4(w1, LO, 0u, false) + (__builtin_amdgcn_udot4(w1, HI, 0u, false) << 14);
    const uint32_t c = __builtin_amdgcn_udot4(w2, LO, 0u, false);  // b8 + 128 b9 (only b9's bit 0 stays, at 63)
    const uint64_t raw = (uint64_t)a + ((uint64_t)b << 28) + ((uint64_t)c << 56);
    constexpr uint64_t K10 = 0x8102040810204080ull;  // sum_{j=1}^{9} 2^(7j)
    const int cut = max(57 - __mul24(e - s, 7), 0);   // 64 - 7 len: the bits above the value (24-bit mul)
    return ((raw - K10) << cut) >> cut;
}

// Terminator bits of 16 bytes (bit k: byte k has bit 7 clear) in byte dot products: the 0x80 bytes
// of ~v & 0x80808080 weighted 1, 2, 4, 8 (16 .. 128 for the second dword) sum to 128 x the mask.
__device__ __forceinline__ uint32_t term_mask16(const u32x4& v) {
    const uint32_t t0 = ~v[0] & 0x80808080u, t1 = ~v[1] & 0x80808080u;
    const uint32_t t2 = ~v[2] & 0x80808080u, t3 = ~v[3] & 0x80808080u;
    const uint32_t m01 = __builtin_amdgcn_udot4(t0, 0x08040201u, __builtin_amdgcn_udot4(t1, 0x80402010u, 0u, false), false);
    const uint32_t m23 = __builtin_amdgcn_udot4(t2, 0x08040201u, __builtin_amdgcn_udot4(t3, 0x80402010u, 0u, false), false);
    return (m01 >> 7) | (m23 << 1);
}

// K4: one workgroup per chunk of <= VARINT_CHUNK bytes (16 KiB), one wave per 4 KiB of it.  Each
// wave loads its 4 KiB (four 1 KiB windows, 16 bytes per lane each) at once, counts the value ends
// (terminator bytes) in them, and the four counts -- one barrier -- give each wave its starting
// rank from the chunk's `first` (the host counts terminators per chunk while staging).  Then per
// window lane t decodes the values that END in its 16 bytes itself: a value is at most 10 bytes,
// so it starts in lane t's bytes or lane t - 1's, both staged in the wave's LDS window; its rank
// is a DPP wave prefix sum of the terminator counts, its start the last terminator of lane t - 1
// (DPP wave shift) or, for lane 0, the carry from the previous window (or the 16 bytes before the
// wave's 4 KiB).  The values leave through LDS by rank, in rows of 64 consecutive int64s.
// Rounds 2-5 ran a block form (a workgroup per 64 KiB chunk compacting the value ends of 4 KiB
// windows into an LDS list by rank, three barriers per window): 55.6-57.9 us per 111 MB message of
// shares against this form's 37.4-38.1 us (tools/exp_varint.cpp, profiles/r06m/, r06q/).
// Byte-level work on a stream PCIe fills at ~55 GB/s; HBM traffic is ~1.84 bytes per byte in.
constexpr int VWIN = 1024;                  // a window: 64 lanes x 16 bytes
constexpr int VSUB = 4096;                  // a wave's part of a chunk
constexpr int VNW = VSUB / VWIN;            // windows per wave
static_assert(VARINT_CHUNK == 4 * VSUB, "K4: four waves of VSUB bytes per chunk");
constexpr int VSTAGE = 256;  // values of a window staged per wave (int64 shares: <= 115 values of 9-10 bytes)
__global__ __launch_bounds__(256) void k_varint_decode(const uint8_t* bytes, const VChunk* chunks, int64_t* row,
                                                       SlabMap m, int64_t lo, int64_t hi) {
    __shared__ u32x4 lds[4][1 + 64 + 1];    // per wave: [0] the 16 bytes before the window, [65] slack
    __shared__ uint64_t stage[4][VSTAGE];    // per wave: the window's values by rank
    __shared__ int wcount[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32x4* const win4 = lds[wave];
    uint64_t* const stg = stage[wave];
    const uint8_t* const win = reinterpret_cast<const uint8_t*>(win4) + 16;  // win[-16 .. 1039]
    const VChunk ch = chunks[blockIdx.x];
    const int sub0 = wave * VSUB;                    // this wave's bytes: [sub0, sub0 + subn) of the chunk
    const int subn = max(0, min(VSUB, ch.n - sub0));  // (0 for the waves past a short chunk's end)
    const int p = 16 * lane;
    const u32x4 zero = {0, 0, 0, 0};
    // Loads are unconditional (a branch around a load makes hipcc wait for it at once): offsets past
    // the chunk clamp to its last 16 bytes, masked out by the byte counts; zero bytes before a
    // payload's start read as terminators (the first value starts at offset 0).
    const int last16 = (ch.n - 1) & ~15;
    const bool has_before = sub0 > 0 || ch.off > ch.span_off;
    const u32x4 b16 = *reinterpret_cast<const u32x4*>(bytes + ch.off + (has_before ? min(sub0, last16 + 16) - 16 : 0));
    u32x4 buf[VNW];
#pragma unroll
    for (int i = 0; i < VNW; ++i)
        buf[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(bytes + ch.off + min(sub0 + i * VWIN + p, last16)));
    // value ends per window (bit k: byte p + k ends a value), this wave's total, the waves before it
    uint32_t tms[VNW];
    int mine = 0;
#pragma unroll
    for (int i = 0; i < VNW; ++i) {
        uint32_t tm = term_mask16(buf[i]);
        const int lim = subn - i * VWIN - p;  // bytes of mine inside the wave's part
        if (lim < 16) tm &= lim > 0 ? (1u << lim) - 1u : 0u;
        tms[i] = tm;
        mine += __popc(tm);
    }
    const int wtot = __builtin_amdgcn_readlane(wave_inclusive_sum(mine), 63);
    if (lane == 0) wcount[wave] = wtot;
    __syncthreads();
    int64_t base = ch.first;
    for (int w = 0; w < wave; ++w) base += wcount[w];
    if (subn == 0) return;  // (after the barrier: every wave reaches it)
    const u32x4 before = has_before ? b16 : zero;
    const uint32_t tb = term_mask16(before);
    int carry = tb ? (31 - __clz(tb)) - 16 : -16;  // window offset of the last value end before the window
    if (lane == 0) win4[65] = zero;
    u32x4 last = before;  // lane 63: the previous window's last 16 bytes
#pragma unroll
    for (int i = 0; i < VNW; ++i) {
        if (i * VWIN >= subn) break;
        const u32x4 v = buf[i];
        const uint32_t tm = tms[i];
        win4[1 + lane] = v;
        if (lane == 63) win4[0] = last;
        const int cnt = __popc(tm);
        const int x = wave_inclusive_sum(cnt);
        const int total = __builtin_amdgcn_readlane(x, 63);
        // my last value end; lane t - 1's is where my first value starts (every full 16 bytes of
        // valid input hold a value end); lane 0 takes the carry
        const int mylast = tm ? p + 31 - __clz(tm) : -64;
        const int prev = __builtin_amdgcn_update_dpp(carry, mylast, 0x138, 0xf, 0xf, false);  // wave_shr:1
        const uint64_t with = __ballot(tm != 0);
        // the window's values inside the shard and in one slab block (the usual case): consecutive
        // addresses from one base
        const int64_t l0 = base - lo, l1 = base + total - 1 - lo;
        const bool flat = base >= lo && base + total <= hi && ((m.off + l0) >> m.bshift) == ((m.off + l1) >> m.bshift);
        int64_t* const dst0 = row + (flat ? m.at(l0) : 0);
        // LDS writes above, reads below: one wave, in order; keep the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int r = x - cnt, pe = prev;  // r: my first value's rank in the window
        uint32_t left = tm;
        auto next = [&]() -> uint64_t {  // my next value, in order (validated input: s >= e - 9)
            const int e = p + __ffs(left) - 1;
            const uint64_t val = varint_at(win, max(pe + 1, e - 9), e);
            pe = e;
            left &= left - 1;
            return val;
        };
        // wave-uniform branches: one loop per case rather than a branch per value (decoding a
        // lane's two values as two independent chains measured no faster, r06m)
        if (flat && total <= VSTAGE) {  // by rank into LDS, then out in rows of 64 consecutive values
            while (left) stg[r++] = next();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int q = lane; q < total; q += 64) dst0[q] = (int64_t)stg[q];
        } else if (flat) {  // a dense window (> VSTAGE values, short varints)
            while (left) dst0[r++] = (int64_t)next();
        } else {            // a shard or slab-block edge inside the window
            while (left) {
                const int64_t idx = base + r++;
                const uint64_t val = next();
                if (idx >= lo && idx < hi) row[m.at(idx - lo)] = (int64_t)val;
            }
        }
        if (with) carry = __builtin_amdgcn_readlane(mylast, 63 - __clzll(with));
        carry -= VWIN;
        base += total;
        last = v;
        // the next window's LDS writes come after this window's reads (in order within the wave)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// K7 and K12: sums of squares along slab rows (the clipping norm; the geometric median's distances to a moving
// point), the reductions here that run along a client's row instead of down a param column.  One tile body:
// a workgroup owns one tile of SUMSQ_TILE params and a chunk of RC rows, which it walks in groups of SUMSQ_RB
// rows.  Per group every lane issues its four 16-byte columns of all RB rows (4 RB non-temporal loads in
// flight) before it squares any, then each row is reduced on its own in the fixed order of pgh_kernels.h (lane
// partial -> shuffle tree per wave -> four wave sums through LDS).  The squares are exact in f64, so the fma
// below is the rounded add of the definition.  Addresses past the shard clamp to its last column and are masked
// to +0.0 (the slab's padding columns hold stale bytes); a chunk's last row group repeats its last row instead
// of branching around the loads.  The wave sums of every row of the chunk meet in LDS behind one barrier.
//   K7  (RC = SUMSQ_RB, OP = ROW_SQ): x = d_c[i]; one row group per workgroup.
//   K12 (RC = DISTSQ_RC, OP = ROW_DIST): x = d_c[i] + negv[i] (one f32 addition; negv holds -v, so this is d - v).
//       The workgroup brings its 16 KiB of the plane into registers once (16 floats per lane, plain loads: the
//       workgroups of the other row chunks read the same tile; clamped like the rows: the plane is at least p
//       long) and streams its rows past it, so the plane costs 1 / DISTSQ_RC of the slab's bytes instead of
//       1 / SUMSQ_RB.  The tile partials go where K7's go and k_row_sumsq_fold[_rows] finishes the rows.
//   K14 (RC = DISTSQ_RC, OP = ROW_DOT): the sum runs over (double)d_c[i] * (double)g0[i], the plane (`negv`) holding
//       g0 itself: K12's shape with a convert of the plane's value in place of the f32 addition.  The product of
//       two f32 values is exact in f64, so the fma is again the rounded add.  Past p both factors are masked: the
//       product is +0.0 there, never 0 x NaN.  A tile partial may be negative, but not -0.0: a lane's sum starts
//       at +0.0, and +0.0 + (-0.0) and every exact cancellation round to +0.0.
constexpr int SUMSQ_RB = 4;

enum RowOp : int { ROW_SQ = 0, ROW_DIST = 1, ROW_DOT = 2 };

template <int SRC, int RC, int OP>
__device__ __forceinline__ void row_sq_tile(const SumsqArgs& a, const float* negv, const Rows rows) {
    __shared__ double wsum[RC][4];
    const int lane = threadIdx.x, wave = lane >> 6;
    const int64_t t = blockIdx.x, base = t * SUMSQ_TILE;
    const int r0 = (int)blockIdx.y * RC;
    const int nr = min(RC, a.n_rows - r0);
    const bool full = base + SUMSQ_TILE <= a.p;
    const int64_t last4 = (a.p - 1) & ~int64_t(3);
    int64_t idx[4], off[4];
    f32x4 nv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        idx[j] = base + 4 * (lane + BLOCK * j);
        const int64_t i = full ? idx[j] : min(idx[j], last4);
        off[j] = a.map.at(i);
        if constexpr (OP != ROW_SQ) nv[j] = ld4<false>(negv + i);
    }
    const int ng = RC == SUMSQ_RB ? SUMSQ_RB : nr;  // (nr is uniform over the workgroup; K7: one trip)
#pragma unroll 1
    for (int g = 0; g < ng; g += SUMSQ_RB) {
        size_t row[SUMSQ_RB];
#pragma unroll
        for (int rr = 0; rr < SUMSQ_RB; ++rr) row[rr] = row_at<SRC>(rows, r0 + min(g + rr, nr - 1));
        f32x4 v[SUMSQ_RB][4];
#pragma unroll
        for (int rr = 0; rr < SUMSQ_RB; ++rr)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[rr][j] = ld4<true>(a.slab + row[rr] * (size_t)a.map.ld + off[j]);
#pragma unroll
        for (int rr = 0; rr < SUMSQ_RB; ++rr) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = full || idx[j] + e < a.p;
                    const float xf = OP == ROW_DIST ? v[rr][j][e] + nv[j][e] : v[rr][j][e];
                    const double x = in ? (double)xf : 0.0;
                    double y = x;
                    if constexpr (OP == ROW_DOT) {
                        // K14: both factors masked, so the product past p is +0.0 whatever the padding holds.  The
                        // plane's value is converted at each use: the empty asm keeps the compiler from holding the
                        // tile as 16 doubles across the row loop, 32 VGPRs and one wave of occupancy more than K12.
                        float yf = nv[j][e];
                        asm volatile("" : "+v"(yf));
                        y = in ? (double)yf : 0.0;
                    }
                    acc = __builtin_fma(x, y, acc);
                }
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) acc += __shfl_down(acc, h, 64);
            if ((lane & 63) == 0) wsum[g + rr][wave] = acc;  // (g + rr < RC: a multiple of SUMSQ_RB)
        }
    }
    __syncthreads();
    if (lane < nr)
        a.part[row_at<SRC>(rows, r0 + lane) * (size_t)a.ntiles + (size_t)t] =
            ((wsum[lane][0] + wsum[lane][1]) + wsum[lane][2]) + wsum[lane][3];
}

__global__ __launch_bounds__(BLOCK) void k_row_sumsq(SumsqArgs a) {
    row_sq_tile<0, SUMSQ_RB, ROW_SQ>(a, nullptr, Rows{nullptr, nullptr, a.row0});
}
__global__ __launch_bounds__(BLOCK) void k_row_sumsq_rows(SumsqArgs a, RowTab tab) { row_sq_tile<1, SUMSQ_RB, ROW_SQ>(a, nullptr, Rows{&tab}); }
__global__ __launch_bounds__(BLOCK) void k_row_distsq(DistsqArgs d) {
    row_sq_tile<0, DISTSQ_RC, ROW_DIST>(d.s, d.negv, Rows{nullptr, nullptr, d.s.row0});
}
__global__ __launch_bounds__(BLOCK) void k_row_distsq_rows(DistsqArgs d, RowTab tab) { row_sq_tile<1, DISTSQ_RC, ROW_DIST>(d.s, d.negv, Rows{&tab}); }
__global__ __launch_bounds__(BLOCK) void k_row_dot(DistsqArgs d) {
    row_sq_tile<0, DISTSQ_RC, ROW_DOT>(d.s, d.negv, Rows{nullptr, nullptr, d.s.row0});
}
// (K12's occupancy: without the hint the table form takes 101 VGPRs, 5 past the step to 4 waves per SIMD)
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(5))) void k_row_dot_rows(DistsqArgs d, RowTab tab) { row_sq_tile<1, DISTSQ_RC, ROW_DOT>(d.s, d.negv, Rows{&tab}); }

// The row's tile partials, left-folded in ascending tile order by one lane; the workgroup brings
// them into LDS 1,024 at a time (coalesced) so the serial chain reads LDS, not HBM.
constexpr int SUMSQ_FOLD_CHUNK = 4 * BLOCK;

// (every lane returns; lane 0 holds the sum)
__device__ __forceinline__ double tile_partials_fold(const double* part, int64_t ntiles) {
    __shared__ double buf[SUMSQ_FOLD_CHUNK];
    double acc = 0.0;  // + 0.0 + partial 0 is partial 0 (partials are never -0.0, K14's signed ones included)
    for (int64_t c0 = 0; c0 < ntiles; c0 += SUMSQ_FOLD_CHUNK) {
        const int m = (int)min((int64_t)SUMSQ_FOLD_CHUNK, ntiles - c0);
        for (int k = threadIdx.x; k < m; k += BLOCK) buf[k] = part[c0 + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < m; ++k) acc += buf[k];
        __syncthreads();
    }
    return acc;
}

template <int SRC>
__device__ __forceinline__ void row_sumsq_fold(const SumsqArgs& a, const Rows rows) {
    const size_t row = row_at<SRC>(rows, (int)blockIdx.x);
    const double acc = tile_partials_fold(a.part + row * (size_t)a.ntiles, a.ntiles);
    if (threadIdx.x == 0) a.sumsq[row] = acc;
}

__global__ __launch_bounds__(BLOCK) void k_row_sumsq_fold(SumsqArgs a) { row_sumsq_fold<0>(a, Rows{nullptr, nullptr, a.row0}); }
__global__ __launch_bounds__(BLOCK) void k_row_sumsq_fold_rows(SumsqArgs a, RowTab tab) { row_sumsq_fold<1>(a, Rows{&tab}); }

// K13: every pairwise squared distance among the listed rows (Multi-Krum's scores), K12's sum for each pair.
// A workgroup owns one tile, a block of PAIRDIST_RA anchor rows and a chunk of PAIRDIST_RC later rows of the
// list: the anchors' tile comes into registers once (16 floats per lane and anchor; K12's nv[] is the
// one-anchor case) and the chunk streams past in K7's row groups, every (anchor, streamed row) pair reduced on
// its own in K7's order over x = anchor - row (one f32 subtraction; the square of the other way round is the
// same, so one triangle serves both).  Only pairs with list index b > a are stored.  The workgroups of one tile
// are neighbours in the grid (chunk fastest, then anchor block, then tile) and load plainly, so the tile of a
// row is fetched from HBM about once and served from the caches to the other anchor blocks.  Addresses past
// the shard clamp and mask as in K7; a short anchor block or row group repeats its last row.
template <int SRC>
__device__ __forceinline__ void row_pairdist_tile(const PairdistArgs& a) {
    __shared__ double wsum[PAIRDIST_RA][PAIRDIST_RC][4];
    const Rows rows{nullptr, a.d_rows, a.row0};
    const int lane = threadIdx.x, wave = lane >> 6;
    const int nabs = (a.na + PAIRDIST_RA - 1) / PAIRDIST_RA;
    const int chunk = (int)(blockIdx.x % (unsigned)a.nchunks);
    const int ab = (int)((blockIdx.x / (unsigned)a.nchunks) % (unsigned)nabs);
    const int64_t t = blockIdx.x / ((unsigned)a.nchunks * (unsigned)nabs), base = t * SUMSQ_TILE;
    const int ab0 = a.a0 + ab * PAIRDIST_RA;                 // the block's first anchor (list index)
    const int nra = min(PAIRDIST_RA, a.a0 + a.na - ab0);
    const int b0 = ab0 + 1 + chunk * PAIRDIST_RC;            // the chunk's first streamed row
    const int nr = min(PAIRDIST_RC, a.n - b0);
    if (nr <= 0) return;  // (uniform over the workgroup: the triangle leaves the later chunks of a late block empty)
    const bool full = base + SUMSQ_TILE <= a.p;
    const int64_t last4 = (a.p - 1) & ~int64_t(3);
    int64_t idx[4], off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        idx[j] = base + 4 * (lane + BLOCK * j);
        off[j] = a.map.at(full ? idx[j] : min(idx[j], last4));
    }
    f32x4 av[PAIRDIST_RA][4];
#pragma unroll
    for (int ra = 0; ra < PAIRDIST_RA; ++ra) {
        const size_t row = row_at<SRC>(rows, ab0 + min(ra, nra - 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) av[ra][j] = ld4<false>(a.slab + row * (size_t)a.map.ld + off[j]);
    }
#pragma unroll 1
    for (int g = 0; g < nr; g += SUMSQ_RB) {
        f32x4 v[SUMSQ_RB][4];
#pragma unroll
        for (int rr = 0; rr < SUMSQ_RB; ++rr) {
            const size_t row = row_at<SRC>(rows, b0 + min(g + rr, nr - 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) v[rr][j] = ld4<false>(a.slab + row * (size_t)a.map.ld + off[j]);
        }
#pragma unroll
        for (int ra = 0; ra < PAIRDIST_RA; ++ra)
#pragma unroll
            for (int rr = 0; rr < SUMSQ_RB; ++rr) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float xf = av[ra][j][e] - v[rr][j][e];
                        const double x = (full || idx[j] + e < a.p) ? (double)xf : 0.0;
                        acc = __builtin_fma(x, x, acc);
                    }
#pragma unroll
                for (int h = 32; h >= 1; h >>= 1) acc += __shfl_down(acc, h, 64);
                if ((lane & 63) == 0) wsum[ra][g + rr][wave] = acc;  // (g + rr < PAIRDIST_RC: a multiple of SUMSQ_RB)
            }
    }
    __syncthreads();
    const int ra = lane / PAIRDIST_RC, rr = lane % PAIRDIST_RC;  // one pair per lane
    const int ia = ab0 + ra, ib = b0 + rr;
    if (ra < nra && rr < nr && ib > ia)
        a.part[((size_t)(ia - a.a0) * (size_t)a.n + (size_t)ib) * (size_t)a.ntiles + (size_t)t] =
            ((wsum[ra][rr][0] + wsum[ra][rr][1]) + wsum[ra][rr][2]) + wsum[ra][rr][3];
}

__global__ __launch_bounds__(BLOCK) void k_row_pairdist(PairdistArgs a) { row_pairdist_tile<0>(a); }
__global__ __launch_bounds__(BLOCK) void k_row_pairdist_rows(PairdistArgs a) { row_pairdist_tile<2>(a); }

// The pair's tile partials left to right, as a row's: workgroup (b, a - a0) of the launch's anchors.
__global__ __launch_bounds__(BLOCK) void k_row_pairdist_fold(PairdistArgs a) {
    const int ia = a.a0 + (int)blockIdx.y, ib = (int)blockIdx.x;
    if (ib <= ia) return;  // (uniform over the workgroup)
    const double acc =
        tile_partials_fold(a.part + ((size_t)blockIdx.y * (size_t)a.n + (size_t)ib) * (size_t)a.ntiles, a.ntiles);
    if (threadIdx.x == 0) a.dist[(size_t)ia * (size_t)a.n + (size_t)ib] = acc;
}

int cu_count() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// The launch shapes are the rows of pgh_variants.def; these are the words its columns are written in.
// nt loads won 2-5 % on the once-read diff stream (r01c).  Small shards are bound by lanes / CU
// balance, not by the loads: the auto choice (variant -1) picks by shard size and mode
// (auto_variant below, r01l measurements on the column-blocked slab).
namespace shape {
enum Grid { tile, persistent, pipelined, xmap };
constexpr bool nt = true, plain = false, rowtab = true, no_rowtab = false;
}  // namespace shape

inline unsigned grid_for(int64_t ncol, int64_t tile, bool persistent) {
    const int64_t full = (ncol + tile - 1) / tile;
    if (!persistent) return (unsigned)(full > 0 ? full : 1);
    const int64_t pers = (int64_t)cu_count() * 4;
    return (unsigned)(full < pers ? (full > 0 ? full : 1) : pers);
}

// One fold shape.  With a row table it runs k_fedavg_rows, which exists for the TAB shapes only
// (launch_fedavg sends no other shape a table).
template <int MODE, bool NT, int U, int W, int TB, int VEC, shape::Grid G, bool TAB>
hipError_t go_fedavg(const FedavgArgs& a, const Rows& rows, hipStream_t s) {
    static_assert(G != shape::pipelined || W == 1, "the pipelined walk has one column per lane");
    static_assert(!TAB || G == shape::tile, "k_fedavg_rows has the plain grid");
    const int64_t ncol = (a.p + VEC - 1) / VEC;
    const unsigned grid = grid_for(ncol, (int64_t)TB * W, G == shape::persistent);
    if (rows.tab) {
        if constexpr (TAB) k_fedavg_rows<MODE, U, W, NT, TB, VEC><<<grid, TB, 0, s>>>(a, ncol, *rows.tab);
        else return hipErrorInvalidValue;
    } else if constexpr (G == shape::pipelined) {
        k_fedavg_pipe<MODE, U, NT, TB, VEC><<<grid, TB, 0, s>>>(a, ncol);
    } else {
        k_fedavg<MODE, U, W, NT, TB, VEC, G == shape::xmap><<<grid, TB, 0, s>>>(a, ncol);
    }
    return hipGetLastError();
}

template <int MODE>
hipError_t dispatch_fedavg(const FedavgArgs& a, const Rows& rows, int variant, hipStream_t s) {
    using namespace shape;
    switch (variant) {
#define PGH_FOLD(id, loads, U, W, block, VEC, grid, tab) \
    case id: return go_fedavg<MODE, loads, U, W, block, VEC, grid, tab>(a, rows, s);
#include "pgh_variants.def"
    default: return hipErrorInvalidValue;
    }
}

// Whether the fold of that id has a row-table kernel.
constexpr bool has_rowtab(int variant) {
    using namespace shape;
    switch (variant) {
#define PGH_FOLD(id, loads, U, W, block, VEC, grid, tab) case id: return tab;
#include "pgh_variants.def"
    default: return false;
    }
}
static_assert(has_rowtab(0), "a row-table fold without a kernel of its own id runs id 0's shape");

// K8 shapes: 16-byte columns in 256-thread blocks with 8 rows in flight (the mean's big-shard shape,
// variant 0), or one param per lane in 64-thread blocks with 32 rows in flight (its small-shard
// shape, variant 14).  Registers per lane: (2B + 1) VEC of state + U VEC of rows.
template <int B, int VEC>
hipError_t go_trim(const FedavgArgs& a, const RowTab* t, hipStream_t s) {
    constexpr int TB = VEC == 4 ? 256 : 64, U = VEC == 4 ? 8 : 32;
    const int64_t ncol = (a.p + VEC - 1) / VEC;
    const unsigned grid = grid_for(ncol, TB, false);
    if (t) k_fedavg_trim_rows<B, U, TB, VEC><<<grid, TB, 0, s>>>(a, ncol, *t);
    else k_fedavg_trim<B, U, TB, VEC><<<grid, TB, 0, s>>>(a, ncol);
    return hipGetLastError();
}

template <int VEC>
hipError_t dispatch_trim(const FedavgArgs& a, const RowTab* t, hipStream_t s) {
    switch (a.trim_b) {
    case 1: return go_trim<1, VEC>(a, t, s);
    case 2: return go_trim<2, VEC>(a, t, s);
    case 3: return go_trim<3, VEC>(a, t, s);
    case 4: return go_trim<4, VEC>(a, t, s);
    case 5: return go_trim<5, VEC>(a, t, s);
    case 6: return go_trim<6, VEC>(a, t, s);
    case 7: return go_trim<7, VEC>(a, t, s);
    case 8: return go_trim<8, VEC>(a, t, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

// K8's column width: the mean's threshold between one param per lane and 16-byte columns (below
// ~360 K params the 16-byte columns leave CUs without lanes, auto_variant).
int auto_trim_vec(int64_t p, int b) {
    (void)b;
    return p < 360000 ? 1 : 4;
}

// Measured on MI355X, column-blocked slab (r01l, tools/sweep_r01l.sh; GB/s of algorithmic bytes):
//   P = 11.69M x 1K:     mean v0 6930 / v6 6921 / v15 6882 / v11 6861 / v14 6576
//                        iterative v0 6845 / v6 6828 / v15 6817;  weighted v15 7035 / v0 6921
//   P = 3M x 1K:         mean v6 6829 / v0 6822 / v15 6773;  iterative v6 6619 / v0 6615
//   P = 1M x 3K:         mean v0 6921 / v6 6912 / v11 6769;  iterative v0 6753 / v6 6555
//   P = 311,650 x 10K:   mean v11 6885 / v15 6645 / v0 5753;  iterative v12 5711 / v14 5670 / v11 5351
//   P = 100K x 30K:      mean v11 6403 / v12 6251;  iterative v14 4742 / v12 4465 / v11 2784
//   single block (P < 65,536; layout unchanged from r01g): P = 50K x 60K v14 6088 / v12 4013
// Pipelined walk (r01w): P = 11.69M x 1K mean v0 6809 / v21 6798 / v22 6822, iterative 6834 / 6864 /
//   6834, weighted 6816 / 6831 / 6820; 1M x 3K and 12.5M x 1K within 0.4 %: not latency-bound.
// Iterative fold with the reciprocal-multiply division (r01o, tools/ab_iterative.sh):
//   P = 50K x 60K v17 3665 / v14 3496;  100K x 30K v14 5970 / v17 5616;  311,650 x 10K v11 6359 /
//   v14 5894;  1M x 3K v0 6755;  11.69M x 1K v0 6846  (IEEE division: 3209 / 4757 / 5784 / 6753 / 6845)
// Big shards: 16-byte columns in 256-thread blocks (the blocked slab made them 5 % faster than one
// param per lane).  Below ~786K params those give < 768 workgroups for 256 CUs, so 64-thread
// blocks (CU balance); below ~200K params one param per lane (lanes), with deeper row pipelines
// for the iterative fold of the smallest shards (few waves: latency).
int auto_variant(int64_t p, int mode) {
    // under 80 K params (many clients per launch): the mean's 64-row walk (v17) up to ~45 K
    // (+10-37 % over v14 at 10-40 K x 3,000), the iterative fold's 32-row walk in 128-thread blocks
    // (v18) from ~35 K (+7-29 % over v17 at 40-65 K; below that the division chain ties them all),
    // weighted unchanged, r02ax / r02ay
    if (p < 80000) {
        if (mode == MODE_ITERATIVE) return p < 35000 ? 17 : 18;
        return mode == MODE_MEAN && p < 45000 ? 17 : 14;
    }
    // 80-125 K: the weighted fold on one param per lane with 16 rows in flight (v12: +21 % at
    // 100 K x 3,000; at 150-190 K v11 matches or beats it, r02bc / r02bd)
    if (p < 200000) return mode == MODE_ITERATIVE ? 14 : mode == MODE_WEIGHTED && p < 125000 ? 12 : 11;
    // between 200 K and 786 K params: the iterative fold takes one param per lane in 256-thread
    // blocks up to ~360 K (v13: 5.9-6.6 TB/s vs v11's 4.5-5.4 at 200-311 K x 1,000) and the
    // 16-byte columns of v0 above (6.3-6.7 vs 6.1-6.5); the mean takes v13 up to ~360 K too
    // (6.5 vs 5.9 at 200 K, equal at 250-350 K); weighted stays on v11 (mixed), r02ar-r02au
    if (p < 786432) {
        if (mode == MODE_ITERATIVE) return p < 360000 ? 13 : 0;
        return mode == MODE_MEAN && p < 360000 ? 13 : 11;
    }
    return 0;  // r01p (masked last batch): mean 6918, iterative 6910, weighted 6905 (v15 6647)
}

template <bool NT, int U, int TB, int VEC, shape::Grid G>
hipError_t go_secagg(const SecaggArgs& a, hipStream_t s) {
    static_assert(G == shape::tile || G == shape::persistent, "the share sum has these two grids");
    const int64_t ncol = (a.p + VEC - 1) / VEC;
    k_secagg<U, NT, TB, VEC><<<grid_for(ncol, TB, G == shape::persistent), TB, 0, s>>>(a, ncol);
    return hipGetLastError();
}

// Geometry a kernel may rely on: rows 16-byte aligned (ld a multiple of 4), blocks
// power-of-two wide (or one block holding the launch's columns), the launch's first column
// 4-aligned so a 16-byte column never straddles a block.
bool valid_map(const SlabMap& m, int64_t p) {
    if (m.ld <= 0 || (m.ld & 3) || (m.off & 3) || m.off < 0) return false;
    if (m.bshift == 62) return m.bmask == (int64_t(1) << 62) - 1 && m.off + p <= m.ld;
    return m.bshift > 0 && m.bshift < 40 && (int64_t(1) << m.bshift) == m.ld && m.bmask == m.ld - 1 && m.bstride >= m.ld;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// What a family takes as its Rows.  device_table: it has a kernel that reads one; from_row0: its
// contiguous rows may start past the slab pointer (K7).
static bool valid_rows(const Rows& r, int n_rows, bool device_table, bool from_row0) {
    if (r.tab && r.d_rows) return false;
    if (r.tab && n_rows > ROWTAB_MAX) return false;
    if (r.d_rows && !device_table) return false;
    return r.row0 == 0 || (from_row0 && r.row0 > 0 && !r.tab && !r.d_rows);
}

// MODE_TRIMMED behind the common checks of launch_fedavg.
static hipError_t launch_trim(const FedavgArgs& a, const RowTab* t, hipStream_t s) {
    if (a.trim_b < 1 || a.trim_b > TRIM_MAX || a.client0 < 0) return hipErrorInvalidValue;
    if (a.trim_vec != 0 && a.trim_vec != 1 && a.trim_vec != 4) return hipErrorInvalidValue;
    if ((a.flags & (FL_FIRST | FL_FINAL)) != (FL_FIRST | FL_FINAL) &&
        (!a.tstate || !aligned16(a.tstate) || a.tplane < a.p || (a.tplane & 3)))
        return hipErrorInvalidValue;
    if ((a.flags & FL_FIRST) && a.client0 != 0) return hipErrorInvalidValue;
    const int vec = a.trim_vec ? a.trim_vec : auto_trim_vec(a.p, a.trim_b);
    return vec == 4 ? dispatch_trim<4>(a, t, s) : dispatch_trim<1>(a, t, s);
}

static bool valid_fedavg(const FedavgArgs& a, const Rows& rows) {
    if (!valid_rows(rows, a.n_rows, false, false)) return false;
    if (a.p <= 0 || a.n_rows < 0 || !valid_map(a.map, a.p)) return false;
    if ((a.flags & FL_FIRST) && a.n_rows < 1) return false;
    if (a.n_rows > 0 && (!a.diffs || !aligned16(a.diffs))) return false;
    if ((a.flags & (FL_FIRST | FL_FINAL)) != (FL_FIRST | FL_FINAL) && (!a.acc || !aligned16(a.acc))) return false;
    if ((a.flags & FL_FINAL) && (!a.ckpt || !a.out || !aligned16(a.ckpt) || !aligned16(a.out))) return false;
    if (a.mode == MODE_WEIGHTED && a.n_rows > 0 && !a.weights) return false;
    if (a.mode == MODE_ITERATIVE && a.n_rows > 0 && !a.recips) return false;
    return true;
}

// Contiguous rows: a.variant, or the auto choice when it is negative.  A row table: a.variant where
// that id has a row-table kernel (pgh_variants.def), the auto choice for every other value; an auto
// choice without such a kernel (12, 13, 18) runs id 0's shape.
hipError_t launch_fedavg(const FedavgArgs& a, const Rows& rows, hipStream_t s) {
    if (!valid_fedavg(a, rows)) return hipErrorInvalidValue;
    if (a.mode == MODE_TRIMMED) return launch_trim(a, rows.tab, s);
    int v = a.variant;
    if (rows.tab ? !has_rowtab(v) : v < 0) v = auto_variant(a.p, a.mode);
    if (rows.tab && !has_rowtab(v)) v = 0;
    switch (a.mode) {
    case MODE_MEAN: return dispatch_fedavg<MODE_MEAN>(a, rows, v, s);
    case MODE_ITERATIVE: return dispatch_fedavg<MODE_ITERATIVE>(a, rows, v, s);
    case MODE_WEIGHTED: return dispatch_fedavg<MODE_WEIGHTED>(a, rows, v, s);
    default: return hipErrorInvalidValue;
    }
}

// The kernel's arguments: a with the device table of rows in it (k_median<.., 2> reads it from there).
static bool median_args(const MedianArgs& a, const Rows& rows, MedianArgs* k) {
    if (!valid_rows(rows, a.n_rows, true, false)) return false;
    if (a.p <= 0 || a.n_rows < 1 || !valid_map(a.map, a.p)) return false;
    if (!a.diffs || !aligned16(a.diffs) || !a.ckpt || !a.out) return false;
    *k = a;
    k->d_rows = rows.d_rows;
    return true;
}

template <int W, int KPL>
static hipError_t go_median(const MedianArgs& k, const RowTab* t, hipStream_t s) {
    constexpr int TB = W == 1 ? BLOCK : 64 * W;
    const unsigned grid = grid_for(k.p, W == 1 ? BLOCK : 64, false);
    if (t) k_median_tab<W, KPL><<<grid, TB, 0, s>>>(k, *t);
    else if (k.d_rows) k_median<W, KPL, 2><<<grid, TB, 0, s>>>(k);
    else k_median<W, KPL, 0><<<grid, TB, 0, s>>>(k);
    return hipGetLastError();
}

// K9's tiers (waves per tile x keys per lane): up to 64 rows a lane holds its whole column, in 8, 16,
// 32 or 64 registers; up to 128 / 256 / 512 / 1,024 rows 2 / 4 / 8 / 16 waves hold 64 keys per lane.
hipError_t launch_median(const MedianArgs& a, const Rows& rows, hipStream_t s) {
    MedianArgs k;
    const RowTab* t = rows.tab;
    if (!median_args(a, rows, &k) || a.n_rows > MEDIAN_NCHIP) return hipErrorInvalidValue;
    if (a.n_rows <= 8) return go_median<1, 8>(k, t, s);
    if (a.n_rows <= 16) return go_median<1, 16>(k, t, s);
    if (a.n_rows <= 32) return go_median<1, 32>(k, t, s);
    if (a.n_rows <= 64) return go_median<1, 64>(k, t, s);
    if (a.n_rows <= 128) return go_median<2, 64>(k, t, s);
    if (a.n_rows <= 256) return go_median<4, 64>(k, t, s);
    if (a.n_rows <= 512) return go_median<8, 64>(k, t, s);
    return go_median<MEDIAN_WAVES, 64>(k, t, s);
}

hipError_t launch_median_pass(const MedianArgs& a, const Rows& rows, int bit, hipStream_t s) {
    MedianArgs k;
    if (!median_args(a, rows, &k) || !a.prefix || bit < -1 || bit > 31) return hipErrorInvalidValue;
    if (bit < 0 && (a.n_rows & 1)) return hipErrorInvalidValue;  // an odd n closes at bit 0
    const unsigned grid = grid_for(a.p, BLOCK, false);
    if (rows.tab) k_median_pass_tab<<<grid, BLOCK, 0, s>>>(k, bit, *rows.tab);
    else if (k.d_rows) k_median_pass<2><<<grid, BLOCK, 0, s>>>(k, bit);
    else k_median_pass<0><<<grid, BLOCK, 0, s>>>(k, bit);
    return hipGetLastError();
}

hipError_t launch_secagg(const SecaggArgs& a, hipStream_t s) {
    using namespace shape;
    if (a.p <= 0 || a.n_rows < 0 || !valid_map(a.map, a.p)) return hipErrorInvalidValue;
    if (a.n_rows > 0 && (!a.shares || (reinterpret_cast<uintptr_t>(a.shares) & 15))) return hipErrorInvalidValue;
    if (!(a.flags & FL_FINAL) && !a.acc) return hipErrorInvalidValue;
    if (!(a.flags & FL_FIRST) && !a.acc) return hipErrorInvalidValue;
    // auto: one int64 per lane, 32 rows in flight, 64-thread blocks (r01l, blocked slab: 6878 GB/s
    // at ResNet-18 x 1,000 x 2 (v16 6886, 16-byte columns v0 6613), 6747 at 311,650 x 2,500 x 2)
    const int v = a.variant < 0 ? SECAGG_AUTO_VARIANT : a.variant;
    if (v >= N_VARIANTS) return hipErrorInvalidValue;
    switch (v) {
#define PGH_SECAGG(id, loads, U, block, VEC, grid) case id: return go_secagg<loads, U, block, VEC, grid>(a, s);
#define PGH_SECAGG_DEFAULT(loads, U, block, VEC, grid) default: return go_secagg<loads, U, block, VEC, grid>(a, s);
#include "pgh_variants.def"
    }
}

hipError_t launch_synth_f32(float* out, const SlabMap& m, int64_t ncols, int n_rows, int64_t p, uint64_t seed,
                            uint64_t stream_id, int64_t row0, int64_t idx0, float scale, hipStream_t s,
                            int64_t max_wgs, int kind, bool nt) {
    if (!out || n_rows < 0 || n_rows > 65535 || ncols < p || (ncols & 3) || m.off != 0 || !valid_map(m, 0) ||
        (kind != 0 && kind != 1) ||
        (m.bshift == 62 && ncols > m.ld) || (reinterpret_cast<uintptr_t>(out) & 15))
        return hipErrorInvalidValue;
    if (n_rows == 0 || ncols == 0) return hipSuccess;
    int64_t gx = (ncols / 4 + BLOCK - 1) / BLOCK;
    if (gx > 1024) gx = 1024;
    int64_t gy = n_rows;
    if (max_wgs > 0) {  // bounded grid: rows strided, leaves CU slots to a fold running beside it
        if (gx > max_wgs) gx = max_wgs;
        gy = std::max<int64_t>(1, std::min<int64_t>(n_rows, max_wgs / gx));
    }
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (kind == 1 && nt)
        k_synth_f32<1, true><<<grid, BLOCK, 0, s>>>(out, m, ncols, n_rows, p, seed, stream_id, row0, idx0, scale);
    else if (kind == 1)
        k_synth_f32<1, false><<<grid, BLOCK, 0, s>>>(out, m, ncols, n_rows, p, seed, stream_id, row0, idx0, scale);
    else if (nt)
        k_synth_f32<0, true><<<grid, BLOCK, 0, s>>>(out, m, ncols, n_rows, p, seed, stream_id, row0, idx0, scale);
    else
        k_synth_f32<0, false><<<grid, BLOCK, 0, s>>>(out, m, ncols, n_rows, p, seed, stream_id, row0, idx0, scale);
    return hipGetLastError();
}

hipError_t launch_varint_decode(const uint8_t* bytes, const VChunk* chunks, int n_chunks, int64_t* row,
                                const SlabMap& m, int64_t lo, int64_t hi, hipStream_t s) {
    if (n_chunks < 0 || (n_chunks > 0 && (!bytes || !chunks || !row)) || (reinterpret_cast<uintptr_t>(bytes) & 15) ||
        m.off != 0 || !valid_map(m, 0) || lo > hi)
        return hipErrorInvalidValue;
    if (n_chunks == 0) return hipSuccess;
    k_varint_decode<<<(unsigned)n_chunks, 256, 0, s>>>(bytes, chunks, row, m, lo, hi);
    return hipGetLastError();
}

hipError_t launch_gather_f32(const uint8_t* bytes, const GChunk* chunks, int n_chunks, float* row, const SlabMap& m,
                             hipStream_t s) {
    // 16-byte row stores: the row and the map's column offset 4-aligned (blocks are multiples of 4)
    if (n_chunks < 0 || (n_chunks > 0 && (!bytes || !chunks || !row)) || (reinterpret_cast<uintptr_t>(bytes) & 3) ||
        (reinterpret_cast<uintptr_t>(row) & 15) || (m.off & 3) || (m.ld & 3) || (m.bstride & 3))
        return hipErrorInvalidValue;
    if (n_chunks == 0) return hipSuccess;
    k_gather_f32<<<(unsigned)n_chunks, BLOCK, 0, s>>>(bytes, chunks, row, m);
    return hipGetLastError();
}

hipError_t launch_secagg_decode(const int64_t* sum, float* dec, int64_t n, float divisor, hipStream_t s) {
    if (n < 0 || (n > 0 && (!sum || !dec))) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    int64_t g = (n + BLOCK - 1) / BLOCK;
    if (g > 8192) g = 8192;
    k_secagg_decode<<<(unsigned)g, BLOCK, 0, s>>>(sum, dec, n, divisor);
    return hipGetLastError();
}

hipError_t launch_server_opt(const ServerOptArgs& a, hipStream_t s) {
    static_assert(SERVER_OPT_WG_PARAMS == 4 * BLOCK, "one 16-byte column per lane");
    const bool adaptive = a.kind != 1;
    if (a.kind < 1 || a.kind > 4 || a.p <= 0 || !a.d || !a.ckpt || !a.out || !a.m || !a.m2 || (adaptive && (!a.v || !a.v2)))
        return hipErrorInvalidValue;
    for (const void* p : {(const void*)a.d, (const void*)a.ckpt, (const void*)a.out, (const void*)a.m, (const void*)a.v,
                          (const void*)a.m2, (const void*)a.v2})
        if (reinterpret_cast<uintptr_t>(p) & 15) return hipErrorInvalidValue;
    const int64_t ncol = (a.p + 3) >> 2;
    const unsigned g = (unsigned)std::min<int64_t>((ncol + BLOCK - 1) / BLOCK, SERVER_OPT_MAX_WGS);
    switch (a.kind) {
    case 1: k_server_opt<1><<<g, BLOCK, 0, s>>>(a); break;
    case 2: k_server_opt<2><<<g, BLOCK, 0, s>>>(a); break;
    case 3: k_server_opt<3><<<g, BLOCK, 0, s>>>(a); break;
    default: k_server_opt<4><<<g, BLOCK, 0, s>>>(a); break;
    }
    return hipGetLastError();
}

hipError_t launch_dp_noise(const DpNoiseArgs& a, hipStream_t s) {
    static_assert(DP_WG_PARAMS == 4 * BLOCK, "one 16-byte column per lane");
    if (a.p <= 0 || a.i0 < 0 || (a.i0 & 3) || !a.d || !a.out) return hipErrorInvalidValue;
    for (const void* p : {(const void*)a.d, (const void*)a.ckpt, (const void*)a.out})
        if (reinterpret_cast<uintptr_t>(p) & 15) return hipErrorInvalidValue;
    const int64_t ncol = (a.p + 3) >> 2;
    const unsigned g = (unsigned)std::min<int64_t>((ncol + BLOCK - 1) / BLOCK, DP_MAX_WGS);
    k_dp_noise<<<g, BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_dp_normals(uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out, hipStream_t s) {
    if (i0 < 0 || n < 0 || i0 > INT64_MAX - n || (n > 0 && !out)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const int64_t npairs = ((i0 + n - 1) >> 1) - (i0 >> 1) + 1;
    const unsigned g = (unsigned)std::min<int64_t>((npairs + BLOCK - 1) / BLOCK, DP_MAX_WGS);
    k_dp_normals<<<g, BLOCK, 0, s>>>(key, round, i0, n, out);
    return hipGetLastError();
}

static_assert(DISTSQ_RC % SUMSQ_RB == 0 && DISTSQ_RC <= BLOCK, "K12's row chunk: whole row groups, one lane per row at the end");

// K7 (negv null), K12 or K14 over the launch's rows, RC rows per workgroup, and the fold of the tile partials behind it.
template <int OP>
static hipError_t launch_row_sq(const SumsqArgs& a, const float* negv, const Rows& rows, hipStream_t s) {
    constexpr bool DIST = OP != ROW_SQ;  // a plane beside the rows
    constexpr int RC = DIST ? DISTSQ_RC : SUMSQ_RB;
    const RowTab* tab = rows.tab;
    if (!valid_rows(rows, a.n_rows, false, true) || a.p <= 0 || a.n_rows < 0 || a.map.off != 0 || !valid_map(a.map, a.p) ||
        a.ntiles != (a.p + SUMSQ_TILE - 1) / SUMSQ_TILE || a.ntiles > 0x7fffffff)
        return hipErrorInvalidValue;
    if (a.n_rows == 0) return hipSuccess;
    if (!a.slab || !a.part || !a.sumsq || (DIST && !negv) ||
        ((reinterpret_cast<uintptr_t>(a.slab) | reinterpret_cast<uintptr_t>(negv)) & 15))
        return hipErrorInvalidValue;
    const int max_rows = 65535 * RC;  // grid rows of one launch
    for (int done = 0; done < a.n_rows; done += max_rows) {
        SumsqArgs b = a;
        b.row0 = rows.row0 + done;
        b.n_rows = std::min(max_rows, a.n_rows - done);
        const dim3 grid((unsigned)b.ntiles, (unsigned)((b.n_rows + RC - 1) / RC));
        if (OP == ROW_DOT && tab) k_row_dot_rows<<<grid, BLOCK, 0, s>>>(DistsqArgs{b, negv}, *tab);
        else if (OP == ROW_DOT) k_row_dot<<<grid, BLOCK, 0, s>>>(DistsqArgs{b, negv});
        else if (DIST && tab) k_row_distsq_rows<<<grid, BLOCK, 0, s>>>(DistsqArgs{b, negv}, *tab);
        else if (DIST) k_row_distsq<<<grid, BLOCK, 0, s>>>(DistsqArgs{b, negv});
        else if (tab) k_row_sumsq_rows<<<grid, BLOCK, 0, s>>>(b, *tab);
        else k_row_sumsq<<<grid, BLOCK, 0, s>>>(b);
        if (tab) k_row_sumsq_fold_rows<<<(unsigned)b.n_rows, BLOCK, 0, s>>>(b, *tab);
        else k_row_sumsq_fold<<<(unsigned)b.n_rows, BLOCK, 0, s>>>(b);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_row_sumsq(const SumsqArgs& a, const Rows& rows, hipStream_t s) { return launch_row_sq<ROW_SQ>(a, nullptr, rows, s); }
hipError_t launch_row_distsq(const DistsqArgs& d, const Rows& rows, hipStream_t s) { return launch_row_sq<ROW_DIST>(d.s, d.negv, rows, s); }
hipError_t launch_row_dot(const DistsqArgs& d, const Rows& rows, hipStream_t s) { return launch_row_sq<ROW_DOT>(d.s, d.negv, rows, s); }

static_assert(PAIRDIST_RC % SUMSQ_RB == 0 && PAIRDIST_RA * PAIRDIST_RC == BLOCK, "K13: whole row groups, one lane per pair at the end");

hipError_t launch_row_pairdist(const PairdistArgs& a, hipStream_t s) {
    if (a.p <= 0 || a.n < 0 || a.n > PAIRDIST_MAX_ROWS || a.na < 0 || a.a0 < 0 || a.a0 + a.na > a.n || a.row0 < 0 ||
        (a.d_rows && a.row0) || a.map.off != 0 || !valid_map(a.map, a.p) || a.ntiles != (a.p + SUMSQ_TILE - 1) / SUMSQ_TILE)
        return hipErrorInvalidValue;
    if (a.na == 0 || a.n - a.a0 < 2) return hipSuccess;  // no pair with b > a
    if (!a.slab || !a.part || !a.dist || !aligned16(a.slab)) return hipErrorInvalidValue;
    PairdistArgs b = a;
    b.nchunks = (a.n - a.a0 - 1 + PAIRDIST_RC - 1) / PAIRDIST_RC;  // of the launch's first anchor block: the most
    const int64_t nabs = (a.na + PAIRDIST_RA - 1) / PAIRDIST_RA;
    const int64_t grid = a.ntiles * nabs * (int64_t)b.nchunks;
    if (a.ntiles > 0x7fffffff || grid > 0x7fffffff) return hipErrorInvalidValue;
    if (a.d_rows) k_row_pairdist_rows<<<(unsigned)grid, BLOCK, 0, s>>>(b);
    else k_row_pairdist<<<(unsigned)grid, BLOCK, 0, s>>>(b);
    k_row_pairdist_fold<<<dim3((unsigned)a.n, (unsigned)a.na), BLOCK, 0, s>>>(b);
    return hipGetLastError();
}

hipError_t launch_synth_shares(int64_t* out, const SlabMap& m, int64_t ncols, int n_clients, int n_parties,
                               int64_t p, uint64_t seed, int64_t client0, int64_t idx0, float enc_scale,
                               hipStream_t s) {
    if (!out || n_clients < 0 || n_clients > 65535 || n_parties < 1 || ncols < p || m.off != 0 || !valid_map(m, 0) ||
        (m.bshift == 62 && ncols > m.ld))
        return hipErrorInvalidValue;
    if (n_clients == 0 || ncols == 0) return hipSuccess;
    int64_t gx = (ncols + BLOCK - 1) / BLOCK;
    if (gx > 1024) gx = 1024;
    k_synth_shares<<<dim3((unsigned)gx, (unsigned)n_clients), BLOCK, 0, s>>>(out, m, ncols, n_parties, p, seed,
                                                                            client0, idx0, enc_scale);
    return hipGetLastError();
}

}  // namespace pgh
