// gfx950 (CDNA4, MI355X) kernel K20 of the cycle-close aggregation path.
//
// K20 k_row_gram_bf16  the Gram matrix G = X X^T of the listed slab rows from split-bf16 products on the matrix
//       cores (the "gram_bf16" distances; the definition is in include/pgh_api.h, the design in DESIGN.md section 5).
//       K16's k_row_gram_fold finishes each entry over the chunks, scales it back and mirrors the triangle.
//
// A translation unit of its own, beside pgh_gram.hip.  A row is scaled by a power of two so that its norm lies in
// [1, 2), every scaled f32 value x is split exactly into three bf16 values h + m + l, and a product x_a x_b is
// taken as the six bf16 x bf16 terms hh, hm, mh, mm, hl, lh, each exact in f32, by v_mfma_f32_32x32x16_bf16.
//
// Work split.  K16's: blocks of GRAM_RB = 128 list positions, the block pairs (A, B) with B >= A, chunks of whole
// 4,096-param tiles; a workgroup of 256 lanes owns one (chunk, block pair) and the block pair runs fastest in the
// grid, so the workgroups that read one chunk's rows are neighbours in dispatch order.
// Data path.  Per step of GRAM_BF16_KSTEP = 32 params the workgroup brings 128 A rows' and 128 B rows' segments
// (a diagonal pair: A alone) from global memory: lane l loads the 16-byte column l & 7 of rows (l >> 3) + 32 q,
// q = 0 .. 3.  Params past p are masked to +0.0 (the address clamps to the row's last column as in K7).  The
// lane then scales and splits its values ONCE, in registers, and stores 8 bytes (four bf16) to each of the three
// planes h, m, l of the operand in LDS; the MFMA operands are plain 16-byte LDS reads of a plane.  The row stride
// of a plane is 40 bf16 = 80 bytes, off the bank period: the 16 rows that a quarter wave reads at one k fall
// into 16 distinct 16-byte slots of the 256-byte period.  Two LDS buffers of 2 operands x 3 planes (120 KiB of the
// 160): the next step's global loads are issued before this step's MFMAs and split and stored behind them, one
// barrier per step.
// Compute.  Wave w owns the 64 x 64 sub-block (w >> 1, w & 1) as 2 x 2 MFMA tiles of 32 x 32: 64 f32
// accumulators per lane, and 64 f64 ones that take them over every GRAM_BF16_RUN params.  Lane (r = l & 31,
// kh = l >> 5) reads the eight bf16 k = 8 kh .. 8 kh + 7 of row r of each tile's planes per 16-param slice; per
// slice and tile the six terms go lh, hl, mm, mh, hm, hh, the small ones first.
// A wave whose sub-block lies past n, or below the diagonal of a diagonal pair, computes nothing; tiles past n
// and tiles below the diagonal are not stored.
// Result layout of the MFMA: register v of lane l holds entry (8 (v >> 2) + 4 (l >> 5) + (v & 3), l & 31).
#include "pgh_gram_bf16.h"

namespace pgh {
namespace {

constexpr int BLOCK = 256;
constexpr int KSTEP = GRAM_BF16_KSTEP;
constexpr int LDB = KSTEP + 8;  // LDS row stride of a plane in bf16: 80 bytes, a multiple of 16 and not of 128
constexpr int GRAM_BLK = GRAM_RB * GRAM_RB;
constexpr int RUN_STEPS = GRAM_BF16_RUN / KSTEP;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

static_assert(GRAM_RB == 128 && KSTEP == 32 && BLOCK == 256, "K20: 4 waves of 64 x 64, 8 lanes a row, 4 rows a lane");
static_assert(sizeof(uint16_t) * 2 * 2 * 3 * GRAM_RB * LDB <= 160 * 1024, "K20: two buffers of six planes within gfx950's LDS");

// four f32 -> four bf16 (round to nearest even), packed; and back, exactly
__device__ __forceinline__ uint2 to_bf16(f32x4 v) { return __builtin_bit_cast(uint2, __builtin_convertvector(v, bf16x4)); }
__device__ __forceinline__ f32x4 from_bf16(uint2 p) {
    return f32x4{__uint_as_float(p.x << 16), __uint_as_float(p.x & 0xffff0000u), __uint_as_float(p.y << 16), __uint_as_float(p.y & 0xffff0000u)};
}

struct Split {
    uint2 h, m, l;
};

// x = d 2^-e per element, then h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), both subtractions in f32 and
// exact.  A finite x whose rounding would be an infinity (past the largest bf16: only a row whose sum is not
// finite is left unscaled and can hold one) takes the largest finite bf16 of its sign as h.
__device__ __forceinline__ Split split3(f32x4 d, int neg_e) {
    constexpr float BF16_MAX = 0x1.fep127f;
    f32x4 x, hx;
#pragma unroll
    for (int e = 0; e < 4; ++e) hx[e] = x[e] = __builtin_ldexpf(d[e], neg_e);
    if (fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3]))) > BF16_MAX) {  // (rare; a NaN is not above)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (fabsf(x[e]) > BF16_MAX && fabsf(x[e]) < __builtin_inff()) hx[e] = copysignf(BF16_MAX, x[e]);
    }
    Split s;
    s.h = to_bf16(hx);
    const f32x4 r1 = x - from_bf16(s.h);
    s.m = to_bf16(r1);
    s.l = to_bf16(r1 - from_bf16(s.m));
    return s;
}

template <int SRC>
__global__ __launch_bounds__(BLOCK) void k_row_gram_bf16(GramArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t sm[2][2][3][GRAM_RB][LDB];  // [buffer][A, B][h, m, l][row][k]
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
    int negA[4], negB[4];  // -e of the lane's rows
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const size_t ra = gram_row_at<SRC>(a, A * GRAM_RB + min(lr + 32 * q, na - 1)), rb = gram_row_at<SRC>(a, B * GRAM_RB + min(lr + 32 * q, nb - 1));
        rowA[q] = a.slab + ra * (size_t)a.map.ld;
        rowB[q] = a.slab + rb * (size_t)a.map.ld;
        negA[q] = -gram_row_exp(a.sums[ra]);
        negB[q] = -gram_row_exp(a.sums[rb]);
    }
    const int64_t kbeg = (int64_t)chunk * a.chunk_tiles * SUMSQ_TILE;
    const int64_t kend = min(a.p, kbeg + a.chunk_tiles * SUMSQ_TILE);
    const int ns = (int)((kend - kbeg + KSTEP - 1) / KSTEP);  // >= 1: kbeg < p
    const int64_t last4 = (a.p - 1) & ~int64_t(3);
    f32x4 ga[4], gb[4];
    auto fetch = [&](int s) {
        const int64_t idx = kbeg + (int64_t)s * KSTEP + lc;
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
    auto stash_one = [&](int buf, int op, int q, f32x4 g, int neg_e) {
        const Split sp = split3(g, neg_e);
        *reinterpret_cast<uint2*>(&sm[buf][op][0][lr + 32 * q][lc]) = sp.h;
        *reinterpret_cast<uint2*>(&sm[buf][op][1][lr + 32 * q][lc]) = sp.m;
        *reinterpret_cast<uint2*>(&sm[buf][op][2][lr + 32 * q][lc]) = sp.l;
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) stash_one(buf, 0, q, ga[q], negA[q]);
        if (!diag) {
#pragma unroll
            for (int q = 0; q < 4; ++q) stash_one(buf, 1, q, gb[q], negB[q]);
        }
    };

    // ---- the wave's 2 x 2 MFMA tiles and which of them it stores ----
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, kh = (lane & 63) >> 5;
    unsigned live = 0;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int r0 = wr * 64 + ti * 32, c0 = wc * 64 + tj * 32;
            if (r0 < na && c0 < nb && (!diag || c0 >= r0)) live |= 1u << (ti * 2 + tj);
        }
    live = (unsigned)__builtin_amdgcn_readfirstlane((int)live);
    f32x16 acc[2][2];
    double acc64[2][2][16];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                acc[ti][tj][v] = 0.f;
                acc64[ti][tj][v] = 0.0;
            }

    auto compute = [&](int buf) {
        const int opb = diag ? 0 : 1;
#pragma unroll
        for (int ks = 0; ks < KSTEP / 16; ++ks) {
            bf16x8 af[2][3], bf[2][3];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    af[t][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(&sm[buf][0][pl][wr * 64 + t * 32 + li][ks * 16 + kh * 8]));
                    bf[t][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(&sm[buf][opb][pl][wc * 64 + t * 32 + li][ks * 16 + kh * 8]));
                }
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    f32x16 c = acc[ti][tj];
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti][2], bf[tj][0], c, 0, 0, 0);  // l h
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti][0], bf[tj][2], c, 0, 0, 0);  // h l
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti][1], bf[tj][1], c, 0, 0, 0);  // m m
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti][1], bf[tj][0], c, 0, 0, 0);  // m h
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti][0], bf[tj][1], c, 0, 0, 0);  // h m
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti][0], bf[tj][0], c, 0, 0, 0);  // h h
                    acc[ti][tj] = c;
                }
        }
    };
    auto flush = [&]() {  // a run ends: its f32 sums join the f64 ones
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    acc64[ti][tj][v] += (double)acc[ti][tj][v];
                    acc[ti][tj][v] = 0.f;
                }
    };

    // ---- the steps: buffer s & 1 holds step s; step s + 1 is loaded ahead of the MFMAs, split and stored behind them ----
    fetch(0);
    stash(0);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
        const bool more = s + 1 < ns;  // (uniform)
        if (more) fetch(s + 1);
        if (live) {  // (a wave with any tile to store computes all four: no branch between the MFMAs)
            compute(s & 1);
            if (s % RUN_STEPS == RUN_STEPS - 1 || !more) flush();
        }
        if (more) stash((s + 1) & 1);
        __syncthreads();
    }

    // ---- the partial block: register v of lane (li, kh) is entry (8 (v >> 2) + 4 kh + (v & 3), li) of its tile ----
    double* part = a.part + ((size_t)chunk * (size_t)a.nbp + (size_t)bpl) * GRAM_BLK;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            if (!((live >> (ti * 2 + tj)) & 1u)) continue;
            const int j = wc * 64 + tj * 32 + li;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = wr * 64 + ti * 32 + 8 * (v >> 2) + 4 * kh + (v & 3);
                if (i < na && j < nb) part[i * GRAM_RB + j] = acc64[ti][tj][v];
            }
        }
}

}  // namespace

hipError_t launch_row_gram_bf16(const GramArgs& a, hipStream_t s) {
    if (check_row_gram(a) != hipSuccess || !a.sums) return hipErrorInvalidValue;
    const int64_t grid = (int64_t)a.nchunks * a.nbp;
    if (a.d_rows) k_row_gram_bf16<2><<<(unsigned)grid, BLOCK, 0, s>>>(a);
    else k_row_gram_bf16<0><<<(unsigned)grid, BLOCK, 0, s>>>(a);
    return launch_row_gram_fold(a, s);
}

}  // namespace pgh
