// Internal launcher interface between the C-ABI context code (pgh_api.cpp, pgh_ingest.cpp,
// pgh_reduce.cpp, pgh_slots.cpp) and the gfx950 kernels (pgh_kernels.hip).
// Not installed; the public surface is include/pgh_api.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pgh {

// fedavg modes (same numbering as PGH_MEAN / PGH_ITERATIVE_MEAN / PGH_WEIGHTED_MEAN)
// (3, PGH_CLIPPED_MEAN, reaches the kernels as MODE_WEIGHTED over the scales)
enum { MODE_MEAN = 0, MODE_ITERATIVE = 1, MODE_WEIGHTED = 2, MODE_TRIMMED = 4, MODE_MEDIAN = 5 };
constexpr int TRIM_MAX = 8;
// flags for a chunked (client-streaming) reduction
enum { FL_FIRST = 1, FL_FINAL = 2 };

// Column-blocked slab: the shard's params are cut into blocks of `ld`
// columns; block j holds every row's columns [j*ld, (j+1)*ld) row after row, so element
// (row r, shard param i) lives at  (i >> bshift) * bstride + r * ld + (i & bmask).
// A lane walking down the rows of one column then streams through one compact block (rows ld
// apart) instead of rows a whole shard apart.  One block (bshift = 62) is the plain row-major
// [rows][ld] layout, used for shards of at most one block and for the [p] vectors.
struct SlabMap {
    int64_t ld;        // columns per block = row stride inside a block (multiple of 4; slab: of 64)
    int64_t bstride;   // elements from block j to block j + 1 (= rows in the slab x ld)
    int bshift;        // log2(ld) when blocked, 62 for a single block
    int64_t bmask;     // ld - 1 when blocked, 2^62 - 1 for a single block
    int64_t off;       // shard param of the launch's local column 0 (range folds)
    __host__ __device__ int64_t at(int64_t local) const {
        const int64_t i = off + local;
        return (i >> bshift) * bstride + (i & bmask);
    }
};

inline SlabMap single_block(int64_t ld) { return SlabMap{ld, 0, 62, (int64_t(1) << 62) - 1, 0}; }

struct FedavgArgs {
    const float* diffs;     // slab at the first row: clients client0 .. client0+n_rows-1
    SlabMap map;            // slab geometry; map.off = shard param of local column 0
    int n_rows;
    int64_t client0;        // global index of row 0 (iterative k, weight index)
    int64_t p;              // params in this shard
    const float* weights;   // [n_rows] device, MODE_WEIGHTED only
    const double* recips;   // [n_rows] device, MODE_ITERATIVE: 1 / (double)(float)(client0 + r + 1)
    float* acc;             // [p] running state; read unless FL_FIRST, written unless FL_FINAL
    const float* ckpt;      // [p], FL_FINAL only
    float* out;             // [p], FL_FINAL only
    float divisor;          // float(N) or sum of weights, FL_FINAL of MEAN / WEIGHTED
    int flags;
    int mode;
    int variant;            // kernel variant (table in pgh_variants.def); < 0 = auto by shard size
    // MODE_TRIMMED (K8, the streaming definition in include/pgh_api.h): b = trim_b values dropped per
    // side; divisor = float(N - 2b); client0 + r is the fold index k of row r.  The selection state
    // of a param lives in registers for the launch; a launch without FL_FIRST reads it and a launch
    // without FL_FINAL writes it: lo[j] in plane j and hi[j] in plane b + j of tstate (int32 keys,
    // planes tplane elements apart, each indexed like acc), the running sum in acc.
    int trim_b;             // 1 .. TRIM_MAX
    int trim_vec;           // 4: 16-byte columns, 1: one param per lane, 0: auto_trim_vec
    int32_t* tstate;        // [2 b][tplane] at this launch's column 0; unused when FL_FIRST | FL_FINAL
    int64_t tplane;
};
// The column width K8 takes for a shard of p params at b (variant ids 40: 16-byte, 41: one param).
int auto_trim_vec(int64_t p, int b);

// The fold's and the share sum's variant ids: 0 .. N_VARIANTS - 1, one PGH_FOLD row each, in order.
constexpr int N_VARIANTS = 0
#define PGH_FOLD(...) +1
#include "pgh_variants.def"
    ;
constexpr bool variant_ids_in_order() {
    int next = 0;
    bool ok = true;
#define PGH_FOLD(id, ...) ok = ok && id == next++;
#define PGH_SECAGG(id, ...) ok = ok && id >= 0 && id < next;
#include "pgh_variants.def"
    return ok && next == N_VARIANTS;
}
static_assert(variant_ids_in_order(), "pgh_variants.def: fold ids 0, 1, 2, ... each once; share-sum ids among them");

// Slab rows given by index instead of contiguous: row r of the launch is slab row rows[r] (the
// launch's slab pointer = the slab at row 0).  Report-time aggregation folds the reported diffs where
// they landed, in assignment order, skipping workers that never reported
// (cycle_manager.py:243-245).  Passed by value as a kernel argument (scalar loads from the
// kernarg segment), so a launch covers at most ROWTAB_MAX rows.
constexpr int ROWTAB_MAX = 512;
struct RowTab {
    int32_t rows[ROWTAB_MAX];
};
// Which slab rows a launch of n_rows rows reads: tab->rows[r], else d_rows[r] (a device table of
// n_rows entries), else row0 + r.  At most one table is set, and row0 is 0 beside one.  The fold and
// K7 have no kernel for a device table.  The fold and the median take their contiguous rows from
// the slab pointer they are given (row0 = 0); K7, whose outputs are indexed by slab row, from row0.
struct Rows {
    const RowTab* tab = nullptr;
    const int32_t* d_rows = nullptr;
    int row0 = 0;
};
// (a row table runs the shapes pgh_variants.def marks rowtab, launch_fedavg in pgh_kernels.hip)
hipError_t launch_fedavg(const FedavgArgs& a, const Rows& rows, hipStream_t s);

// MODE_MEDIAN (the definition is in include/pgh_api.h): out = ckpt - median over the launch's rows,
// per param.  Values are compared as u = key(x) ^ 0x80000000 (unsigned order = the key's signed
// order); the element of rank (n - 1) / 2 is found by bisection on u, most significant bit first:
// T = prefix | 1 << bit; prefix = T when #{u < T} <= rank.  An even n also needs the next element:
// with c = #{u <= lower} it is lower when c >= n / 2 + 1 and min{u > lower} otherwise.
// K9 launch_median: one pass over HBM.  The rows of a tile of 64 columns come on chip as keys in
// registers, one column per lane: up to 64 rows in one lane (8 / 16 / 32 / 64 keys), more rows split
// over the 2 / 4 / 8 / MEDIAN_WAVES waves of a workgroup (64 keys per lane, wave w holding rows w,
// w + W, ...), whose per-bit counts meet in LDS.  n_rows <= MEDIAN_NCHIP.
// K9p launch_median_pass: any n_rows.  One launch per bit (31 .. 0) and one more (bit = -1) for the
// upper middle of an even n; one lane walks down its column and counts.  The prefix of a param
// lives in `prefix` ([p] words at the launch's column 0) between the launches: bit 31 starts it,
// the last launch (bit 0 for an odd n, -1 for an even one) writes out instead.
constexpr int MEDIAN_WAVES = 16;
constexpr int MEDIAN_NCHIP = 64 * MEDIAN_WAVES;
struct MedianArgs {
    const float* diffs;      // the slab at row 0 (a table) or at the first row
    SlabMap map;             // map.off = shard param of local column 0
    int n_rows;
    int64_t p;               // params of the launch
    const int32_t* d_rows;   // the launcher's: Rows::d_rows on its way to the kernel
    const float* ckpt;       // [p]
    float* out;              // [p]
    uint32_t* prefix;        // [p], K9p only
};
hipError_t launch_median(const MedianArgs& a, const Rows& rows, hipStream_t s);
hipError_t launch_median_pass(const MedianArgs& a, const Rows& rows, int bit, hipStream_t s);

struct SecaggArgs {
    const int64_t* shares;  // slab at the first row (rows = clients x parties)
    SlabMap map;
    int n_rows;
    int64_t p;
    uint64_t* acc;          // [p] running wrap-sum; read unless FL_FIRST, written unless FL_FINAL
    int64_t* sum_out;       // [p] nullable, FL_FINAL only
    float* dec_out;         // [p] nullable, FL_FINAL only
    float divisor;          // float(base ** prec)
    int flags;
    int variant;
};
constexpr int SECAGG_AUTO_VARIANT = 14;  // what variant < 0 runs (measured in launch_secagg)
hipError_t launch_secagg(const SecaggArgs& a, hipStream_t s);
// The fp32 fold variant the auto choice (variant < 0) picks for a shard of p params.
int auto_variant(int64_t p, int mode);

// Deterministic synthetic inputs (restated bit for bit by oracle/oracle.py).  `out` is the
// slab (or a [p] vector: single_block) at its first row; params [p, ncols) are zero-filled.
hipError_t launch_synth_f32(float* out, const SlabMap& m, int64_t ncols, int n_rows, int64_t p, uint64_t seed,
                            uint64_t stream_id, int64_t row0, int64_t idx0, float scale, hipStream_t s,
                            int64_t max_wgs = 0,  // > 0: cap the grid at max_wgs workgroups
                            int kind = 0,         // 0 Irwin-Hall per param, 1 fast (4 params per word)
                            bool nt = false);     // non-temporal stores
// dec[i] = float32(int64 sum[i]) / divisor for i < n (decode after a cross-rank share-sum reduction).
hipError_t launch_secagg_decode(const int64_t* sum, float* dec, int64_t n, float divisor, hipStream_t s);
hipError_t launch_synth_shares(int64_t* out, const SlabMap& m, int64_t ncols, int n_clients, int n_parties,
                               int64_t p, uint64_t seed, int64_t client0, int64_t idx0, float enc_scale,
                               hipStream_t s);

// Packed-varint int64 payloads (secagg shares as State bytes) decoded on the GPU.  The payload
// bytes sit in HBM as received, each tensor's payload starting 16-byte aligned; they are cut into
// chunks of at most VARINT_CHUNK bytes.  `first` = index (in the flat layout) of the first value
// whose LAST byte lies in the chunk: the host counts terminator bytes per chunk while staging.
constexpr int VARINT_CHUNK = 16384;  // one wave of K4 per chunk
struct VChunk {
    int64_t off;       // chunk start, bytes from the payload buffer base (16-aligned)
    int64_t span_off;  // start of the tensor payload holding the chunk (nothing before it is read)
    int64_t first;     // flat index of the first value ending in the chunk
    int32_t n;         // bytes in the chunk
    int32_t pad;
};
// Decode every chunk into one slab row: value with flat index i goes to row[m.at(i - lo)] when
// lo <= i < hi.  Requires validated input (no varint longer than 10 bytes).
hipError_t launch_varint_decode(const uint8_t* bytes, const VChunk* chunks, int n_chunks, int64_t* row,
                                const SlabMap& m, int64_t lo, int64_t hi, hipStream_t s);

// Float payloads of a page-locked State message, DMA'd into HBM as they lie in the message (no host
// staging copy), gathered into one slab row: chunk k moves n floats starting at byte `src` of the
// buffer (any alignment: protobuf puts a payload right after its varint length) to shard elements
// dst .. dst + n - 1 of the row (row[m.at(i)]).  The buffer holds 8 readable bytes past the last
// payload byte.
constexpr int GATHER_CHUNK = 4096;
struct GChunk {
    int64_t src;
    int64_t dst;
    int32_t n;
    int32_t pad;
};
hipError_t launch_gather_f32(const uint8_t* bytes, const GChunk* chunks, int n_chunks, float* row, const SlabMap& m,
                             hipStream_t s);

// K7: per-row sum of squares in f64, in the fixed order of DESIGN.md "Clipped FedAvg": tiles of
// SUMSQ_TILE params, 256 lane partials per tile (lane l adds the squares of its four 16-byte columns
// 4(l + 256j) .. + 3, j = 0 .. 3, in index order), a shuffle tree per wave, ((w0 + w1) + w2) + w3,
// then a left fold of the row's tile partials.  Params at or past p count as +0.0.  The launch
// covers the n_rows slab rows of its Rows (contiguous from row0, or a RowTab), writes
// part[row * ntiles + t] and then sumsq[row] (row = slab row).
constexpr int SUMSQ_TILE = 4096;
struct SumsqArgs {
    const float* slab;   // the slab at row 0
    SlabMap map;         // map.off = 0
    int64_t p;           // params in the shard
    int64_t ntiles;      // ceil(p / SUMSQ_TILE)
    int row0;            // the launcher's: Rows::row0 on its way to the kernel
    int n_rows;
    double* part;        // [slab rows][ntiles]
    double* sumsq;       // [slab rows]
};
hipError_t launch_row_sumsq(const SumsqArgs& a, const Rows& rows, hipStream_t s);

// K12: the geometric median's squared distances (the definition is in include/pgh_api.h): K7's sum, in
// K7's order, over x = d_c[i] + negv[i], one f32 addition per param (negv = -v: d + (-v) is d - v in
// IEEE).  A workgroup owns one tile and DISTSQ_RC rows: the plane tile is read once per DISTSQ_RC rows,
// not once per K7 row group (the tile body is K7's, pgh_kernels.hip row_sq_tile, and so is the launcher).  The launch writes s.part[row * ntiles + t] and then s.sumsq[row] like K7
// (s.sumsq is the distances' buffer here); negv holds at least p floats rounded up to 4, 16-byte aligned.
constexpr int DISTSQ_RC = 32;
struct DistsqArgs {
    SumsqArgs s;
    const float* negv;   // [p], -v
};
hipError_t launch_row_distsq(const DistsqArgs& a, const Rows& rows, hipStream_t s);

// K14: every row's inner product with a fixed vector (the trust root of PGH_TRUSTED_MEAN; the definition is in
// include/pgh_api.h): K7's sum, in K7's order, over (double)d_c[i] * (double)g0[i] -- exact products, one rounded
// f64 addition each.  K12's shape, tile body and launcher: `negv` holds g0 itself here (at least p floats rounded
// up to 4, 16-byte aligned), params at or past p contribute +0.0 whatever either operand holds there, and the
// launch writes s.part[row * ntiles + t] and then s.sumsq[row] (the dots' buffer).  A sum may be negative.
hipError_t launch_row_dot(const DistsqArgs& a, const Rows& rows, hipStream_t s);

// K13: Multi-Krum's pairwise squared distances (the definition is in include/pgh_api.h): for list indices
// a < b of the n listed rows, K12's sum of row a against the point row b -- K7's sum, in K7's order, over
// x = d_a[i] - d_b[i], one f32 subtraction per param.  List index k is slab row d_rows[k] (a device table of n
// entries) or, without a table, row0 + k.  A workgroup owns one tile, PAIRDIST_RA anchors (their tile in
// registers: 16 floats per lane and anchor) and PAIRDIST_RC of the rows after the block's first anchor, so the
// slab is read n / PAIRDIST_RA times at most, not n times.  One launch takes the anchors [a0, a0 + na) against
// every later row, writes part[((a - a0) * n + b) * ntiles + t] and then dist[a * n + b], b > a only: the
// caller sizes `part` for na anchors and batches them; the lower triangle and the diagonal of `dist` are not
// written.
constexpr int PAIRDIST_RA = 8;
constexpr int PAIRDIST_RC = 32;
constexpr int PAIRDIST_MAX_ROWS = 1024;
struct PairdistArgs {
    const float* slab;       // the slab at row 0
    SlabMap map;             // map.off = 0
    int64_t p;               // params in the shard
    int64_t ntiles;          // ceil(p / SUMSQ_TILE)
    const int32_t* d_rows;   // [n] slab rows in list order, or null: row0 + k
    int row0;
    int n;                   // rows in the list
    int a0, na;              // the launch's anchors
    int nchunks;             // the launcher's: row chunks per anchor block in the grid
    double* part;            // [na][n][ntiles]
    double* dist;            // [n][n]
};
hipError_t launch_row_pairdist(const PairdistArgs& a, hipStream_t s);

// K10: the server optimizer's step behind a FINAL fold (the definition is in include/pgh_api.h).  The
// fold ran with ckpt = a plane of -0.0f and out = d, so d = (-0.0f) - g, which is -g bit for bit for
// every non-NaN g: x - y = x + (-y) in IEEE 754, so d = (-0) + (-g); a finite non-zero or infinite
// -g added to a zero is itself, (-0) + (-0) = -0 = -(+0), and (-0) + (+0) = +0 = -(-0) when rounding
// to nearest.  K10 takes g back by flipping d's sign bit (a NaN stays a NaN).  Elementwise over the
// launch's p params: a lane owns one 16-byte column per grid step and issues the loads of d
// (non-temporal: nobody reads it again), ckpt, m and v before any arithmetic; the last column of a
// ragged p goes scalar.  It reads the committed m / v and writes out and the pending m2 / v2, never
// in place.  KIND 1 (FedAvgM) touches neither v nor v2.  Workgroups of SERVER_OPT_WG_PARAMS params,
// at most SERVER_OPT_MAX_WGS of them (grid-stride beyond).
constexpr int SERVER_OPT_WG_PARAMS = 1024;
constexpr int SERVER_OPT_MAX_WGS = 2048;
struct ServerOptArgs {
    const float* d;      // every pointer at the launch's column 0, 16-byte aligned
    const float* ckpt;
    float* out;
    const float* m;
    const float* v;      // kinds 2 .. 4
    float* m2;
    float* v2;           // kinds 2 .. 4
    int64_t p;           // params of the launch
    int kind;            // 1 momentum, 2 adagrad, 3 adam, 4 yogi (pgh_server_opt)
    float lr, beta1, beta2, c1, c2, tau;
};
hipError_t launch_server_opt(const ServerOptArgs& a, hipStream_t s);

// K11: Gaussian noise on the clipped close (the definition is in include/pgh_api.h).  Like K10 it runs
// behind a FINAL fold that wrote d = -g into a delta plane: g comes back by a sign flip, the param with
// model index i takes n_i = (float)(sigma * Z_i), g' = g + n_i, and the launch writes out = ckpt - g', or
// -- ahead of K10, ckpt == NULL -- the delta plane -(g') (out may be d itself: a lane reads its column
// before it writes it).  Z comes from Philox4x32-10 with the counter (pair, round, attempt) and Marsaglia's
// polar method, at most DP_ATTEMPTS attempts per pair; pair = i >> 1, so with i0 a multiple of 4 the
// lane of a 16-byte column owns two whole pairs.  The last column of a ragged p goes scalar.  Integer-
// and f64-ALU bound (12 bytes of HBM per param); no LDS, no atomics.  Workgroups of DP_WG_PARAMS
// params, at most DP_MAX_WGS of them (grid-stride beyond).
constexpr int DP_ATTEMPTS = 32;
constexpr int DP_WG_PARAMS = 1024;
constexpr int DP_MAX_WGS = 8192;
struct DpNoiseArgs {
    const float* d;      // every pointer at the launch's column 0, 16-byte aligned
    const float* ckpt;   // NULL: write the delta plane
    float* out;
    int64_t p;           // params of the launch
    int64_t i0;          // model index of column 0, a multiple of 4
    uint64_t key;
    uint32_t round;
    double sigma;
};
hipError_t launch_dp_noise(const DpNoiseArgs& a, hipStream_t s);
// The sampler alone: out[k] = Z_(i0 + k) for k < n (f64, device memory), any i0 >= 0.
hipError_t launch_dp_normals(uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out, hipStream_t s);

constexpr uint64_t STREAM_DIFF = 0, STREAM_CKPT = 1, STREAM_SECRET = 2, STREAM_SHARE = 3;
constexpr float DIFF_SCALE = 2.6429e-7f;
constexpr float CKPT_SCALE = 1.32145e-6f;

}  // namespace pgh
