// What each averaging rule and the server optimizer keep in a single-GPU context: one struct per feature,
// members of struct pgh_ctx (pgh_ctx.h) as clip, noise, geo, trim, med and opt.  Their owners release with the context.
// The code that works on them: pgh_rules.cpp (clip, geo, trim, med and the lifecycle calls rules_*),
// pgh_serveropt.cpp (opt).  Not installed.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "pgh_res.h"

namespace pgh_detail {

// Clipped FedAvg (pgh_set_clip_norm, PGH_CLIPPED_MEAN).  K7 (k_row_sumsq)
// runs on the copy stream -- behind the row's ingest, ahead of any later overwrite of the slot --
// and its sum comes back through h_sq in a small D2H on the same stream, followed by sq_ev.
// sq_state: NONE (no sum of the slot's present diff), QUEUED (K7 + D2H issued, value lands in
// h_sq before the latest sq_ev), VALID (sq_host holds it).  Any ingest into a slot resets it.
struct ClipState {
    enum : uint8_t { SQ_NONE = 0, SQ_QUEUED = 1, SQ_VALID = 2 };
    float c = 0.f;                    // the L2 bound; 0 = clipping off
    std::vector<uint8_t> sq_state;    // per slot
    std::vector<double> sq_host;      // per slot: the cached sum of squares
    std::vector<int32_t> sq_queued;   // slots that went QUEUED since the last harvest
    DeviceBuf d_sq_part;              // double [slots][ceil(pg / SUMSQ_TILE)] tile partials
    DeviceBuf d_sq;                   // double [slots]
    PinnedBuf h_sq;                   // double [slots]
    Event sq_ev;
    // the scales live in the context's `weights` (fold order) and go to the device like weights.  Resident
    // folds: scales_valid says weights[0, n) are the scales of the slab as it is (range folds reuse them).
    bool scales_valid = false;
    std::vector<double> norms;        // slot folds of the running cycle, in fold order (beside weights)
    int64_t rows = 0, clipped = 0;    // folds finished since pgh_reset / pgh_reserve
    double max_norm = 0.0;

    // The diffs in slots [slot, slot + n) are being replaced: their cached sums were the old diffs', and the
    // slab is no longer the one the resident scales were computed for.  The one place a sum goes to NONE
    // slot by slot.
    void slot_written(int slot, int n = 1) {
        std::fill_n(sq_state.begin() + slot, n, (uint8_t)SQ_NONE);
        scales_valid = false;
    }
    void forget();  // every slot back to SQ_NONE, the scales, the running cycle and the totals (pgh_reset)
    void count(const float* scales, const double* row_norms, int64_t n);  // rows into the finished totals
    // the slot folds of the running cycle into the finished totals: scales[k] beside norms[k]
    void count_cycle(const std::vector<float>& scales) {
        count(scales.data(), norms.data(), (int64_t)std::min(norms.size(), scales.size()));
    }
};

// Gaussian noise on the clipped close (pgh_set_dp_noise): a modifier of the clip
// rule, not a rule of its own.  With z > 0 fold_launch runs every fp32 FINAL -- PGH_CLIPPED_MEAN only,
// any other mode is refused -- against a -0 plane into a delta plane and K11 behind it: the server
// optimizer's planes when one is set (K10 follows K11), else the two owned here, allocated by the first
// noised FINAL.  The setting belongs to the model like the optimizer's: pgh_reset / pgh_reserve keep it,
// a new layout or shard clears it (rules_shard_set).
struct NoiseState {
    float z = 0.f;        // the noise multiplier; 0 = off
    uint64_t key = 0;
    uint32_t round = 0;
    DeviceBuf d_nz, d_d;  // float [pvec]: -0.0f everywhere; d = -g of the last noised FINAL without an optimizer
    int64_t pvec = 0;     // the planes' length
    double sigma_last = 0.0;  // what the last noised FINAL used: z * C / N, and N
    int64_t n_last = 0;

    void release() {  // planes and setting; the caller has waited for the context's work
        d_nz.reset();
        d_d.reset();
        z = 0.f;
        pvec = 0;
    }
};

// Geometric-median FedAvg (pgh_set_geomed, PGH_GEOMETRIC_MEDIAN): the smoothed
// Weiszfeld iteration.  With the rule on every ingest queues K7 like clipping (the cached sums are iteration
// 0's squared distances and say which rows are excluded).  A close computes the final weights on the
// context's stream -- per inner iteration a weighted fold against the -0 plane into d_negv (= -v), K12
// against it, a D2H of the distances, the host step -- and leaves them in the context's `weights` (fold
// order of the included rows) for the one FINAL fold, which is the weighted fold over `rows`.  Both planes
// are float [pvec], allocated by the first close that iterates (iters >= 2) or by pgh_row_distsq.
struct GeomedState {
    int iters = 0;                  // 0 = the rule is off
    float nu = 0.f;
    std::vector<int32_t> rows;      // the included slots, in fold order
    float W = 0.f;                  // the f32 left fold of the final weights
    // Resident folds: weights[0, rows.size()) are the final weights of the slab as it is, computed for
    // clients [0, n_valid) -- range folds and repeated closes reuse them.
    bool weights_valid = false;
    int64_t n_valid = 0;
    DeviceBuf d_nz, d_negv;         // -0.0f everywhere; -v of the last inner iteration (or -point)
    DeviceBuf d_dist;               // double [slots]: K12's sums, by slab row
    PinnedBuf h_dist;               // double [slots]
    // what the last computation of the weights saw (pgh_geomed_stats)
    int64_t n_rows = 0, n_excluded = 0;
    double objective = 0.0;
    float max_weight = 0.f;

    void forget() {  // the weights and the tallies (pgh_reset); the setting stays
        weights_valid = false;
        rows.clear();
        n_rows = n_excluded = 0;
        objective = 0.0;
        max_weight = 0.f;
    }
    void release() {  // planes and setting; the caller has waited for the context's work
        d_nz.reset();
        d_negv.reset();
        iters = 0;
        nu = 0.f;
        forget();
    }
};

// Trimmed-mean FedAvg (pgh_set_trim, PGH_TRIMMED_MEAN).  A fold that is a
// whole cycle in one launch keeps K8's selection state in registers; any other keeps it in HBM
// between launches: 2 b planes of pvec int32 keys here (lo, then hi) and the running sum in the
// context's d_acc -- (2b + 1) x 4 x pvec bytes, allocated by the first launch that needs them.
struct TrimState {
    int b = 0;    // values dropped per side; 0 = trimming off
    int vec = 0;  // PGH_TRIM_VEC: 4 or 1 forces K8's column width, 0 = by shard size
    DeviceBuf d_planes;
};

// Median FedAvg (PGH_MEDIAN).  K9 keeps everything on chip; K9p keeps the
// bisection's prefix in a plane of pvec words between its launches, and a slot list longer than
// a RowTab goes to the kernels as a device table: both allocated by the first fold that needs them.
struct MedianState {
    bool passes = false;  // PGH_MEDIAN_PATH=passes: K9p whatever the row count
    DeviceBuf d_prefix;   // uint32 [pvec]
    DeviceBuf d_rowidx;   // int32 [slots]
};

// Server optimizer (pgh_set_server_opt).  With one set, fold_launch runs every
// fp32 FINAL against the -0 plane into the delta plane and K10 behind it, which reads the committed
// moments and writes the pending ones; pgh_server_opt_commit swaps the two.  All planes are
// float [pvec] and belong to the model: pgh_reset / pgh_reserve keep them (rules_slab_freed does not
// touch them), a new layout or shard drops them and the setting (rules_shard_set -> release).
struct ServerOptState {
    int kind = 0;  // pgh_server_opt; 0 = off
    float lr = 0.f, beta1 = 0.f, beta2 = 0.f, tau = 0.f, c1 = 0.f, c2 = 0.f;
    DeviceBuf d_nz, d_d;          // -0.0f everywhere; d = -g of the last FINAL
    DeviceBuf d_m, d_v;           // committed
    DeviceBuf d_m2, d_v2;         // pending: written by K10, committed by the swap
    bool pending = false;         // a FINAL has run since the last commit / upload / (re)initialisation
    // the param ranges K10 has written into the pending planes since then: at the commit every param
    // outside them keeps its committed moments (a FINAL over part of the shard)
    std::vector<std::pair<int64_t, int64_t>> cov;
    int64_t steps = 0;            // commits since the state was initialised
    int64_t pvec = 0;             // the planes' length (pvec when they were allocated)

    void nothing_pending() { pending = false; cov.clear(); }  // after a commit, an upload, an initialisation
    void release();  // planes and setting; the caller has waited for the context's work
};

}  // namespace pgh_detail
