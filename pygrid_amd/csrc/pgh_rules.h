// What each averaging rule and the server optimizer keep in a single-GPU context: one struct per feature,
// members of struct pgh_ctx (pgh_ctx.h) as clip, noise, geo, trust, krum, trim, med and opt, and what they share:
// the row reductions and their two per-slot caches (RowSums, rowsums; a cache is a RowCache), the rows a
// row-wise rule includes (IncludedRows, in geo and trust), the fold's weights (FoldWeights, fw) and the -0 plane
// (NegZeroPlane, nz).  Their owners release with the context.
// The code that works on them: pgh_rules.cpp (every rule, the noise and the lifecycle calls rules_*),
// pgh_serveropt.cpp (opt).  Not installed.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "pgh_host.h"
#include "pgh_kernels.h"
#include "pgh_res.h"

struct pgh_ctx;

namespace pgh_detail {

// One per-slot cache of a row reduction: the state machine (SlotCache, pgh_host.h) with the device buffer its
// kernel writes, by slab row, the pinned image the D2H behind the kernel fills, and the event recorded behind
// that D2H.  `what` names the values in an allocation error.
struct RowCache : SlotCache {
    const char* what;
    DeviceBuf d;   // double [slots]
    PinnedBuf h;   // double [slots]
    Event ev;
    explicit RowCache(const char* w) : what(w) {}
    bool alloc(size_t slots) { return d.reserve(8 * slots) && h.reserve(8 * slots); }
    // What the values were computed against changed or went.  A kernel still in flight is waited for first, so
    // that "nothing queued" keeps meaning "nobody writes the shared tile partials" for RowSums::wait's callers.
    void stale() {
        if (anything_queued()) (void)hipEventSynchronize(ev);
        all_stale();
    }
    void slab_freed() {  // the streams are idle
        d.reset();
        h.reset();
        clear();
    }
};

struct RowOp;  // a row reduction against a plane: its launcher and its bytes per tile (pgh_rules.cpp)

// What the row-wise rules share (clipping, the geometric median, the Multi-Krum selection, the trust rule): two
// per-slot caches -- `sq`, K7's sums of squares, and `dot`, K14's inner products with the cycle's trust root --
// and everything device-side that the row reductions (K7, K12, K13, K14) need.  A cached reduction runs on the
// copy stream (queue_cached): behind the row's ingest, ahead of any later overwrite of the slot, and K14 behind
// the row's K7, since all of them write the one set of tile partials and one stream orders them.  Its values
// come back through the cache's pinned image in a small D2H on the same stream, followed by the cache's event.
// An ingest into a slot resets its entry in both caches (slot_written); a new root resets every dot
// (dots_stale).  An uncached reduction (run_listed: K12, or K14 against another plane) runs on the stream its
// caller gives, after a wait, and its sums come back through d_dist / h_dist: the caches stay as they are.
// sq's buffers come with the tile partials, all three or none (ensure); dot's with the first queued K14.
// The methods are in pgh_rules.cpp.
struct RowSums {
    RowCache sq{"clipping sums"}, dot{"trust rule's dots"};
    DeviceBuf d_part;               // double [slots][ceil(pg / SUMSQ_TILE)] tile partials, K7's, K12's and K14's
    DeviceBuf d_dist;               // double [slots]: an uncached reduction's sums, by slab row
    PinnedBuf h_dist;
    // K13's (Multi-Krum's pairwise distances), allocated by the first pgh_row_pairdist / pgh_krum_select: the
    // tile partials of one batch of anchors, at most pair_budget bytes whatever n and the model; the n x n
    // matrix; the listed slab rows as a device table
    DeviceBuf d_pair_part, d_pair, d_pair_rows;
    size_t pair_budget = (size_t)1 << 30;  // PGH_PAIRDIST_BUDGET (bytes) lowers it, for tests of the batching

    double at(int slot) const { return sq.at(slot); }       // after wait(): the sum of a slot queued before it
    double dot_at(int slot) const { return dot.at(slot); }  // after wait(): the dot, likewise
    void reserved(int slots) {  // pgh_reserve: the caches at their new length
        for (RowCache* r : {&sq, &dot}) r->reserved(slots);
    }
    // the diffs in slots [slot, slot + n) are being replaced: their cached sums and dots were the old diffs'
    void slot_written(int slot, int n) {
        for (RowCache* r : {&sq, &dot}) r->written(slot, n);
    }
    void dots_stale() { dot.stale(); }  // the root changed or went: every cached dot was the old root's
    void forget() {  // every slot back to NONE (pgh_reset)
        for (RowCache* r : {&sq, &dot}) r->forget();
    }
    void slab_freed() {  // the streams are idle: every buffer sized by the slab goes, and the caches
        for (auto* v : {&d_part, &d_dist, &d_pair_part, &d_pair, &d_pair_rows}) v->reset();
        h_dist.reset();
        for (RowCache* r : {&sq, &dot}) r->slab_freed();
    }
    // the kernel arguments of any of the reductions from the context, the sums going to `sums`
    pgh::SumsqArgs args(pgh_ctx* c, double* sums) const;
    int ensure(pgh_ctx* c);  // the tile partials, sq's buffer and its pinned image: all three or none
    // one launch of `op` per run of the listed slots (for_row_runs, pgh_ctx.h) on stream s, the sums to `sums`
    int launch_rows(pgh_ctx* c, const RowOp& op, const float* plane, const int32_t* slots, size_t n, double* sums, hipStream_t s);
    // `op` against `plane` (K7 reads none) on the copy stream for those of `slots` that `cache` has no value of
    // yet, the D2H of the values and the cache's event
    int queue_cached(pgh_ctx* c, RowCache& cache, const RowOp& op, const float* plane, const int32_t* slots, int n);
    int wait(pgh_ctx* c);  // nothing is queued afterwards: the queued sums are in at(), the queued dots in dot_at()
    // `op` over the listed slots against `plane` on stream s through d_dist / h_dist, the D2H and the wait:
    // D[k] = the sum of slots[k]
    int run_listed(pgh_ctx* c, const RowOp& op, const std::vector<int32_t>& slots, const float* plane, hipStream_t s, double* D);
    // K13 over the listed slots (n <= PAIRDIST_MAX_ROWS) on stream s in batches of anchors, the D2H and the wait:
    // D[a * n + b] = the squared distance of slots[a] to slots[b], symmetric, +0.0 on the diagonal
    int pairdist(pgh_ctx* c, const int32_t* slots, int n, hipStream_t s, double* D);
};

// The fold's per-client weights (fold order) and their device copy.  Four writers: the caller
// (pgh_set_weights), the clip scales, the geometric median's final weights, the trust rule's.  A rule that wrote them for the
// resident slab as it is marks them valid for clients [0, n): range folds and repeated closes reuse them.
// PGH_WEIGHTED_MEAN folds with whatever the vector holds, whoever wrote it.
struct FoldWeights {
    enum Writer : uint8_t { CALLER = 0, CLIP = 1, GEOMED = 2, TRUST = 3 };
    std::vector<float> v;
    DeviceBuf d;             // float per client
    bool on_device = false;
    Writer writer = CALLER;  // who replaced the contents last
    int64_t n_valid = -1;    // >= 0: `writer`'s weights of resident clients [0, n_valid) of the slab as it is

    // The contents are about to be replaced (or were): the one place that drops the device copy's claim and
    // the validity.  Returns the vector to write.
    std::vector<float>& replace(Writer w) {
        on_device = false;
        writer = w;
        n_valid = -1;
        return v;
    }
    void clear() { replace(CALLER).clear(); }
    // the slab or a rule's setting changed under the contents: they stay, a resident fold of the rule computes anew
    void stale() { n_valid = -1; }
    void stale(Writer w) { if (writer == w) stale(); }
    bool valid(Writer w, int64_t n) const { return writer == w && n_valid == n; }
    void validate(int64_t n) { n_valid = n; }
    void slab_freed() {  // the device copy goes with the slab's other buffers; the contents stay
        d.reset();
        replace(writer);
    }
    int upload(pgh_ctx* c, hipStream_t s);  // the contents on the device when this returns (pgh_reduce.cpp)
};

// The context's plane of -0.0f, float [pvec]: a FINAL fold against it writes -avg (the server optimizer's and the
// noise's delta planes, the geometric median's iterate).  Allocated and filled by the first tenant that needs it,
// complete before ensure returns; released where the shard or pvec changes and with the context, never when
// a tenant is switched off or the slab is reserved again.
struct NegZeroPlane {
    DeviceBuf d;
    int ensure(pgh_ctx* c, hipStream_t s);  // pgh_rules.cpp
    const float* get() const { return d.as<float>(); }
};

// Clipped FedAvg (pgh_set_clip_norm, PGH_CLIPPED_MEAN): the bound, the norms of the running
// cycle's slot folds and the tallies.  The sums: RowSums; the scales: FoldWeights (writer CLIP).
struct ClipState {
    float c = 0.f;                    // the L2 bound; 0 = clipping off
    std::vector<double> norms;        // slot folds of the running cycle, in fold order (beside the weights)
    int64_t rows = 0, clipped = 0;    // folds finished since pgh_reset / pgh_reserve
    double max_norm = 0.0;

    void forget() {  // the running cycle and the totals (pgh_reset)
        norms.clear();
        rows = clipped = 0;
        max_norm = 0.0;
    }
    void count(const float* scales, const double* row_norms, int64_t n);  // rows into the finished totals
    // the slot folds of the running cycle into the finished totals: scales[k] beside norms[k]
    void count_cycle(const std::vector<float>& scales) {
        count(scales.data(), norms.data(), (int64_t)std::min(norms.size(), scales.size()));
    }
};

// Gaussian noise on the clipped close (pgh_set_dp_noise): a modifier of the clip
// rule, not a rule of its own.  With z > 0 fold_launch runs every fp32 FINAL -- PGH_CLIPPED_MEAN only,
// any other mode is refused -- against the context's -0 plane into a delta plane and K11 behind it: the server
// optimizer's delta plane when one is set (K10 follows K11), else the one owned here, allocated by the first
// noised FINAL.  The setting belongs to the model like the optimizer's: pgh_reset / pgh_reserve keep it,
// a new layout or shard clears it (rules_shard_set).
struct NoiseState {
    float z = 0.f;        // the noise multiplier; 0 = off
    uint64_t key = 0;
    uint32_t round = 0;
    DeviceBuf d_d;        // float [pvec]: d = -g of the last noised FINAL without an optimizer
    int64_t pvec = 0;     // the plane's length
    double sigma_last = 0.0;  // what the last noised FINAL used: z * C / N, and N
    int64_t n_last = 0;

    void release() {  // plane and setting; the caller has waited for the context's work
        d_d.reset();
        z = 0.f;
        pvec = 0;
    }
};

// The rows of a close that a row-wise rule folds -- those whose K7 sum is finite, in fold order -- and what its
// last computation of the weights saw of them (pgh_geomed_stats, pgh_trust_stats).
struct IncludedRows {
    std::vector<int32_t> rows;  // the included slots, in fold order
    int64_t n_rows = 0, n_excluded = 0;
    float max_weight = 0.f;
    void forget() {
        rows.clear();
        n_rows = n_excluded = 0;
        max_weight = 0.f;
    }
};

// Geometric-median FedAvg (pgh_set_geomed, PGH_GEOMETRIC_MEDIAN): the smoothed
// Weiszfeld iteration.  With the rule on every ingest queues K7 like clipping (RowSums: the cached sums are
// iteration 0's squared distances and say which rows are excluded).  A close computes the final weights on the
// context's stream -- per inner iteration a weighted fold against the -0 plane into d_negv (= -v), K12
// against it, a D2H of the distances, the host step -- and leaves them in the context's FoldWeights (writer
// GEOMED, fold order of the included rows) for the one FINAL fold, which is the weighted fold over `inc.rows`.
// The iterate plane is float [pvec], allocated by the first close that iterates (iters >= 2) or by pgh_row_distsq.
struct GeomedState {
    int iters = 0;                  // 0 = the rule is off
    float nu = 0.f;
    IncludedRows inc;
    float W = 0.f;                  // the f32 left fold of the final weights
    DeviceBuf d_negv;               // -v of the last inner iteration (or -point)
    double objective = 0.0;         // of the last computation of the weights (pgh_geomed_stats)

    void forget() {  // the included rows and the tallies (pgh_reset); the setting stays
        inc.forget();
        objective = 0.0;
    }
    void release() {  // plane and setting; the caller has waited for the context's work
        d_negv.reset();
        iters = 0;
        nu = 0.f;
        forget();
    }
};

// Trust-bootstrapped FedAvg (pgh_set_trust, pgh_trust_root, PGH_TRUSTED_MEAN): FLTrust.
// With the rule on every ingest queues K7 like clipping, and, while the cycle's root is valid, K14 behind it
// (RowSums: the cached sums and dots).  A close computes what is missing in one batch, runs the host step
// (trust_weights, pgh_host.cpp) and leaves the weights in the context's FoldWeights (writer TRUST, fold order of
// the included rows) for the one FINAL fold, the weighted fold over `inc.rows` with the divisor 1.  The root plane
// is float [pvec], zero past the root, allocated by the first pgh_trust_root and kept over pgh_reset /
// pgh_reserve (the validity is not); pgh_row_dot's scratch plane likewise, by its first call.
struct TrustState {
    bool on = false;
    bool root_valid = false;        // a root set since pgh_reset / pgh_reserve
    double s0 = 0.0;                // K7's sum of squares of the root
    DeviceBuf d_root, d_point;      // float [pvec]
    int64_t pvec = 0;               // the planes' length
    IncludedRows inc;
    int64_t n_trusted = 0;          // of the last computation of the weights (pgh_trust_stats)
    double total_trust = 0.0;

    void forget() {  // the cycle's root, the included rows and the tallies (pgh_reset, pgh_reserve); the setting stays
        root_valid = false;
        s0 = 0.0;
        inc.forget();
        n_trusted = 0;
        total_trust = 0.0;
    }
    void release() {  // planes and setting; the caller has waited for the context's work
        d_root.reset();
        d_point.reset();
        pvec = 0;
        on = false;
        forget();
    }
};

// Multi-Krum selection (pgh_krum_select): a call, not a setting -- what the last
// selection saw, for pgh_krum_stats.  The sums and the distance matrix: RowSums.
struct KrumState {
    int64_t n_rows = 0, n_excluded = 0, n_picked = 0;
    double max_picked_score = 0.0, min_dropped_score = 0.0;  // (min_dropped: +inf when nothing was dropped)
    void forget() { *this = KrumState{}; }  // pgh_reset
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
// fp32 FINAL against the context's -0 plane into the delta plane and K10 behind it, which reads the committed
// moments and writes the pending ones; pgh_server_opt_commit swaps the two.  All planes are
// float [pvec] and belong to the model: pgh_reset / pgh_reserve keep them (rules_slab_freed does not
// touch them), a new layout or shard drops them and the setting (rules_shard_set -> release).
struct ServerOptState {
    int kind = 0;  // pgh_server_opt; 0 = off
    float lr = 0.f, beta1 = 0.f, beta2 = 0.f, tau = 0.f, c1 = 0.f, c2 = 0.f;
    DeviceBuf d_d;                // d = -g of the last FINAL
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
