// libpygrid_hip: the averaging rules on top of the fp32 fold -- what a mode may do (check_mode_use); the row
// reductions (RowSums: K7 and K14 through their per-slot caches, K12 and K14 over a listed set of rows, K13) and
// the Multi-Krum selection over them; clipping's scales and tallies; the Gaussian noise on the clipped close (K11
// behind a FINAL launch, its plane, setting and entry points); the trimmed mean's state planes (K8); the
// median's driver and row table (K9, K9p); what the geometric median and the trust rule share (the finite rows
// of a close, the resident weights, the plan over the included rows) and each one's own: the inner iterations
// and final weights (K12 between weighted folds), the root and the weights from the cached dots; the context's
// -0 plane; what the rules' state does at each lifecycle event of the context (rules_*: the one call each
// event's site makes) and what they hand a fold driver before its launches (rules_slot_plan,
// rules_resident_plan).  The state itself: pgh_rules.h.
// (struct pgh_ctx and the shared helpers: pgh_ctx.h)
#include "pgh_ctx.h"

#include <cmath>

using namespace pgh_detail;

// (the public entry points take their C linkage from include/pgh_api.h)

namespace pgh_detail {

namespace {
int mode_use_rule(pgh_ctx* c, int mode, ModeUse use);
int queue_sums(pgh_ctx* c, const int32_t* slots, int n);
int queue_dots(pgh_ctx* c, const int32_t* slots, int n);
}

int check_mode_use(pgh_ctx* c, int mode, ModeUse use) {
    RC(mode_use_rule(c, mode, use));
    // a RESIDENT fold and a closing slot fold end in a FINAL launch (noise is never on for a group or a stream)
    return use == USE_RESIDENT || use == USE_SLOT_FINAL ? check_noise_final(c, mode) : PGH_OK;
}

int check_noise_final(pgh_ctx* c, int mode) {
    if (noise_on(c) && mode != PGH_CLIPPED_MEAN)
        return fail(c, PGH_E_STATE, "DP noise is set (pgh_set_dp_noise): only PGH_CLIPPED_MEAN may close a cycle, not mode %d", mode);
    return PGH_OK;
}

namespace {
// The rules that close a whole cycle in one fold (rules_one_fold_cycle, which has their names): every row at
// once; with whole_rows the whole row of each, like clipping.
int one_fold_cycle_use(pgh_ctx* c, int mode, ModeUse use, bool whole_rows) {
    const char* a_rule = rules_one_fold_cycle(mode);  // "a median"
    const char* rule = a_rule + 2;                    // "median"
    if (use == USE_STREAM) return fail(c, PGH_E_UNSUPPORTED, "STREAM use takes no %s: it needs every row at once", rule);
    if (use == USE_SLOT_EARLY) return fail(c, PGH_E_UNSUPPORTED, "%s needs every row at once: nothing can be folded early", a_rule);
    if (!whole_rows) return PGH_OK;
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "group contexts take no %s: the shards each hold part of a row", rule);
    if (c->layout && c->pg != c->P)
        return fail(c, PGH_E_UNSUPPORTED, "%s needs whole rows: the shard [%lld,%lld) is narrower than the model", a_rule, (long long)c->lo, (long long)c->hi);
    return PGH_OK;
}

int mode_use_rule(pgh_ctx* c, int mode, ModeUse use) {
    switch (mode) {
    case PGH_MEAN: case PGH_ITERATIVE_MEAN: case PGH_WEIGHTED_MEAN:
        return PGH_OK;
    case PGH_CLIPPED_MEAN:
        if (use == USE_STREAM) return fail(c, PGH_E_UNSUPPORTED, "STREAM use does not clip: a scale needs the whole row of every client");
        if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "group contexts do not clip: the shards each hold part of a row");
        if (!(c->clip.c > 0.f)) return fail(c, PGH_E_STATE, "PGH_CLIPPED_MEAN needs a bound: call pgh_set_clip_norm first");
        return PGH_OK;
    case PGH_TRIMMED_MEAN:
        if (use == USE_STREAM) return fail(c, PGH_E_UNSUPPORTED, "STREAM use does not trim: fold a RESIDENT slab or slots");
        if (!c->grp && c->trim.b == 0) return fail(c, PGH_E_STATE, "PGH_TRIMMED_MEAN needs a trim count: call pgh_set_trim first");
        return PGH_OK;
    case PGH_MEDIAN:
        return one_fold_cycle_use(c, mode, use, false);
    case PGH_GEOMETRIC_MEDIAN:
        RC(one_fold_cycle_use(c, mode, use, true));
        if (c->geo.iters == 0) return fail(c, PGH_E_STATE, "PGH_GEOMETRIC_MEDIAN needs its setting: call pgh_set_geomed first");
        return PGH_OK;
    case PGH_TRUSTED_MEAN:
        RC(one_fold_cycle_use(c, mode, use, true));
        if (!c->trust.on) return fail(c, PGH_E_STATE, "PGH_TRUSTED_MEAN needs its setting: call pgh_set_trust first");
        if (!c->trust.root_valid) return fail(c, PGH_E_STATE, "PGH_TRUSTED_MEAN needs the cycle's root: call pgh_trust_root (none set since pgh_reset / pgh_reserve)");
        if (noise_on(c)) return fail(c, PGH_E_STATE, "DP noise is set (pgh_set_dp_noise): a trusted mean takes none");
        return PGH_OK;
    default:
        return fail(c, PGH_E_ARG, "unknown averaging mode %d", mode);
    }
}
}  // namespace

// ---- the lifecycle events of the context, as the rules see them -------------------------------------------

bool rules_made(pgh_ctx* c) {
    if (const char* e = std::getenv("PGH_TRIM_VEC")) c->trim.vec = std::atoi(e) == 4 ? 4 : std::atoi(e) == 1 ? 1 : 0;
    if (const char* e = std::getenv("PGH_MEDIAN_PATH")) c->med.passes = std::strcmp(e, "passes") == 0;
    if (const char* e = std::getenv("PGH_PAIRDIST_BUDGET")) {  // bytes of K13's tile partials per batch of anchors
        const long long v = std::atoll(e);
        if (v > 0 && (unsigned long long)v < c->rowsums.pair_budget) c->rowsums.pair_budget = (size_t)v;
    }
    return c->rowsums.sq.ev.make() == hipSuccess && c->rowsums.dot.ev.make() == hipSuccess;
}

void rules_slab_freed(pgh_ctx* c) {  // the streams are idle (free_slab synchronised them)
    for (auto* v : {&c->trim.d_planes, &c->med.d_prefix, &c->med.d_rowidx, &c->geo.d_negv}) v->reset();
    c->rowsums.slab_freed();
    c->geo.forget();
    c->trust.forget();  // (the root's validity goes with the cycle; its plane is sized by the shard and stays)
    c->krum.forget();
    c->clip.forget();
}

void rules_shard_set(pgh_ctx* c, int64_t lo, int64_t hi, int64_t pvec, bool keep_opt) {
    const bool same_shard = lo == c->lo && hi == c->hi;
    const bool same = keep_opt && same_shard;
    if (!(same && pvec == c->opt.pvec)) c->opt.release();
    if (!(same && pvec == c->noise.pvec)) c->noise.release();  // (free_slab has synchronised the streams)
    if (!(same_shard && pvec == c->pvec)) c->nz.d.reset();     // (its tenants above and below are gone with it)
    if (hi - lo != c->P) c->clip.c = 0.f;  // a norm needs the whole row (pgh_set_clip_norm refuses too)
    c->geo.release();  // (free_slab has dropped the plane; the setting goes with the layout or shard)
    c->trust.release();
}

void rules_reserved(pgh_ctx* c, int slots) { c->rowsums.reserved(slots); }

void rules_reset(pgh_ctx* c) {
    c->rowsums.forget();
    c->clip.forget();
    c->geo.forget();
    c->trust.forget();
    c->krum.forget();
}

void rules_slot_written(pgh_ctx* c, int slot, int n) {
    c->rowsums.slot_written(slot, n);
    c->fw.stale();  // the slab is no longer the one a rule's resident weights were computed for
}

void rules_folds_restarted(pgh_ctx* c) { c->clip.norms.clear(); }

void rules_cycle_finished(pgh_ctx* c, int mode) {
    if (mode != PGH_CLIPPED_MEAN) return;
    c->clip.count_cycle(c->fw.v);  // the cycle's rows join the finished totals (pgh_clip_stats)
    c->clip.norms.clear();
}

int rules_row_ingested(pgh_ctx* c, int slot) {
    if (!norms_wanted(c)) return PGH_OK;
    const int32_t sl = slot;
    RC(queue_sums(c, &sl, 1));
    // the trust rule with the cycle's root in place: the row's K14 behind its K7, both behind the next report's copy
    if (trust_on(c) && c->trust.root_valid) RC(queue_dots(c, &sl, 1));
    return PGH_OK;
}

const char* rules_one_fold_cycle(int mode) {
    return mode == PGH_MEDIAN ? "a median" : mode == PGH_GEOMETRIC_MEDIAN ? "a geometric median" : mode == PGH_TRUSTED_MEAN ? "a trusted mean" : nullptr;
}

int NegZeroPlane::ensure(pgh_ctx* c, hipStream_t s) {
    if (d) return PGH_OK;
    if (!d.reserve(4 * (size_t)c->pvec)) return fail(c, PGH_E_OOM, "allocation of the -0 plane (%zu bytes) failed", 4 * (size_t)c->pvec);
    const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)d.as<void>(), (int)0x80000000u, (size_t)c->pvec, s);
    // (complete before any tenant reads it, on whichever stream: paid once per shard)
    if (e == hipSuccess && hipStreamSynchronize(s) == hipSuccess) return PGH_OK;
    d.reset();
    return fail(c, PGH_E_HIP, "filling the -0 plane failed: %s", hipGetErrorString(e));
}

// ---- trimmed mean: K8's arguments and state planes ---------------------------------------------------------

int trim_args(pgh_ctx* c, pgh::FedavgArgs* a) {
    a->mode = pgh::MODE_TRIMMED;
    a->trim_b = c->trim.b;
    a->trim_vec = c->trim.vec;
    if ((a->flags & (pgh::FL_FIRST | pgh::FL_FINAL)) == (pgh::FL_FIRST | pgh::FL_FINAL)) return PGH_OK;
    // (a buffer left from a larger b serves; one too small is only ever replaced before a cycle's
    // first launch -- pgh_set_trim -- and hipFree waits for the launches that still use it)
    if (!c->trim.d_planes.reserve(2 * (size_t)c->trim.b * 4 * (size_t)c->pvec))
        return fail(c, PGH_E_OOM, "allocation of the trimmed mean's %d state planes failed", 2 * c->trim.b);
    a->tstate = c->trim.d_planes.as<int32_t>() + a->map.off;
    a->tplane = c->pvec;
    return PGH_OK;
}

// ---- median: the row table and the fold's launches (K9, K9p) ------------------------------------------------

int median_row_table(pgh_ctx* c, const int32_t* slots, int n, hipStream_t s) {
    if (!c->med.d_rowidx.reserve(sizeof(int32_t) * (size_t)c->slots))
        return fail(c, PGH_E_OOM, "allocation of the median's row table (%d rows) failed", c->slots);
    std::vector<int32_t> rows((size_t)n);
    for (int k = 0; k < n; ++k) rows[(size_t)k] = slots[k] * c->parties;
    // (an earlier fold that still reads the table runs on c->stream too, or has been waited for)
    CK(c, hipMemcpyAsync(c->med.d_rowidx.as<int32_t>(), rows.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    CK(c, hipStreamSynchronize(s));  // rows is freed on return
    return PGH_OK;
}

int median_fold(pgh_ctx* c, const pgh::FedavgArgs& a, const pgh::Rows& rows, hipStream_t s) {
    pgh::MedianArgs m{};
    m.diffs = a.diffs;
    m.map = a.map;
    m.n_rows = a.n_rows;
    m.p = a.p;
    m.ckpt = a.ckpt;
    m.out = a.out;
    const uint64_t slab = 4ull * (uint64_t)a.n_rows * (uint64_t)a.p, rp = (uint64_t)a.p;
    if (median_variant(c, a.n_rows) == 50)  // K9: the slab once, ckpt in, out
        return timed_launch(c, s, slab + 8 * rp, [&] { return pgh::launch_median(m, rows, s); });
    if (!c->med.d_prefix.reserve(sizeof(uint32_t) * (size_t)c->pvec))
        return fail(c, PGH_E_OOM, "allocation of the median's prefix plane failed");
    m.prefix = c->med.d_prefix.as<uint32_t>() + a.map.off;
    // K9p: bits 31 .. 0, then the upper middle of an even count; each launch reads the rows, reads
    // the prefix plane (not the first) and writes it, or ckpt in and out (the last)
    const int last = (a.n_rows & 1) ? 0 : -1;
    for (int bit = 31; bit >= last; --bit) {
        const uint64_t bytes = slab + (bit == 31 ? 0 : 4 * rp) + (bit == last ? 8 * rp : 4 * rp);
        RC(timed_launch(c, s, bytes, [&] { return pgh::launch_median_pass(m, rows, bit, s); }));
    }
    return PGH_OK;
}

// ---- clipped FedAvg: the tallies -------------------------------------------------------------------------------

void ClipState::count(const float* scales, const double* row_norms, int64_t n) {
    for (int64_t k = 0; k < n; ++k) {
        rows += 1;
        clipped += scales[k] == 1.0f ? 0 : 1;
        if (!std::isnan(max_norm) && (std::isnan(row_norms[k]) || row_norms[k] > max_norm)) max_norm = row_norms[k];
    }
}

// ---- the row reductions: K7 and K14 through their caches, K12 and K14 over listed rows (RowSums) ---------------

// A row reduction against a plane: its launcher, the f64s it moves per tile and row (the partial out: K7; out and
// in again: K12 and K14, whose plane comes once per row chunk, from L2 mostly) and what an allocation error
// calls its sums.
struct RowOp {
    hipError_t (*launch)(const pgh::DistsqArgs&, const pgh::Rows&, hipStream_t);
    uint64_t tile_bytes;
    const char* what;
};
namespace {
const RowOp ROW_SUMSQ{[](const pgh::DistsqArgs& a, const pgh::Rows& r, hipStream_t s) { return pgh::launch_row_sumsq(a.s, r, s); }, 8, "clipping sums"};
const RowOp ROW_DISTSQ{pgh::launch_row_distsq, 16, "geometric median's distances"};
const RowOp ROW_DOT{pgh::launch_row_dot, 16, "row dots"};
}  // namespace

int RowSums::ensure(pgh_ctx* c) {
    if (d_part) return PGH_OK;
    const size_t ntiles = (size_t)((c->pg + pgh::SUMSQ_TILE - 1) / pgh::SUMSQ_TILE);
    const size_t rows = (size_t)c->slots;
    if (!d_part.reserve(8 * rows * ntiles) || !sq.alloc(rows)) {
        d_part.reset();  // (the test above: all three or none)
        return fail(c, PGH_E_OOM, "allocation of the clipping sums (%zu rows x %zu tiles) failed", rows, ntiles);
    }
    return PGH_OK;
}

pgh::SumsqArgs RowSums::args(pgh_ctx* c, double* sums) const {
    pgh::SumsqArgs a{};
    a.slab = c->d_slab.as<float>();
    a.map = slab_map(c);
    a.p = c->pg;
    a.ntiles = (c->pg + pgh::SUMSQ_TILE - 1) / pgh::SUMSQ_TILE;
    a.part = d_part.as<double>();
    a.sumsq = sums;
    return a;
}

int RowSums::launch_rows(pgh_ctx* c, const RowOp& op, const float* plane, const int32_t* slots, size_t n, double* sums, hipStream_t s) {
    pgh::DistsqArgs a{args(c, sums), plane};
    // HBM bytes of a row: the row, its tile partials
    const uint64_t row_bytes = 4ull * (uint64_t)c->pg + op.tile_bytes * (uint64_t)a.s.ntiles;
    return for_row_runs(c, slots, n, [&](const pgh::Rows& rows, size_t, size_t m) {
        a.s.n_rows = (int)m;
        return timed_launch(c, s, m * row_bytes, [&] { return op.launch(a, rows, s); });
    });
}

namespace {
// sums[lo, hi] of the listed slots from the device to their pinned image on stream s.  Entries of other slots
// inside [lo, hi] are rewritten with what the device holds for them: the same value an earlier copy brought
// (same stream), or one nobody reads.
int sums_d2h(pgh_ctx* c, const int32_t* slots, size_t n, double* h, const double* d, hipStream_t s) {
    const auto mm = std::minmax_element(slots, slots + n);
    const int32_t lo = *mm.first, hi = *mm.second;
    CK(c, hipMemcpyAsync(h + lo, d + lo, 8 * (size_t)(hi - lo + 1), hipMemcpyDeviceToHost, s));
    return PGH_OK;
}
}  // namespace

int RowSums::queue_cached(pgh_ctx* c, RowCache& cache, const RowOp& op, const float* plane, const int32_t* slots, int n) {
    const std::vector<int32_t> todo = cache.missing(slots, n);
    if (todo.empty()) return PGH_OK;
    RC(ensure(c));
    if (!cache.alloc((size_t)c->slots)) return fail(c, PGH_E_OOM, "allocation of the %s (%d rows) failed", cache.what, c->slots);
    const hipStream_t s = c->copy;
    RC(launch_rows(c, op, plane, todo.data(), todo.size(), cache.d.as<double>(), s));
    RC(sums_d2h(c, todo.data(), todo.size(), cache.h.as<double>(), cache.d.as<double>(), s));
    CK(c, hipEventRecord(cache.ev, s));
    cache.mark_queued(todo);
    return PGH_OK;
}

int RowSums::wait(pgh_ctx* c) {
    for (RowCache* r : {&sq, &dot})
        if (r->anything_queued()) {
            CK(c, hipEventSynchronize(r->ev));
            r->harvest(r->h.as<double>());
        }
    return PGH_OK;
}

// (The tile partials are free: everything queued has been waited for.  The sums go through d_dist / h_dist:
// neither cache is touched.)
int RowSums::run_listed(pgh_ctx* c, const RowOp& op, const std::vector<int32_t>& slots, const float* plane, hipStream_t s, double* D) {
    RC(wait(c));
    RC(ensure(c));
    if (!d_dist.reserve(8 * (size_t)c->slots) || !h_dist.reserve(8 * (size_t)c->slots))
        return fail(c, PGH_E_OOM, "allocation of the %s (%d rows) failed", op.what, c->slots);
    RC(launch_rows(c, op, plane, slots.data(), slots.size(), d_dist.as<double>(), s));
    RC(sums_d2h(c, slots.data(), slots.size(), h_dist.as<double>(), d_dist.as<double>(), s));
    CK(c, hipStreamSynchronize(s));
    for (size_t k = 0; k < slots.size(); ++k) D[k] = h_dist.as<double>()[slots[k]];
    return PGH_OK;
}

namespace {
// K7 into its cache for those of `slots` that have no sum yet; K14 against the cycle's root, likewise (on the
// copy stream like K7: the two share the tile partials, and one stream orders them)
int queue_sums(pgh_ctx* c, const int32_t* slots, int n) {
    return c->rowsums.queue_cached(c, c->rowsums.sq, ROW_SUMSQ, nullptr, slots, n);
}
int queue_dots(pgh_ctx* c, const int32_t* slots, int n) {
    return c->rowsums.queue_cached(c, c->rowsums.dot, ROW_DOT, c->trust.d_root.as<float>(), slots, n);
}
}  // namespace

// (K7's and K12's buffers are not touched: the cached sums stay what they were.)
int RowSums::pairdist(pgh_ctx* c, const int32_t* slots, int n, hipStream_t s, double* D) {
    const size_t nn = (size_t)n * (size_t)n;
    std::fill_n(D, nn, 0.0);  // the diagonal, and everything when n < 2
    if (n < 2) return PGH_OK;
    pgh::PairdistArgs a{};
    a.slab = c->d_slab.as<float>();
    a.map = slab_map(c);
    a.p = c->pg;
    a.ntiles = (c->pg + pgh::SUMSQ_TILE - 1) / pgh::SUMSQ_TILE;
    a.n = n;
    // the anchors a batch takes: whole anchor blocks within the budget, or what fits of one
    const size_t per_anchor = 8 * (size_t)n * (size_t)a.ntiles;
    size_t batch = pair_budget / per_anchor;
    if (batch == 0)
        return fail(c, PGH_E_OOM, "pairwise distances: the tile partials of one row against %d (%zu bytes) exceed the budget of %zu", n, per_anchor, pair_budget);
    if (batch > (size_t)pgh::PAIRDIST_RA) batch -= batch % (size_t)pgh::PAIRDIST_RA;
    batch = std::min(batch, (size_t)n - 1);  // (the last row anchors nothing)
    if (!d_pair_part.reserve(batch * per_anchor) || !d_pair.reserve(8 * nn) || !d_pair_rows.reserve(sizeof(int32_t) * (size_t)pgh::PAIRDIST_MAX_ROWS))
        return fail(c, PGH_E_OOM, "allocation of the pairwise distances (%d rows, %zu anchors a batch) failed", n, batch);
    a.part = d_pair_part.as<double>();
    a.dist = d_pair.as<double>();
    bool run = true;
    for (int k = 0; k < n; ++k) run = run && slots[k] == slots[0] + k;
    std::vector<int32_t> tab((size_t)n);
    if (run) {
        a.row0 = slots[0] * c->parties;
    } else {
        for (int k = 0; k < n; ++k) tab[(size_t)k] = slots[k] * c->parties;
        // (an earlier K13 that read the table ran on this stream too)
        CK(c, hipMemcpyAsync(d_pair_rows.as<int32_t>(), tab.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
        CK(c, hipStreamSynchronize(s));  // tab is pageable: the copy has left it
        a.d_rows = d_pair_rows.as<int32_t>();
    }
    for (int a0 = 0; a0 < n - 1; a0 += (int)batch) {
        a.a0 = a0;
        a.na = std::min((int)batch, n - 1 - a0);
        // HBM bytes as issued, before the caches: every anchor block reads its own tile and the rows after it;
        // the pairs' partials out and in again, the sums out
        uint64_t rows_read = 0, pairs = 0;
        for (int b0 = a0; b0 < a0 + a.na; b0 += pgh::PAIRDIST_RA) rows_read += (uint64_t)(std::min(pgh::PAIRDIST_RA, a0 + a.na - b0) + n - 1 - b0);
        for (int k = a0; k < a0 + a.na; ++k) pairs += (uint64_t)(n - 1 - k);
        const uint64_t bytes = rows_read * 4ull * (uint64_t)c->pg + pairs * (16ull * (uint64_t)a.ntiles + 8ull);
        RC(timed_launch(c, s, bytes, [&] { return pgh::launch_row_pairdist(a, s); }));
    }
    std::vector<double> h(nn);
    CK(c, hipMemcpyAsync(h.data(), d_pair.as<double>(), 8 * nn, hipMemcpyDeviceToHost, s));
    CK(c, hipStreamSynchronize(s));
    for (int x = 0; x < n; ++x)
        for (int y = x + 1; y < n; ++y) D[(size_t)x * n + y] = D[(size_t)y * n + x] = h[(size_t)x * n + y];
    return PGH_OK;
}

// ---- clipped FedAvg: the scales and the tallies ------------------------------------------------------------

float clip_scale_of(double sumsq, float c) {
    const double norm = std::sqrt(sumsq);
    return norm <= (double)c ? 1.0f : (float)((double)c / norm);
}

namespace {
// weights[c0 + k] = the scale of slots[k] (K7 for the sums still missing in one batch, then the wait); norms
// receives sqrt(sumsq) beside them
int clip_set_scales(pgh_ctx* c, const int32_t* slots, int n, int64_t c0, std::vector<double>* norms) {
    RC(queue_sums(c, slots, n));
    RC(c->rowsums.wait(c));
    std::vector<float>& w = c->fw.replace(FoldWeights::CLIP);
    w.resize((size_t)(c0 + n));
    norms->resize((size_t)(c0 + n));
    for (int k = 0; k < n; ++k) {
        const double ss = c->rowsums.at(slots[k]);
        w[(size_t)(c0 + k)] = clip_scale_of(ss, c->clip.c);
        (*norms)[(size_t)(c0 + k)] = std::sqrt(ss);
    }
    return PGH_OK;
}

std::vector<int32_t> first_slots(int64_t n) {  // resident folds: client k is in slot k
    std::vector<int32_t> slots((size_t)n);
    for (int64_t k = 0; k < n; ++k) slots[(size_t)k] = (int32_t)k;
    return slots;
}

// Resident folds in PGH_CLIPPED_MEAN: the scales of clients [0, n), computed once per state of the slab --
// the range form and repeated folds reuse them.
int resident_clip_scales(pgh_ctx* c, int64_t n) {
    if (c->fw.valid(FoldWeights::CLIP, n)) return PGH_OK;
    std::vector<double> norms;
    RC(clip_set_scales(c, first_slots(n).data(), (int)n, 0, &norms));
    c->clip.count(c->fw.v.data(), norms.data(), n);
    c->fw.validate(n);
    return PGH_OK;
}

// ---- what the geometric median, the trust rule and the Multi-Krum selection share ------------------------------

// K7 for the sums of slots[0, n) still missing in one batch and the wait; then those of the slots whose sum is
// finite, in list order, into *inc and (sums nullable) their sums beside them.  Every other row is excluded: no
// fold and no later pass of the caller reads it.
int finite_rows(pgh_ctx* c, const int32_t* slots, int n, std::vector<int32_t>* inc, std::vector<double>* sums) {
    RC(queue_sums(c, slots, n));
    RC(c->rowsums.wait(c));
    for (int k = 0; k < n; ++k) {
        const double ss = c->rowsums.at(slots[k]);
        if (!std::isfinite(ss)) continue;
        inc->push_back(slots[k]);
        if (sums) sums->push_back(ss);
    }
    return PGH_OK;
}

// A resident fold of a rule that writes the included rows' weights: clients [0, n) in slots [0, n), computed
// (compute = the rule's slot weights) once per state of the slab and of whatever else makes them stale.
int resident_weights(pgh_ctx* c, FoldWeights::Writer writer, const IncludedRows& included, int64_t n,
                     int (*compute)(pgh_ctx*, const int32_t*, int)) {
    if (c->fw.valid(writer, n) && c->fw.v.size() == included.rows.size()) return PGH_OK;
    RC(compute(c, first_slots(n).data(), (int)n));
    c->fw.validate(n);
    return PGH_OK;
}

// the included rows alone, fold client k = the k-th of them; the rule supplies the divisor
void included_plan(FoldPlan* p, const IncludedRows& included, float divisor) {
    p->slots = included.rows.data();
    p->n = (int)included.rows.size();
    p->total = p->n;
    p->has_divisor = true;
    p->divisor = divisor;
    p->whole_rows = true;
}

// ---- geometric-median FedAvg: the inner iterations, the final weights -------------------------------------------

int geomed_plane(pgh_ctx* c, hipStream_t s) {  // the iterate plane, -0 until something is written to it
    GeomedState& g = c->geo;
    RC(c->nz.ensure(c, s));
    if (g.d_negv) return PGH_OK;
    if (!g.d_negv.reserve(4 * (size_t)c->pvec))
        return fail(c, PGH_E_OOM, "allocation of the geometric median's planes (%zu bytes each) failed", 4 * (size_t)c->pvec);
    return hipMemsetD32Async((hipDeviceptr_t)g.d_negv.as<void>(), (int)0x80000000u, (size_t)c->pvec, s) == hipSuccess
               ? PGH_OK
               : fail(c, PGH_E_HIP, "hipMemsetD32Async of the iterate plane failed");
}

// The final weights of a close over slots[0, n) in fold order (the included rows into geo.inc, their weights
// into the context's, W into geo.W): the inner iterations run whole-shard on the context's stream and are
// finished when this returns.  PGH_E_STATE with no row included; nothing is launched then.
int geomed_slot_weights(pgh_ctx* c, const int32_t* slots, int n) {
    GeomedState& g = c->geo;
    c->fw.stale();  // (the context's weights become this rule's, whatever happens below)
    std::vector<int32_t> inc;
    std::vector<double> D;  // iteration 0's squared distances: the sums
    RC(finite_rows(c, slots, n, &inc, &D));
    if (inc.empty()) return fail(c, PGH_E_STATE, "geometric median: none of the %d diffs is finite", n);
    const hipStream_t s = c->stream;
    std::vector<float> w(inc.size());
    float W = 0.f, mx = 0.f;
    double obj = 0.0;
    g.inc.rows = inc;
    for (int t = 0;; ++t) {
        if (!geomed_step(D.data(), (int64_t)D.size(), g.nu, w.data(), &W, &obj, &mx))
            return fail(c, PGH_E_STATE, "geometric median: no finite distance in iteration %d", t);
        c->fw.replace(FoldWeights::GEOMED) = w;
        if (t == g.iters - 1) break;
        // v^(t+1) as -v: the weighted fold against the -0 plane, whole shard; then every row's distance to it
        if (t == 0) {
            RC(order_after_ingest(c, s));
            RC(geomed_plane(c, s));
        }
        RC(fold_prepare(c, PGH_GEOMETRIC_MEDIAN, (int64_t)inc.size(), s));
        FinalArgs fa;
        fa.ckpt = c->nz.get();
        fa.out = g.d_negv.as<float>();
        fa.divisor = W;
        fa.off = 0;
        fa.len = c->pg;
        fa.plain = true;
        RC(fold_listed(c, PGH_GEOMETRIC_MEDIAN, inc.data(), inc.size(), true, fa, s));
        RC(c->rowsums.run_listed(c, ROW_DISTSQ, inc, g.d_negv.as<float>(), s, D.data()));
    }
    g.W = W;
    g.inc.n_rows = n;
    g.inc.n_excluded = n - (int64_t)inc.size();
    g.inc.max_weight = mx;
    g.objective = obj;
    return PGH_OK;
}

// ---- trust-bootstrapped FedAvg: the planes and the weights --------------------------------------------------------

// a float [pvec] plane of the trust rule at the context's present length, zeroed when it is (re)allocated
int trust_plane(pgh_ctx* c, DeviceBuf* d, hipStream_t s) {
    if (*d && c->trust.pvec == c->pvec) return PGH_OK;
    if (c->trust.pvec != c->pvec) {  // (both planes are of one length)
        c->trust.d_root.reset();
        c->trust.d_point.reset();
        c->trust.pvec = c->pvec;
    }
    if (!d->reserve(4 * (size_t)c->pvec)) return fail(c, PGH_E_OOM, "allocation of a trust plane (%zu bytes) failed", 4 * (size_t)c->pvec);
    CK(c, hipMemsetAsync(d->as<void>(), 0, 4 * (size_t)c->pvec, s));
    return PGH_OK;
}

// The weights of a close over slots[0, n) in fold order (the included rows into trust.inc, their weights into
// the context's): K7 for the sums still missing, K14 for the included rows' dots still missing, the host step.
// PGH_E_STATE with no row included or none trusted; no fold is launched then.
int trust_slot_weights(pgh_ctx* c, const int32_t* slots, int n) {
    TrustState& t = c->trust;
    c->fw.stale();  // (the context's weights become this rule's, whatever happens below)
    std::vector<int32_t> inc;
    std::vector<double> ss;
    RC(finite_rows(c, slots, n, &inc, &ss));
    if (inc.empty()) return fail(c, PGH_E_STATE, "trusted mean: none of the %d diffs is finite", n);
    const int64_t ni = (int64_t)inc.size();
    RC(queue_dots(c, inc.data(), (int)ni));
    RC(c->rowsums.wait(c));
    std::vector<double> dot((size_t)ni);
    for (int64_t k = 0; k < ni; ++k) dot[(size_t)k] = c->rowsums.dot_at(inc[(size_t)k]);
    // the host step over the included rows alone: it includes every one of them (pos = 0 .. ni - 1)
    std::vector<float> w((size_t)ni);
    std::vector<int32_t> pos((size_t)ni);
    int64_t n_pos = 0, nt = 0;
    double T = 0.0;
    float mx = 0.f;
    const int rc = trust_weights(t.s0, ss.data(), dot.data(), ni, w.data(), pos.data(), &n_pos, &T, &nt, &mx);
    t.inc.n_rows = n;
    t.inc.n_excluded = n - ni;
    t.inc.max_weight = mx;
    t.inc.rows = inc;
    t.n_trusted = nt;
    t.total_trust = T;
    if (rc == -3) return fail(c, PGH_E_STATE, "trusted mean: none of the %lld finite diffs points along the root (T = 0)", (long long)ni);
    if (rc != 0) return fail(c, PGH_E_STATE, "trusted mean: the host step refused the sums (%d)", rc);
    c->fw.replace(FoldWeights::TRUST) = w;
    return PGH_OK;
}
}  // namespace

// ---- the fold plans: what the drivers ask before their launches ------------------------------------------------

int rules_slot_plan(pgh_ctx* c, int mode, const int32_t* slots, int n, int64_t c0, FoldPlan* p) {
    *p = FoldPlan{slots, n, c0 + n};
    if (mode == PGH_CLIPPED_MEAN) {  // a scale needs the whole row of the last report
        p->whole_rows = true;
        if (n == 0) return PGH_OK;
        if (c0 == 0) c->clip.norms.clear();
        return clip_set_scales(c, slots, n, c0, &c->clip.norms);  // scales and norms at fold index c0
    }
    if (mode == PGH_GEOMETRIC_MEDIAN) {
        RC(geomed_slot_weights(c, slots, n));
        included_plan(p, c->geo.inc, c->geo.W);
    }
    if (mode == PGH_TRUSTED_MEAN) {  // the weights carry the normalisation
        RC(trust_slot_weights(c, slots, n));
        included_plan(p, c->trust.inc, 1.0f);
    }
    return PGH_OK;
}

int rules_resident_plan(pgh_ctx* c, int mode, int64_t c0, int64_t n, FoldPlan* p) {
    *p = FoldPlan{nullptr, (int)n, c0 + n};
    // (resident only, check_mode_use: clients [0, n) -- their scales become the fold's weights)
    if (mode == PGH_CLIPPED_MEAN) {
        p->whole_rows = true;
        return resident_clip_scales(c, n);
    }
    if (mode == PGH_GEOMETRIC_MEDIAN) {
        RC(resident_weights(c, FoldWeights::GEOMED, c->geo.inc, n, geomed_slot_weights));
        included_plan(p, c->geo.inc, c->geo.W);
    }
    if (mode == PGH_TRUSTED_MEAN) {
        RC(resident_weights(c, FoldWeights::TRUST, c->trust.inc, n, trust_slot_weights));
        included_plan(p, c->trust.inc, 1.0f);
    }
    return PGH_OK;
}

int trim_divisor(pgh_ctx* c, int64_t n, float* div) {  // b dropped per side; at least one value must be left
    if (n < 2 * (int64_t)c->trim.b + 1)
        return fail(c, PGH_E_STATE, "trimmed mean with b = %d needs at least %d diffs, have %lld", c->trim.b,
                    2 * c->trim.b + 1, (long long)n);
    *div = (float)(n - 2 * (int64_t)c->trim.b);
    return PGH_OK;
}

// ---- Gaussian noise on the clipped close: the planes and K11 behind a FINAL launch ---------------------------

int noise_plane(pgh_ctx* c) {
    if (c->noise.d_d || c->noise.d_d.reserve(4 * (size_t)c->pvec)) return PGH_OK;
    return fail(c, PGH_E_OOM, "allocation of the noise planes (%zu bytes each) failed", 4 * (size_t)c->pvec);
}

int dp_noise_launch(pgh_ctx* c, const FinalArgs& fa, int64_t n, bool into_opt, hipStream_t s) {
    NoiseState& ns = c->noise;
    if (n <= 0) return fail(c, PGH_E_STATE, "a noised close of no diffs");
    pgh::DpNoiseArgs o{};
    float* d = (into_opt ? c->opt.d_d : ns.d_d).as<float>() + fa.off;
    o.d = d;
    o.ckpt = into_opt ? nullptr : fa.ckpt + fa.off;
    o.out = into_opt ? d : fa.out + fa.off;
    o.p = fa.len;
    o.i0 = c->lo + fa.off;
    o.key = ns.key;
    o.round = ns.round;
    o.sigma = dp_sigma(ns.z, c->clip.c, n);
    // HBM bytes: d in and out again (ahead of K10), or d and ckpt in and out out
    RC(timed_launch(c, s, (into_opt ? 8ull : 12ull) * (uint64_t)fa.len, [&] { return pgh::launch_dp_noise(o, s); }));
    ns.sigma_last = o.sigma;
    ns.n_last = n;
    return PGH_OK;
}

}  // namespace pgh_detail

namespace {
int check_clip_ctx(pgh_ctx* c, const char* what) {
    if (!c) return fail(nullptr, PGH_E_ARG, "null context");
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "%s: a group's shards each hold part of a row (the sums would need an all-reduce)", what);
    if (!c->layout) return fail(c, PGH_E_STATE, "pgh_set_layout has not been called");
    if (c->pg != c->P) return fail(c, PGH_E_UNSUPPORTED, "%s: the shard [%lld,%lld) is narrower than the model", what, (long long)c->lo, (long long)c->hi);
    if (c->d_slab && c->dtype != PGH_F32) return fail(c, PGH_E_UNSUPPORTED, "%s: the slab holds int64 shares", what);
    if (c->streaming) return fail(c, PGH_E_UNSUPPORTED, "%s: the context is streaming", what);
    return PGH_OK;
}
}  // namespace

int pgh_set_clip_norm(pgh_ctx* c, float bound) {
    if (!c) return PGH_E_ARG;
    if (bound == 0.f) {  // off: always possible (a group never clips)
        c->clip.c = 0.f;
        c->fw.stale(FoldWeights::CLIP);
        return PGH_OK;
    }
    RC(check_clip_ctx(c, "pgh_set_clip_norm"));
    if (!(bound > 0.f) || !std::isfinite(bound)) return fail(c, PGH_E_ARG, "the clipping bound must be finite and > 0, or 0 for off");
    if (bound != c->clip.c) c->fw.stale(FoldWeights::CLIP);
    c->clip.c = bound;
    return PGH_OK;
}

int pgh_set_trim(pgh_ctx* c, int b) {
    if (!c) return PGH_E_ARG;
    if (b < 0 || b > PGH_TRIM_MAX) return fail(c, PGH_E_ARG, "trim count %d outside [0,%d]", b, PGH_TRIM_MAX);
    if (c->grp) return pgh_group_api::set_trim(c, b);
    if (b != c->trim.b && c->folded > 0 && !c->streaming)
        return fail(c, PGH_E_STATE, "trim count changed from %d to %d with %lld diffs of the cycle folded", c->trim.b, b,
                    (long long)c->folded);
    c->trim.b = b;
    return PGH_OK;
}

int pgh_row_sumsq(pgh_ctx* c, const int32_t* slots, int n, double* out) {
    if (c && c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_row_sumsq: a group's shards each hold part of a row");
    RC(check_dtype(c, PGH_F32));
    if (c->streaming) return fail(c, PGH_E_UNSUPPORTED, "pgh_row_sumsq: the context is streaming");
    if (n < 0 || (n > 0 && !slots)) return fail(c, PGH_E_ARG, "bad slot list (n=%d)", n);
    RC(check_slot_list(c, slots, n, false));
    DeviceGuard g(c->device);
    RC(queue_sums(c, slots, n));
    if (!out) return PGH_OK;
    RC(c->rowsums.wait(c));
    for (int k = 0; k < n; ++k) out[k] = c->rowsums.at(slots[k]);
    return PGH_OK;
}

// ---- geometric-median FedAvg: the setting, K12 alone, what the last close saw ---------------------------------

int pgh_set_geomed(pgh_ctx* c, int iters, float nu) {
    if (!c) return PGH_E_ARG;
    if (iters == 0) {  // off: always possible
        c->geo.iters = 0;
        c->fw.stale(FoldWeights::GEOMED);
        return PGH_OK;
    }
    RC(check_clip_ctx(c, "pgh_set_geomed"));
    if (iters < 0 || iters > PGH_GEOMED_MAX_ITERS) return fail(c, PGH_E_ARG, "geometric median: %d iterations outside [0,%d]", iters, PGH_GEOMED_MAX_ITERS);
    if (!(nu > 0.f) || !std::isfinite(nu)) return fail(c, PGH_E_ARG, "geometric median: the smoothing must be finite and > 0");
    if (iters != c->geo.iters || nu != c->geo.nu) c->fw.stale(FoldWeights::GEOMED);
    c->geo.iters = iters;
    c->geo.nu = nu;
    return PGH_OK;
}

namespace {
// pgh_row_distsq and pgh_row_dot: `op` over the listed slots against the caller's point, which goes -- negated
// for K12, which adds -v -- into the plane that ensure_plane allocates and hands back.
int row_op_against_point(pgh_ctx* c, const char* who, const RowOp& op, bool negate, int (*ensure_plane)(pgh_ctx*, hipStream_t, float**),
                         const int32_t* slots, int n, const float* point, double* out) {
    RC(check_clip_ctx(c, who));
    RC(check_dtype(c, PGH_F32));
    if (n < 0 || (n > 0 && (!slots || !point || !out))) return fail(c, PGH_E_ARG, "bad slot list, point or out (n=%d)", n);
    RC(check_slot_list(c, slots, n, false));
    if (n == 0) return PGH_OK;
    DeviceGuard g(c->device);
    const hipStream_t s = c->stream;
    RC(order_after_ingest(c, s));
    float* plane = nullptr;
    RC(ensure_plane(c, s, &plane));
    std::vector<float> neg;
    if (negate) {
        neg.resize((size_t)c->pg);
        for (int64_t i = 0; i < c->pg; ++i) neg[(size_t)i] = -point[i];
    }
    CK(c, hipMemcpyAsync(plane, negate ? neg.data() : point, 4 * (size_t)c->pg, hipMemcpyHostToDevice, s));
    CK(c, hipStreamSynchronize(s));  // neg is pageable and the caller's bytes are free on return: the copy has left them
    return c->rowsums.run_listed(c, op, std::vector<int32_t>(slots, slots + n), plane, s, out);
}
}  // namespace

int pgh_row_distsq(pgh_ctx* c, const int32_t* slots, int n, const float* point, double* out) {
    return row_op_against_point(c, "pgh_row_distsq", ROW_DISTSQ, true, [](pgh_ctx* c, hipStream_t s, float** plane) {
        RC(geomed_plane(c, s));
        *plane = c->geo.d_negv.as<float>();
        return (int)PGH_OK;
    }, slots, n, point, out);
}

int pgh_geomed_stats(pgh_ctx* c, int* iters, int64_t* n_rows, int64_t* n_excluded, double* objective, float* max_weight) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_geomed_stats: group contexts take no geometric median");
    if (iters) *iters = c->geo.iters;
    if (n_rows) *n_rows = c->geo.inc.n_rows;
    if (n_excluded) *n_excluded = c->geo.inc.n_excluded;
    if (objective) *objective = c->geo.objective;
    if (max_weight) *max_weight = c->geo.inc.max_weight;
    return PGH_OK;
}

// ---- trust-bootstrapped FedAvg: the setting, the root, K14 alone, the host step alone, what the last close saw ----

int pgh_set_trust(pgh_ctx* c, int on) {
    if (!c) return PGH_E_ARG;
    if (!on) {  // off: always possible (the planes stay for the next trusted cycle of this shard)
        if (c->grp) return PGH_OK;
        c->trust.on = false;
        c->trust.forget();
        c->rowsums.dots_stale();
        c->fw.stale(FoldWeights::TRUST);
        return PGH_OK;
    }
    RC(check_clip_ctx(c, "pgh_set_trust"));
    c->trust.on = true;
    return PGH_OK;
}

int pgh_trust_root(pgh_ctx* c, const float* root, size_t nbytes) {
    RC(check_clip_ctx(c, "pgh_trust_root"));
    if (!c->trust.on) return fail(c, PGH_E_STATE, "pgh_trust_root: the rule is off, call pgh_set_trust first");
    if (!root || nbytes != 4 * (size_t)c->P) return fail(c, PGH_E_ARG, "pgh_trust_root: the root must be %lld floats (%zu bytes given)", (long long)c->P, nbytes);
    TrustState& t = c->trust;
    // whatever happens below, the old root is gone: its dots and weights with it
    t.root_valid = false;
    c->rowsums.dots_stale();
    c->fw.stale(FoldWeights::TRUST);
    const double s0 = row_dot_host(root, root, c->P);
    if (!(std::isfinite(s0) && s0 > 0.0))
        return fail(c, PGH_E_ARG, "pgh_trust_root: the root's sum of squares is %g: it must be finite and > 0 (a NaN, an infinity or an all-zero root)", s0);
    DeviceGuard g(c->device);
    // the copy stream: every K14 that read the old root was issued there
    const hipStream_t s = c->copy;
    RC(trust_plane(c, &t.d_root, s));
    CK(c, hipMemcpyAsync(t.d_root.as<float>(), root, nbytes, hipMemcpyHostToDevice, s));
    CK(c, hipStreamSynchronize(s));  // the caller's bytes are free on return
    t.s0 = s0;
    t.root_valid = true;
    return PGH_OK;
}

int pgh_row_dot(pgh_ctx* c, const int32_t* slots, int n, const float* point, double* out) {
    return row_op_against_point(c, "pgh_row_dot", ROW_DOT, false, [](pgh_ctx* c, hipStream_t s, float** plane) {
        RC(trust_plane(c, &c->trust.d_point, s));
        *plane = c->trust.d_point.as<float>();
        return (int)PGH_OK;
    }, slots, n, point, out);
}

int pgh_trust_weights_host(double s0, const double* sumsq, const double* dot, int n, float* weights, int32_t* included,
                           int* n_included, double* total_trust) {
    if (n < 0 || (n > 0 && (!sumsq || !dot || !weights || !included)) || !n_included)
        return fail(nullptr, PGH_E_ARG, "pgh_trust_weights_host: bad arguments (n=%d)", n);
    int64_t ni = 0;
    double T = 0.0;
    const int rc = trust_weights(s0, sumsq, dot, n, weights, included, &ni, &T, nullptr, nullptr);
    if (rc == -1) return fail(nullptr, PGH_E_ARG, "trusted mean: the root's sum of squares must be finite and > 0");
    *n_included = (int)ni;
    if (total_trust) *total_trust = T;
    if (rc == -2) return fail(nullptr, PGH_E_STATE, "trusted mean: none of the %d diffs is finite", n);
    if (rc == -3) return fail(nullptr, PGH_E_STATE, "trusted mean: none of the %lld finite diffs points along the root (T = 0)", (long long)ni);
    return PGH_OK;
}

int pgh_trust_stats(pgh_ctx* c, int* on, int64_t* n_rows, int64_t* n_excluded, int64_t* n_trusted, double* total_trust, float* max_weight,
                    double* root_norm) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_trust_stats: group contexts take no trusted mean");
    if (on) *on = c->trust.on ? 1 : 0;
    if (n_rows) *n_rows = c->trust.inc.n_rows;
    if (n_excluded) *n_excluded = c->trust.inc.n_excluded;
    if (n_trusted) *n_trusted = c->trust.n_trusted;
    if (total_trust) *total_trust = c->trust.total_trust;
    if (max_weight) *max_weight = c->trust.inc.max_weight;
    if (root_norm) *root_norm = c->trust.root_valid ? std::sqrt(c->trust.s0) : 0.0;
    return PGH_OK;
}

// ---- Multi-Krum selection: K13 alone, the host step alone, the selection, what the last one saw ----------------

namespace {
int check_pair_list(pgh_ctx* c, const char* what, const int32_t* slots, int n, bool no_twice) {
    RC(check_clip_ctx(c, what));
    RC(check_dtype(c, PGH_F32));
    if (n < 0 || (n > 0 && !slots)) return fail(c, PGH_E_ARG, "%s: bad slot list (n=%d)", what, n);
    if (n > PGH_KRUM_MAX_ROWS) return fail(c, PGH_E_UNSUPPORTED, "%s: %d rows, at most %d", what, n, PGH_KRUM_MAX_ROWS);
    if (!no_twice) return check_slot_list(c, slots, n, false);  // (as pgh_row_distsq)
    std::vector<char> seen((size_t)c->slots, 0);  // the selection: an unoccupied slot is an argument error too
    for (int k = 0; k < n; ++k) {
        const int32_t sl = slots[k];
        if (sl < 0 || sl >= c->slots || c->slot_client[(size_t)sl] < 0 || seen[(size_t)sl])
            return fail(c, PGH_E_ARG, "%s: slot %d is outside [0,%d), holds no diff or is listed twice", what, sl, c->slots);
        seen[(size_t)sl] = 1;
    }
    return PGH_OK;
}
}  // namespace

int pgh_row_pairdist(pgh_ctx* c, const int32_t* slots, int n, double* out) {
    RC(check_pair_list(c, "pgh_row_pairdist", slots, n, false));
    if (n > 0 && !out) return fail(c, PGH_E_ARG, "pgh_row_pairdist: out is NULL");
    if (n == 0) return PGH_OK;
    DeviceGuard g(c->device);
    const hipStream_t s = c->stream;
    RC(order_after_ingest(c, s));
    return c->rowsums.pairdist(c, slots, n, s, out);
}

int pgh_krum_select_host(const double* dist, int n, int f, int m, int32_t* picked, int* n_picked, double* scores) {
    if (n < 0 || f < 0 || m < 0 || (n > 0 && !dist) || !picked || !n_picked)
        return fail(nullptr, PGH_E_ARG, "pgh_krum_select_host: bad arguments (n=%d, f=%d, m=%d)", n, f, m);
    const int rc = krum_select(dist, n, f, m, picked, n_picked, scores);
    if (rc == -1) return fail(nullptr, PGH_E_ARG, "Multi-Krum: a distance is NaN or negative");
    if (rc == -3) return fail(nullptr, PGH_E_STATE, "Multi-Krum with f = %d, m = %d over %d rows: it needs at least 2f + 3 = %d rows and m <= n - f", f, m, n, 2 * f + 3);
    return PGH_OK;
}

int pgh_krum_select(pgh_ctx* c, const int32_t* slots, int n, int f, int m, int32_t* picked, int* n_picked) {
    RC(check_pair_list(c, "pgh_krum_select", slots, n, true));
    if (f < 0 || m < 0 || !picked || !n_picked) return fail(c, PGH_E_ARG, "pgh_krum_select: bad arguments (f=%d, m=%d)", f, m);
    DeviceGuard g(c->device);
    std::vector<int32_t> inc;
    RC(finite_rows(c, slots, n, &inc, nullptr));
    const int ni = (int)inc.size();
    if ((int64_t)ni < 2 * (int64_t)f + 3 || m > ni - f)  // (nothing is launched)
        return fail(c, PGH_E_STATE, "Multi-Krum with f = %d, m = %d: %d of the %d diffs are finite, it needs at least 2f + 3 = %d and m <= n' - f", f, m, ni, n, 2 * f + 3);
    const hipStream_t s = c->stream;
    RC(order_after_ingest(c, s));
    std::vector<double> D((size_t)ni * (size_t)ni), sc((size_t)ni);
    RC(c->rowsums.pairdist(c, inc.data(), ni, s, D.data()));
    std::vector<int32_t> pos((size_t)ni);
    int np = 0;
    const int rc = krum_select(D.data(), ni, f, m, pos.data(), &np, sc.data());
    if (rc != 0) return fail(c, rc == -1 ? PGH_E_HIP : PGH_E_STATE, "Multi-Krum: the host step refused the distances (%d)", rc);
    KrumState& ks = c->krum;
    ks = KrumState{n, n - ni, np, 0.0, INFINITY};
    std::vector<char> is((size_t)ni, 0);
    for (int k = 0; k < np; ++k) {
        picked[k] = inc[(size_t)pos[(size_t)k]];
        is[(size_t)pos[(size_t)k]] = 1;
        ks.max_picked_score = k == 0 ? sc[(size_t)pos[0]] : std::max(ks.max_picked_score, sc[(size_t)pos[(size_t)k]]);
    }
    for (int k = 0; k < ni; ++k)
        if (!is[(size_t)k]) ks.min_dropped_score = std::min(ks.min_dropped_score, sc[(size_t)k]);
    *n_picked = np;
    return PGH_OK;
}

int pgh_krum_stats(pgh_ctx* c, int64_t* n_rows, int64_t* n_excluded, int64_t* n_picked, double* max_picked_score, double* min_dropped_score) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_krum_stats: group contexts select nothing");
    if (n_rows) *n_rows = c->krum.n_rows;
    if (n_excluded) *n_excluded = c->krum.n_excluded;
    if (n_picked) *n_picked = c->krum.n_picked;
    if (max_picked_score) *max_picked_score = c->krum.max_picked_score;
    if (min_dropped_score) *min_dropped_score = c->krum.min_dropped_score;
    return PGH_OK;
}

int pgh_clip_scale(double sumsq, float bound, float* scale) {
    if (!scale) return fail(nullptr, PGH_E_ARG, "scale is NULL");
    if (!(bound > 0.f) || !std::isfinite(bound)) return fail(nullptr, PGH_E_ARG, "the clipping bound must be finite and > 0");
    *scale = clip_scale_of(sumsq, bound);
    return PGH_OK;
}

int pgh_clip_stats(pgh_ctx* c, int64_t* n_rows, int64_t* n_clipped, double* max_norm) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_clip_stats: group contexts do not clip");
    // the finished folds, and the slot folds of the running cycle on top
    ClipState& cl = c->clip;
    const int64_t rows0 = cl.rows, cl0 = cl.clipped;
    const double mx0 = cl.max_norm;
    cl.count_cycle(c->fw.v);
    if (n_rows) *n_rows = cl.rows;
    if (n_clipped) *n_clipped = cl.clipped;
    if (max_norm) *max_norm = cl.max_norm;
    cl.rows = rows0;
    cl.clipped = cl0;
    cl.max_norm = mx0;
    return PGH_OK;
}

// ---- Gaussian noise on the clipped close: the setting, the sampler alone, what the last close used ----------

int pgh_set_dp_noise(pgh_ctx* c, float z, uint64_t key, uint32_t round) {
    if (!c) return PGH_E_ARG;
    if (z == 0.f) {  // off: always possible (the planes stay for the next noised cycle of this shard)
        c->noise.z = 0.f;
        return PGH_OK;
    }
    if (!(z > 0.f) || !std::isfinite(z)) return fail(c, PGH_E_ARG, "the noise multiplier must be finite and > 0, or 0 for off");
    RC(check_clip_ctx(c, "pgh_set_dp_noise"));
    c->noise.z = z;
    c->noise.key = key;
    c->noise.round = round;
    c->noise.pvec = c->pvec;
    return PGH_OK;
}

int pgh_dp_normals(pgh_ctx* c, uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_dp_normals runs on one GPU: call it on pgh_group_child");
    if (i0 < 0 || n < 0 || i0 > INT64_MAX - n || (n > 0 && !out)) return fail(c, PGH_E_ARG, "bad index range [%lld,+%lld)", (long long)i0, (long long)n);
    if (n == 0) return PGH_OK;
    DeviceGuard g(c->device);
    DeviceBuf d;
    if (!d.reserve(8 * (size_t)n)) return fail(c, PGH_E_OOM, "allocation of %lld normals failed", (long long)n);
    const hipError_t e = pgh::launch_dp_normals(key, round, i0, n, d.as<double>(), c->stream);
    if (e != hipSuccess) return fail(c, PGH_E_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    CK(c, hipMemcpyAsync(out, d.as<double>(), 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));  // d is freed on return
    return PGH_OK;
}

int pgh_dp_normals_host(uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out) {
    if (i0 < 0 || n < 0 || i0 > INT64_MAX - n || (n > 0 && !out)) return fail(nullptr, PGH_E_ARG, "bad index range [%lld,+%lld)", (long long)i0, (long long)n);
    dp_normals(key, round, i0, n, out);
    return PGH_OK;
}

int pgh_dp_stats(pgh_ctx* c, float* z, double* sigma_last, int64_t* n_last) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_dp_stats: group contexts add no noise");
    if (z) *z = c->noise.z;
    if (sigma_last) *sigma_last = c->noise.sigma_last;
    if (n_last) *n_last = c->noise.n_last;
    return PGH_OK;
}
