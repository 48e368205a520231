// libpygrid_hip: report-time folds of scattered slots -- the certain prefix of the close-time order
// folded as its diffs arrive, in any slot.  Reference: submit_worker_diff (cycle_manager.py:151-178)
// feeding _average_plan_diffs (:219-323).  (struct pgh_ctx and the shared helpers: pgh_ctx.h)
#include "pgh_ctx.h"

using namespace pgh_detail;

// (the public entry points take their C linkage from include/pgh_api.h)

// ---- report-time folds of scattered slots (pgh_fold_slots) -------------------------------------

namespace {
int slot_fold(pgh_ctx* c, int mode, const int32_t* slots, int n, bool final) {
    RC(check_dtype(c, PGH_F32));
    if (c->streaming) return fail(c, PGH_E_STATE, "context is streaming: slot folds need a RESIDENT slab");
    if (n < 0 || (n > 0 && !slots)) return fail(c, PGH_E_ARG, "bad slot list (n=%d)", n);
    if (c->slot_mode >= 0 && c->slot_mode != mode)
        return fail(c, PGH_E_STATE, "averaging mode changed from %d to %d within a cycle", c->slot_mode, mode);
    RC(check_slot_list(c, slots, n, true));
    // a median takes every row of the cycle in this one call, a geometric median's weights need them (check_mode_use: final)
    const char* const one_fold = rules_one_fold_cycle(mode);
    if (one_fold && c->folded > 0)
        return fail(c, PGH_E_STATE, "%s closes a cycle without earlier slot folds (%lld diffs folded)", one_fold, (long long)c->folded);
    const bool median = mode == PGH_MEDIAN;
    const int64_t c0 = c->folded, total = c0 + n;
    FinalArgs fa;
    fa.ckpt = c->d_ckpt.as<float>();
    fa.out = c->d_out.as<float>();
    if (final) {
        RC(check_ckpt(c, "pgh_fold_slots_finish_resident"));
        if (total == 0) return fail(c, PGH_E_STATE, "no diffs folded");
        RC(fedavg_divisor(c, mode, total, &fa.divisor));
    } else if (n == 0) {
        return PGH_OK;
    }
    DeviceGuard g(c->device);
    const hipStream_t s = c->stream;
    // a close right behind a ranged ingest (pgh_set_ingest_ranges) orders each FINAL range after the
    // chunk of the last report it reads instead of after the whole copy stream
    // (never where a rule needs the last report's whole row, a scale for one: it takes the whole-stream wait)
    const bool may_range = final && n > 0 && n <= pgh::ROWTAB_MAX && c->pg >= (1 << 20) && c->ranged.valid(c->pg);
    // the rule's part: a clipped fold's scales in fold order, a geometric median's included rows with their
    // final weights and divisor -- the fold below runs over the plan's rows, fold client k = the k-th of them
    const int32_t* const all_slots = slots;
    const int n_all = n;
    FoldPlan plan;
    RC(rules_slot_plan(c, mode, slots, n, c0, &plan));
    slots = plan.slots;
    n = plan.n;
    if (plan.has_divisor) fa.divisor = plan.divisor;
    const bool ranged = may_range && !plan.whole_rows;
    if (!ranged) RC(order_after_ingest(c, s));
    else if (hipEvent_t dec = c->vdec.last_decode()) CK(c, hipStreamWaitEvent(s, dec, 0));  // the copy stream: per range below
    if (n > 0) RC(fold_prepare(c, mode, plan.total, s));
    if (median && n > pgh::ROWTAB_MAX) RC(median_row_table(c, slots, n, s));  // more rows than a RowTab carries
    int done = 0;
    bool prequeued = false;
    do {
        const int m = median ? n : std::min(n - done, pgh::ROWTAB_MAX);
        pgh::RowTab tab;
        for (int k = 0; k < std::min(m, pgh::ROWTAB_MAX); ++k) tab.rows[k] = slots[done + k] * c->parties;
        const bool first = (c0 + done == 0), last = (done + m == n);
        const int flags = (first ? pgh::FL_FIRST : 0) | (final && last ? pgh::FL_FINAL : 0);
        // (only a median comes with more rows than the table carries: they are in the device table then)
        FoldRows rows{c->d_slab.as<float>(), m};
        if (m <= pgh::ROWTAB_MAX) rows.src.tab = &tab;
        else rows.src.d_rows = median_rows(c);
        // The FINAL pass of a report-time close (a short fold of the rows left) as ranges of 4 MiB of
        // output, one after another on one stream, a mark behind every second one: each 8 MiB D2H
        // piece starts behind the two ranges that wrote it instead of behind the whole fold.  Ranges
        // aligned to the pieces on one stream closed 0.1-0.15 ms sooner than 8 equal ranges
        // alternating over two streams (profiles/r04m/: 2.04 vs 2.19 ms, close start -> new
        // checkpoint bytes); a mark (a system-scope release) only where a piece ends (r05).
        const int64_t RF = (int64_t)(D2H_PIECE / 8);
        const int K = (flags & pgh::FL_FINAL) && c->pg >= (1 << 20) ? (int)((c->pg + RF - 1) / RF) : 1;
        if (flags & pgh::FL_FINAL) clear_final_marks(c);
        // the new checkpoint's D2H starts here: after each mark, the pieces whose ranges have
        // finished go out while the later ranges are still being issued (stage_d2h_pieces adopts the
        // ring).  The result is d_out until the swap below.
        D2HRing& pre = c->d2h.pre;
        bool prequeue = false;
        if (K > 1 && (flags & pgh::FL_FINAL)) {
            RC(d2h_ring_begin(c, &pre, c->d_out.as<uint8_t>(), 4 * (size_t)c->pg, s, true, false));
            prequeue = pre.base || pre.n_free > 0;  // own cells, or a free staging slot
        }
        for (int r = 0; r < K; ++r) {
            const hipStream_t rs = s;
            const int64_t lo = std::min(c->pg, RF * r), hi = K == 1 ? c->pg : std::min(c->pg, RF * (r + 1));
            if (ranged && K > 1) RC(c->ranged.wait_range(c, rs, lo, hi));  // every chunk this range reads has landed ...
            else if (ranged && r == 0) RC(c->ranged.wait_all(c, rs));     // ... or all of it
            fa.off = lo;
            fa.len = hi - lo;
            RC(fold_launch(c, mode, rows, c0 + done, flags, fa, rs));
            if (K > 1 && (hi % (2 * RF) == 0 || hi == c->pg)) {
                RC(add_final_mark(c, rs, hi));
                if (prequeue) RC(c->d2h.issue_pre(c));
            }
        }
        prequeued = prequeued || prequeue;
        done += m;
    } while (done < n);
    RC(record_fold(c, c->fold_evs, s));
    RC(record_slot_fold(c, all_slots, n_all));
    for (int k = 0; k < n_all; ++k) c->slot_client[(size_t)all_slots[k]] = -1;  // free for the next ingests
    c->folded = total;
    c->st.n_folded = total;
    c->slot_mode = mode;
    if (final) {
        std::swap(c->d_ckpt, c->d_out);  // the new checkpoint is the next cycle's input
        c->d2h.keep_pre(prequeued, c->d_ckpt.as<uint8_t>());
        c->folded = 0;  // the next cycle folds from scratch
        c->slot_mode = -1;
        rules_cycle_finished(c, mode);
    }
    return PGH_OK;
}
}  // namespace

int pgh_fold_slots(pgh_ctx* c, int mode, const int32_t* slots, int n) {
    if (c) RC(check_mode_use(c, mode, USE_SLOT_EARLY));
    if (c && c->grp) return pgh_group_api::fold_slots(c, mode, slots, n, false);
    if (!c) return PGH_E_ARG;
    return slot_fold(c, mode, slots, n, false);
}

int pgh_fold_slots_finish_resident(pgh_ctx* c, int mode, const int32_t* slots, int n) {
    if (c) RC(check_mode_use(c, mode, USE_SLOT_FINAL));
    if (c && c->grp) return pgh_group_api::fold_slots(c, mode, slots, n, true);
    if (!c) return PGH_E_ARG;
    const double t0 = now_ms();
    RC(slot_fold(c, mode, slots, n, true));
    c->st.close_ms_last = now_ms() - t0;
    return PGH_OK;
}

namespace {
int check_slot_folds(pgh_ctx* c) {
    RC(check_dtype(c, PGH_F32));
    if (c->streaming) return fail(c, PGH_E_STATE, "context is streaming: slot folds need a RESIDENT slab");
    return PGH_OK;
}
}  // namespace

int pgh_fold_slots_restart(pgh_ctx* c) {
    if (c && c->grp) return pgh_group_api::fold_restart(c);
    if (!c) return PGH_E_ARG;
    RC(check_slot_folds(c));
    // The next slot fold's FL_FIRST pass overwrites the fold state on c->stream, behind any fold
    // still in flight there: nothing to wait for.
    c->folded = 0;
    c->st.n_folded = 0;
    c->slot_mode = -1;
    c->fw.clear();  // (a clipped cycle's scales among them)
    rules_folds_restarted(c);
    return PGH_OK;
}
