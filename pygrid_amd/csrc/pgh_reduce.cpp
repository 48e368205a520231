// libpygrid_hip: the one fp32 fold launch (fold_prepare, fold_launch), fold_run and its bookkeeping, the
// divisors, RESIDENT folds (every ingested client in one launch, repeatable), the resident checkpoint kept in
// HBM across cycles, secure aggregation (Z_2^64 share sum + fixed-point decode) and STREAM folds (a ring of
// slots folded in client order while ingest continues).  What the rules add to the fold: pgh_rules.cpp; the
// server optimizer behind a FINAL launch: pgh_serveropt.cpp.  Reference:
// cycle_manager.py:252-296 (fedavg), test_basic_syft_operations.py:417-424 (secagg).
// (struct pgh_ctx and the shared helpers: pgh_ctx.h)
#include "pgh_ctx.h"

using namespace pgh_detail;

// (the public entry points take their C linkage from include/pgh_api.h)

// ---- the fold itself, its weights and divisors, the STREAM / RESIDENT bookkeeping -------------------

namespace pgh_detail {

int FoldWeights::upload(pgh_ctx* c, hipStream_t s) {
    if (on_device || v.empty()) return PGH_OK;
    if (!d.reserve(sizeof(float) * v.size())) return fail(c, PGH_E_OOM, "weight vector allocation failed");
    CK(c, hipMemcpyAsync(d.as<float>(), v.data(), sizeof(float) * v.size(), hipMemcpyHostToDevice, s));
    CK(c, hipStreamSynchronize(s));  // v may change after return
    on_device = true;
    return PGH_OK;
}

// Reciprocal table covering clients [0, n) for the iterative fold's division (div_by_count in
// pgh_kernels.hip).  Grows geometrically; the upload is ordered before stream `s`'s next fold.
static int ensure_recips(pgh_ctx* c, int64_t n, hipStream_t s) {
    const int64_t have = (int64_t)(c->d_rec.cap() / sizeof(double));
    if (n <= have) return PGH_OK;
    const int64_t cap = std::max<int64_t>({n, 2 * have, 4096});
    std::vector<double> h((size_t)cap);
    for (int64_t k = 0; k < cap; ++k) h[(size_t)k] = 1.0 / (double)(float)(k + 1);  // y as the plan sees it
    pgh_ctx::DeviceBuf d;
    if (!d.reserve(sizeof(double) * (size_t)cap)) return fail(c, PGH_E_OOM, "reciprocal table allocation failed");
    CK(c, hipMemcpyAsync(d.as<void>(), h.data(), sizeof(double) * (size_t)cap, hipMemcpyHostToDevice, s));
    CK(c, hipStreamSynchronize(s));  // h is freed on return
    std::swap(c->d_rec, d);
    if (d) c->rec_old.push_back(std::move(d));  // an in-flight fold may read it: kept until pgh_destroy
    return PGH_OK;
}

int fixed_point_divisor(pgh_ctx* c, int base, int prec, float* div) {
    if (base < 2 || prec < 0 || prec > 18) return fail(c, PGH_E_ARG, "bad fixed-point base %d / precision %d", base, prec);
    long double scale = 1;
    for (int k = 0; k < prec; ++k) scale *= base;
    if (scale > 9.2e18L) return fail(c, PGH_E_ARG, "base**prec overflows int64");
    *div = (float)(int64_t)scale;  // python int base**prec, promoted to float32 by the division
    return PGH_OK;
}

float weight_total(const std::vector<float>& w, int64_t n) {  // left fold, float32
    float t = w[0];
    for (int64_t k = 1; k < n; ++k) t = t + w[k];
    return t;
}

int fold_prepare(pgh_ctx* c, int mode, int64_t total, hipStream_t s) {
    if (kernel_mode(mode) == PGH_WEIGHTED_MEAN) {
        if ((int64_t)c->fw.v.size() < total)
            return fail(c, PGH_E_STATE, "weighted mean: %zu weights for %lld clients", c->fw.v.size(), (long long)total);
        RC(c->fw.upload(c, s));
    }
    if (mode == PGH_ITERATIVE_MEAN) RC(ensure_recips(c, total, s));
    return PGH_OK;
}

int fold_launch(pgh_ctx* c, int mode, const FoldRows& rows, int64_t client0, int flags, const FinalArgs& fa, hipStream_t s) {
    const int64_t off = fa.off;
    pgh::FedavgArgs a{};
    a.diffs = rows.diffs;
    a.map = slab_map(c);
    a.map.off = off;
    a.n_rows = rows.n;
    a.client0 = client0;
    a.p = fa.len;
    a.weights = c->fw.d ? c->fw.d.as<float>() + client0 : nullptr;
    a.recips = c->d_rec ? c->d_rec.as<double>() + client0 : nullptr;
    a.acc = c->d_acc.as<float>() + off;
    a.ckpt = fa.ckpt ? fa.ckpt + off : nullptr;
    a.out = fa.out ? fa.out + off : nullptr;
    // A server optimizer: the FINAL launch, unchanged, subtracts the average from -0 into the delta
    // plane, and K10 behind it on the same stream applies the step to the real ckpt / out.
    const bool opt = c->opt.kind != PGH_OPT_NONE && (flags & pgh::FL_FINAL) && !fa.plain;
    // Noise on the clipped close: a second tenant of that mechanism.  K11 follows the FINAL launch and noises
    // the delta plane in place ahead of K10, or, without an optimizer, reads planes of the noise state's
    // own and writes the real out.
    const bool noise = noise_on(c) && (flags & pgh::FL_FINAL) && !fa.plain;
    if (noise) RC(check_noise_final(c, mode));  // (the entry points have checked: nothing was launched)
    if (noise && (!fa.ckpt || !fa.out)) return fail(c, PGH_E_ARG, "a noised FINAL fold needs ckpt and out");
    if (opt || noise) {  // (the lines that name the two tenants' delta planes: fold_launch's own)
        RC(c->nz.ensure(c, s));
        if (!opt) RC(noise_plane(c));
        a.ckpt = c->nz.get() + off;
        a.out = (opt ? c->opt.d_d : c->noise.d_d).as<float>() + off;
    }
    a.divisor = fa.divisor;
    a.flags = flags;
    a.mode = kernel_mode(mode);
    a.variant = c->variant;
    if (mode == PGH_MEDIAN) {  // (its own launches and bytes)
        RC(median_fold(c, a, rows.src, s));
        return opt ? server_opt_launch(c, fa, s) : PGH_OK;
    }
    // HBM bytes: the rows; the running state in unless FIRST; the state out, or ckpt in and out when FINAL
    const uint64_t pg = (uint64_t)fa.len;
    uint64_t bytes = 4ull * (uint64_t)rows.n * pg + ((flags & pgh::FL_FIRST) ? 0 : 4 * pg) +
                     ((flags & pgh::FL_FINAL) ? 8 * pg : 4 * pg);
    if (mode == PGH_TRIMMED_MEAN) {
        RC(trim_args(c, &a));
        bytes += trim_state_bytes(c, flags, pg);
    }
    RC(timed_launch(c, s, bytes, [&] { return pgh::launch_fedavg(a, rows.src, s); }));
    if (noise) RC(dp_noise_launch(c, fa, client0 + rows.n, opt, s));  // the FINAL launch ends the cycle's N rows
    return opt ? server_opt_launch(c, fa, s) : PGH_OK;
}

int fold_listed(pgh_ctx* c, int mode, const int32_t* slots, size_t n, bool final, const FinalArgs& fa, hipStream_t s) {
    return for_row_runs(c, slots, n, [&](const pgh::Rows& rows, size_t k0, size_t m) {
        const int flags = (k0 == 0 ? pgh::FL_FIRST : 0) | (final && k0 + m == n ? pgh::FL_FINAL : 0);
        FoldRows fr{rows.tab ? c->d_slab.as<float>() : (const float*)slot_row(c, slots[0], 0), (int)m, rows};
        fr.src.row0 = 0;  // (the fold takes contiguous rows from its slab pointer)
        return fold_launch(c, mode, fr, (int64_t)k0, flags, fa, s);
    });
}

// Fold slots holding clients [c0, c0 + n) (slot order may wrap) into the running state.
// FIRST when c0 == 0; FINAL writes out (fedavg: ckpt - avg; secagg: sum/dec) instead of the state.
int fold_run(pgh_ctx* c, int kind, int64_t c0, int64_t n, bool final, const FinalArgs& fa, hipStream_t s) {
    FoldPlan plan;  // a rule's weights, and the rows it folds where they are not all n
    RC(rules_resident_plan(c, kind, c0, n, &plan));
    RC(order_after_ingest(c, s));
    if (kind != KIND_SECAGG && n > 0) RC(fold_prepare(c, kind, plan.total, s));
    const int R = c->slots;
    FinalArgs r = fa;  // the launches' param range, its length resolved, and the rule's divisor
    if (plan.has_divisor) r.divisor = plan.divisor;
    if (r.len < 0) r.len = c->pg - r.off;
    const int64_t off = r.off, len = r.len;
    if (off < 0 || (off & 3) || len <= 0 || off + len > c->pg)
        return fail(c, PGH_E_ARG, "param range [%lld,+%lld) outside the shard or not 4-aligned", (long long)off,
                    (long long)len);
    int64_t done = 0;
    if (plan.slots) RC(fold_listed(c, kind, plan.slots, (size_t)plan.n, final, r, s));
    else do {
        const int slot = (int)((c0 + done) % R);
        const int64_t seg = std::min<int64_t>(n - done, (int64_t)(R - slot));
        const bool first = (c0 + done == 0);
        const bool last = (done + seg == n);
        const int flags = (first ? pgh::FL_FIRST : 0) | (final && last ? pgh::FL_FINAL : 0);
        if (kind == KIND_SECAGG) {
            const uint64_t pg = (uint64_t)len;
            pgh::SecaggArgs a{};
            a.shares = (const int64_t*)slot_row(c, slot, 0);
            a.map = slab_map(c);
            a.map.off = off;
            a.n_rows = (int)(seg * c->parties);
            a.p = len;
            a.acc = c->d_uacc.as<uint64_t>() + off;
            a.sum_out = fa.sum ? fa.sum + off : nullptr;
            a.dec_out = fa.dec ? fa.dec + off : nullptr;
            a.divisor = fa.divisor;
            a.flags = flags;
            a.variant = c->variant;
            const uint64_t bytes = 8ull * (uint64_t)a.n_rows * pg + (first ? 0 : 8 * pg) +
                                   ((flags & pgh::FL_FINAL) ? (fa.sum ? 8 * pg : 0) + (fa.dec ? 4 * pg : 0) : 8 * pg);
            RC(timed_launch(c, s, bytes, [&] { return pgh::launch_secagg(a, s); }));
        } else {
            RC(fold_launch(c, kind, FoldRows{(const float*)slot_row(c, slot, 0), (int)seg}, c0 + done, flags, r, s));
        }
        done += seg;
    } while (done < n);
    RC(record_fold(c, c->fold_evs, s));
    return record_fold(c, c->slab_evs, s);  // it read every slab row
}

// Length of the run of ingested clients starting at `from` (slot ring order).
int64_t ready_run(pgh_ctx* c, int64_t from) {
    int64_t n = 0;
    while (n < c->slots && c->slot_client[(size_t)((from + n) % c->slots)] == from + n) ++n;
    return n;
}

// Every ingested client must belong to the contiguous run starting at `from`.
int check_no_gaps(pgh_ctx* c, int64_t from, int64_t run) {
    for (int s = 0; s < c->slots; ++s) {
        const int64_t k = c->slot_client[(size_t)s];
        if (k >= 0 && (k < from || k >= from + run))
            return fail(c, PGH_E_STATE, "client %lld is missing but client %lld was ingested",
                        (long long)(from + run), (long long)k);
    }
    return PGH_OK;
}

// STREAM: fold the ready run when it reaches the batch size (or always, when forced).
int maybe_fold(pgh_ctx* c, bool force) {
    const int64_t run = ready_run(c, c->folded);
    if (run == 0 || (!force && run < c->fold_batch)) return PGH_OK;
    RC(fold_run(c, c->kind, c->folded, run, false, FinalArgs{}, c->stream));
    for (int64_t k = 0; k < run; ++k) c->slot_client[(size_t)((c->folded + k) % c->slots)] = -1;
    c->folded += run;
    c->st.n_folded = c->folded;
    return record_mark(c, c->stream, c->folded);
}

// Claim the slot for `client` (both modes) before bytes are written to it.
int claim_slot(pgh_ctx* c, int64_t client, int* slot_out) {
    if (client < 0) return fail(c, PGH_E_ARG, "negative client index");
    if (!c->streaming) {
        if (client >= c->slots)
            return fail(c, PGH_E_ARG, "client %lld outside slab capacity %d", (long long)client, c->slots);
        RC(order_slot_overwrite(c, (int)client));  // a fold issued earlier may still read the slot
        rules_slot_written(c, (int)client);
        *slot_out = (int)client;
        return PGH_OK;
    }
    if (client < c->folded) return fail(c, PGH_E_STATE, "client %lld was already folded", (long long)client);
    const int slot = (int)(client % c->slots);
    const int64_t held = c->slot_client[(size_t)slot];
    if (held >= 0 && held != client)
        return fail(c, PGH_E_STATE, "ring full: slot %d still holds unfolded client %lld (fold front %lld)", slot,
                    (long long)held, (long long)c->folded);
    RC(order_stream_overwrite(c, client));
    *slot_out = slot;
    return PGH_OK;
}

int mark_ingested(pgh_ctx* c, int64_t client, int slot) {
    if (c->slot_client[(size_t)slot] != client) c->st.n_clients += 1;
    c->slot_client[(size_t)slot] = client;
    return c->streaming ? maybe_fold(c, false) : PGH_OK;
}

// RESIDENT: clients [0, n) all present, nothing else.
int resident_count(pgh_ctx* c, int64_t* n_out) {
    if (c->streaming) return fail(c, PGH_E_STATE, "context is streaming: finish with pgh_stream_finish*");
    int64_t n = ready_run(c, 0);
    RC(check_no_gaps(c, 0, n));
    if (n == 0) return fail(c, PGH_E_STATE, "no diffs ingested");
    *n_out = n;
    return PGH_OK;
}

int fedavg_divisor(pgh_ctx* c, int mode, int64_t n, float* div) {
    if (mode == PGH_TRIMMED_MEAN) {
        RC(trim_divisor(c, n, div));
    } else if (mode == PGH_WEIGHTED_MEAN) {
        if ((int64_t)c->fw.v.size() < n)
            return fail(c, PGH_E_STATE, "weighted mean needs %lld weights, have %zu", (long long)n, c->fw.v.size());
        const float t = weight_total(c->fw.v, n);
        if (!(t != 0.f)) return fail(c, PGH_E_ARG, "sum of weights is zero");
        *div = t;
    } else {  // (a geometric median's comes with the plan that computed its weights)
        *div = (float)n;  // th.div(sum, len(diffs)), cycle_manager.py:288
    }
    return PGH_OK;
}

}  // namespace pgh_detail

// ---- RESIDENT reductions -------------------------------------------------------------------------

int pgh_fedavg_device(pgh_ctx* c, int mode, const float* d_ckpt, float* d_out, void* stream) {
    return pgh_fedavg_device_range(c, mode, 0, -1, d_ckpt, d_out, stream);  // the whole shard
}

int pgh_fedavg_device_range(pgh_ctx* c, int mode, int64_t off, int64_t len, const float* d_ckpt, float* d_out,
                            void* stream) {
    if (c && c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_fedavg_device* takes device pointers, which name one GPU: call it on pgh_group_child");
    RC(check_dtype(c, PGH_F32));
    RC(check_mode_use(c, mode, USE_RESIDENT));
    if (!d_ckpt || !d_out) return fail(c, PGH_E_ARG, "d_ckpt / d_out is NULL");
    if (((uintptr_t)d_ckpt | (uintptr_t)d_out) & 15) return fail(c, PGH_E_ARG, "device buffers must be 16-byte aligned");
    DeviceGuard g(c->device);
    int64_t n = 0;
    RC(resident_count(c, &n));
    FinalArgs fa;
    fa.ckpt = d_ckpt;
    fa.out = d_out;
    fa.off = off;
    fa.len = len;
    RC(fedavg_divisor(c, mode, n, &fa.divisor));
    return fold_run(c, mode, 0, n, true, fa, (hipStream_t)stream);
}

// New checkpoint bytes into d_ckpt (one host range, or the pieces of a State message): on the copy
// stream behind every fold that may still read it; the range marks of the last FINAL pass go with it.
static int upload_ckpt(pgh_ctx* c, const uint8_t* src, size_t n, bool pinned_src, const std::vector<Piece>* pieces = nullptr) {
    const Dest dst = vec_dest(c->d_ckpt.as<float>(), c->pvec, 4);
    RC(order_before_overwrite(c));
    c->ckpt_valid = false;
    clear_final_marks(c);
    RC(pieces ? stage_pieces_h2d(c, dst, *pieces) : stage_h2d(c, dst, src, n, pinned_src));
    c->ckpt_valid = true;
    return PGH_OK;
}

int pgh_fedavg(pgh_ctx* c, int mode, const float* ckpt, float* out) {
    if (c) RC(check_mode_use(c, mode, USE_RESIDENT));
    if (c && c->grp) return pgh_group_api::fedavg(c, mode, ckpt, out);
    RC(check_dtype(c, PGH_F32));
    if (!ckpt || !out) return fail(c, PGH_E_ARG, "ckpt / out is NULL");
    DeviceGuard g(c->device);
    const double t0 = now_ms();
    const size_t bytes = sizeof(float) * (size_t)c->pg;
    RC(upload_ckpt(c, (const uint8_t*)ckpt, bytes, is_pinned(ckpt)));
    RC(pgh_fedavg_device(c, mode, c->d_ckpt.as<float>(), c->d_out.as<float>(), c->stream));
    if (is_pinned(out)) {
        CK(c, hipMemcpyAsync(out, c->d_out.as<float>(), bytes, hipMemcpyDeviceToHost, c->stream));
        CK(c, hipStreamSynchronize(c->stream));
    } else {
        RC(stage_d2h_pieces(c, c->d_out.as<uint8_t>(), {OutPiece{(uint8_t*)out, bytes}}, c->stream));
    }
    c->st.close_ms_last = now_ms() - t0;
    return collect_timings(c);
}

// ---- resident checkpoint: the new checkpoint stays in HBM as the next cycle's input ------------

int pgh_ckpt_upload(pgh_ctx* c, const float* ckpt, size_t nbytes) {
    if (c && c->grp) return pgh_group_api::ckpt_upload(c, ckpt, nbytes);
    RC(check_dtype(c, PGH_F32));
    if (!ckpt) return fail(c, PGH_E_ARG, "ckpt is NULL");
    size_t first = 0;
    RC(shard_start(c, "checkpoint", nbytes, 4, &first));
    DeviceGuard g(c->device);
    return upload_ckpt(c, (const uint8_t*)(ckpt + first), 4 * (size_t)c->pg, is_pinned(ckpt));
}

int pgh_ckpt_upload_state(pgh_ctx* c, const uint8_t* pb, size_t n) {
    if (c && c->grp) return pgh_group_api::ckpt_upload_state(c, pb, n);
    RC(check_dtype(c, PGH_F32));
    if (!pb && n) return fail(c, PGH_E_ARG, "pb is NULL");
    std::vector<std::pair<size_t, size_t>> spans;
    RC(state_shard_spans(c, pb, n, &spans, "checkpoint"));
    std::vector<Piece> pieces;
    for (auto& sp : spans) pieces.push_back(Piece{pb + sp.first, sp.second});
    DeviceGuard g(c->device);
    return upload_ckpt(c, nullptr, 0, false, &pieces);
}

int pgh_fedavg_resident(pgh_ctx* c, int mode) {
    if (c) RC(check_mode_use(c, mode, USE_RESIDENT));
    if (c && c->grp) return pgh_group_api::fedavg_resident(c, mode);
    RC(check_dtype(c, PGH_F32));
    RC(check_ckpt(c, "pgh_fedavg_resident"));
    DeviceGuard g(c->device);
    const double t0 = now_ms();
    clear_final_marks(c);
    const int K = final_ranges(c);
    if (K == 1) {
        RC(pgh_fedavg_device(c, mode, c->d_ckpt.as<float>(), c->d_out.as<float>(), c->stream));
    } else {  // the same fold as K range launches, each followed by its mark (pipelined close)
        int64_t n = 0;
        RC(resident_count(c, &n));
        FinalArgs fa;
        fa.ckpt = c->d_ckpt.as<float>();
        fa.out = c->d_out.as<float>();
        RC(fedavg_divisor(c, mode, n, &fa.divisor));
        RC(fork_aux(c, c->stream));
        for (int k = 0; k < K; ++k) {
            fa.off = range_edge(c, k, K);
            fa.len = range_edge(c, k + 1, K) - fa.off;
            const hipStream_t rs = range_stream(c, c->stream, k);
            RC(fold_run(c, mode, 0, n, true, fa, rs));
            RC(add_final_mark(c, rs, fa.off + fa.len));
        }
        RC(join_aux(c, c->stream));
    }
    std::swap(c->d_ckpt, c->d_out);  // the new checkpoint is the next cycle's input
    c->st.close_ms_last = now_ms() - t0;
    return PGH_OK;
}

int pgh_ckpt_download(pgh_ctx* c, float* out) {
    if (c && c->grp) return pgh_group_api::ckpt_download(c, out);
    RC(check_dtype(c, PGH_F32));
    if (!out) return fail(c, PGH_E_ARG, "out is NULL");
    RC(check_ckpt(c, "pgh_ckpt_download"));
    DeviceGuard g(c->device);
    const size_t bytes = 4 * (size_t)c->pg;
    RC(order_after_ingest(c, c->stream));
    if (is_pinned(out)) {
        CK(c, hipMemcpyAsync(out, c->d_ckpt.as<float>(), bytes, hipMemcpyDeviceToHost, c->stream));
        CK(c, hipStreamSynchronize(c->stream));
    } else {
        RC(stage_d2h_pieces(c, c->d_ckpt.as<uint8_t>(), {OutPiece{(uint8_t*)out, bytes}}, c->stream, nullptr, true));
    }
    return collect_timings(c);
}

int pgh_ckpt_patch_state(pgh_ctx* c, const uint8_t* tmpl, size_t n, uint8_t* out) {
    if (c && c->grp) return pgh_group_api::ckpt_patch_state(c, tmpl, n, out);
    RC(check_dtype(c, PGH_F32));
    if (!tmpl || !out) return fail(c, PGH_E_ARG, "tmpl / out is NULL");
    RC(check_ckpt(c, "pgh_ckpt_patch_state"));
    std::vector<std::pair<size_t, size_t>> spans;
    RC(state_shard_spans(c, tmpl, n, &spans, "checkpoint template"));
    DeviceGuard g(c->device);
    std::vector<CopyPool::Seg> gaps;
    bool ordered = true;
    if (out != tmpl) {  // template bytes outside this shard's payload slices (framing, other shards)
        size_t pos = 0;
        for (auto& sp : spans) {
            ordered = ordered && sp.first >= pos;
            if (sp.first > pos) gaps.push_back({out + pos, tmpl + pos, sp.first - pos});
            pos = sp.first + sp.second;
        }
        if (n > pos) gaps.push_back({out + pos, tmpl + pos, n - pos});
    }
    std::vector<OutPiece> pieces;
    for (auto& sp : spans) pieces.push_back(OutPiece{out + sp.first, sp.second});
    RC(order_after_ingest(c, c->stream));
    if (!ordered) {  // overlapping spans (never from the walker): whole template first, then payloads
        c->pool_copy->run({CopyPool::Seg{out, tmpl, n}});
        gaps.clear();
    }
    // the framing copy and the pre-fault of the output run while the first slot's DMA flies (in
    // place, out == tmpl, is how a freshly framed checkpoint is filled: its pages are fresh too)
    RC(stage_d2h_pieces(c, c->d_ckpt.as<uint8_t>(), pieces, c->stream, [&] {
        prefault_parallel(out, n, *c->pool_copy);
        if (!gaps.empty()) c->pool_copy->run(gaps);
    }, true));
    return collect_timings(c);
}

int pgh_secagg_device(pgh_ctx* c, int base, int prec, int64_t* d_sum, float* d_dec, void* stream) {
    return pgh_secagg_device_range(c, base, prec, 0, -1, d_sum, d_dec, stream);  // the whole shard
}

int pgh_secagg_device_range(pgh_ctx* c, int base, int prec, int64_t off, int64_t len, int64_t* d_sum, float* d_dec,
                            void* stream) {
    if (c && c->grp) return fail(c, PGH_E_UNSUPPORTED, "pgh_secagg_device* takes device pointers, which name one GPU: call it on pgh_group_child");
    RC(check_dtype(c, PGH_I64));
    DeviceGuard g(c->device);
    int64_t n = 0;
    RC(resident_count(c, &n));
    FinalArgs fa;
    fa.sum = d_sum;
    fa.dec = d_dec;
    fa.off = off;
    fa.len = len;
    RC(fixed_point_divisor(c, base, prec, &fa.divisor));
    return fold_run(c, KIND_SECAGG, 0, n, true, fa, (hipStream_t)stream);
}

// The share sum and / or its decode from d_sum / d_dec to the host behind the fold on c->stream; ends
// the close that began at t0.
static int secagg_download(pgh_ctx* c, int64_t* sum_out, float* dec_out, double t0) {
    if (sum_out) CK(c, hipMemcpyAsync(sum_out, c->d_sum.as<int64_t>(), 8ull * c->pg, hipMemcpyDeviceToHost, c->stream));
    if (dec_out) CK(c, hipMemcpyAsync(dec_out, c->d_dec.as<float>(), 4ull * c->pg, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    c->st.close_ms_last = now_ms() - t0;
    return collect_timings(c);
}

int pgh_secagg_decode_device(pgh_ctx* c, int base, int prec, const int64_t* d_sum, int64_t n, float* d_dec,
                             void* stream) {
    if (c && c->grp) return fail(c, PGH_E_UNSUPPORTED, "%s takes device pointers, which name one GPU: call it on pgh_group_child", __func__);
    if (!c) return fail(nullptr, PGH_E_ARG, "null context");
    if (n < 0 || (n > 0 && (!d_sum || !d_dec))) return fail(c, PGH_E_ARG, "bad decode arguments (n=%lld)", (long long)n);
    DeviceGuard g(c->device);
    float div = 1.f;
    RC(fixed_point_divisor(c, base, prec, &div));
    const hipStream_t s = (hipStream_t)stream;
    // not in pgh_stats' kernel timings: those stay the share-sum / fold kernels' (12 B per param here)
    const hipError_t e = pgh::launch_secagg_decode(d_sum, d_dec, n, div, s);
    if (e != hipSuccess) return fail(c, PGH_E_HIP, "decode launch failed: %s", hipGetErrorString(e));
    return PGH_OK;
}

int pgh_secagg(pgh_ctx* c, int base, int prec, int64_t* sum_out, float* dec_out) {
    if (c && c->grp) return pgh_group_api::secagg(c, base, prec, sum_out, dec_out);
    RC(check_dtype(c, PGH_I64));
    DeviceGuard g(c->device);
    const double t0 = now_ms();
    RC(pgh_secagg_device(c, base, prec, sum_out ? c->d_sum.as<int64_t>() : nullptr, dec_out ? c->d_dec.as<float>() : nullptr, c->stream));
    return secagg_download(c, sum_out, dec_out, t0);
}

// ---- STREAM reductions ---------------------------------------------------------------------------

int pgh_stream_begin(pgh_ctx* c, int kind, int fold_batch) {
    if (c && kind != PGH_STREAM_SECAGG) RC(check_mode_use(c, kind, USE_STREAM));
    if (c && c->grp) return pgh_group_api::stream_begin(c, kind, fold_batch);
    RC(check_ready(c));
    if (kind == PGH_STREAM_SECAGG) {
        if (c->dtype != PGH_I64) return fail(c, PGH_E_STATE, "secagg stream needs an int64 slab");
    } else if (c->dtype != PGH_F32) {
        return fail(c, PGH_E_ARG, "stream kind %d does not match the slab", kind);
    }
    DeviceGuard g(c->device);
    RC(pgh_reset(c));
    c->streaming = true;
    c->kind = kind == PGH_STREAM_SECAGG ? KIND_SECAGG : kind;
    c->fold_batch = fold_batch <= 0 ? std::max(1, c->slots / 2) : std::min(fold_batch, c->slots);
    return PGH_OK;
}

int pgh_stream_flush(pgh_ctx* c) {
    if (c && c->grp) return pgh_group_api::stream_flush(c);
    RC(check_ready(c));
    if (!c->streaming) return fail(c, PGH_E_STATE, "not streaming");
    DeviceGuard g(c->device);
    return maybe_fold(c, true);
}

namespace {
int stream_finish(pgh_ctx* c, FinalArgs fa, hipStream_t cs, bool fedavg, int mode_or_base) {
    if (!c->streaming) return fail(c, PGH_E_STATE, "not streaming (call pgh_stream_begin first)");
    if (fedavg) RC(check_noise_final(c, c->kind));  // (a stream never clips: with noise on it cannot close)
    const int64_t run = ready_run(c, c->folded);
    RC(check_no_gaps(c, c->folded, run));
    const int64_t n = c->folded + run;
    if (n == 0) return fail(c, PGH_E_STATE, "no diffs ingested");
    if (fedavg) RC(fedavg_divisor(c, mode_or_base, n, &fa.divisor));
    RC(join_in(c, cs));
    RC(fold_run(c, c->kind, c->folded, run, true, fa, c->stream));
    RC(join_out(c, cs));
    for (int64_t k = 0; k < run; ++k) c->slot_client[(size_t)((c->folded + k) % c->slots)] = -1;
    c->folded = n;
    c->st.n_folded = n;
    c->streaming = false;
    return PGH_OK;
}
}  // namespace

int pgh_stream_finish_device(pgh_ctx* c, const float* d_ckpt, float* d_out, void* stream) {
    if (c && c->grp) return fail(c, PGH_E_UNSUPPORTED, "%s takes device pointers, which name one GPU: call it on pgh_group_child", __func__);
    RC(check_dtype(c, PGH_F32));
    if (!d_ckpt || !d_out || (((uintptr_t)d_ckpt | (uintptr_t)d_out) & 15))
        return fail(c, PGH_E_ARG, "d_ckpt / d_out must be 16-byte aligned device pointers");
    DeviceGuard g(c->device);
    FinalArgs fa;
    fa.ckpt = d_ckpt;
    fa.out = d_out;
    return stream_finish(c, fa, (hipStream_t)stream, true, c->kind);
}

int pgh_stream_finish_resident(pgh_ctx* c) {
    if (c && c->grp) return pgh_group_api::stream_finish_resident(c);
    RC(check_dtype(c, PGH_F32));
    RC(check_ckpt(c, "pgh_stream_finish_resident"));
    if (c->streaming) RC(check_noise_final(c, c->kind));
    DeviceGuard g(c->device);
    clear_final_marks(c);
    const double t0 = now_ms();
    RC(pgh_stream_finish_device(c, c->d_ckpt.as<float>(), c->d_out.as<float>(), c->stream));
    std::swap(c->d_ckpt, c->d_out);  // the new checkpoint is the next cycle's input
    c->st.close_ms_last = now_ms() - t0;
    return PGH_OK;
}

int pgh_stream_finish(pgh_ctx* c, const float* ckpt, float* out) {
    if (c && c->grp) return pgh_group_api::stream_finish(c, ckpt, out);
    RC(check_dtype(c, PGH_F32));
    if (!ckpt || !out) return fail(c, PGH_E_ARG, "ckpt / out is NULL");
    if (c->streaming) RC(check_noise_final(c, c->kind));
    DeviceGuard g(c->device);
    const double t0 = now_ms();
    const size_t bytes = sizeof(float) * (size_t)c->pg;
    // staged like pgh_fedavg's checkpoint: on the copy stream after every fold that may still read
    // d_ckpt, so fold_run's order_after_ingest orders the final fold after it (a pageable
    // pgh_ckpt_upload's last ring DMA can no longer land after this copy)
    RC(upload_ckpt(c, (const uint8_t*)ckpt, bytes, is_pinned(ckpt)));
    RC(pgh_stream_finish_device(c, c->d_ckpt.as<float>(), c->d_out.as<float>(), c->stream));
    CK(c, hipMemcpyAsync(out, c->d_out.as<float>(), bytes, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    c->st.close_ms_last = now_ms() - t0;
    return collect_timings(c);
}

int pgh_stream_finish_secagg_device(pgh_ctx* c, int base, int prec, int64_t* d_sum, float* d_dec, void* stream) {
    if (c && c->grp) return fail(c, PGH_E_UNSUPPORTED, "%s takes device pointers, which name one GPU: call it on pgh_group_child", __func__);
    RC(check_dtype(c, PGH_I64));
    DeviceGuard g(c->device);
    FinalArgs fa;
    fa.sum = d_sum;
    fa.dec = d_dec;
    RC(fixed_point_divisor(c, base, prec, &fa.divisor));
    return stream_finish(c, fa, (hipStream_t)stream, false, base);
}

int pgh_stream_finish_secagg(pgh_ctx* c, int base, int prec, int64_t* sum_out, float* dec_out) {
    if (c && c->grp) return pgh_group_api::stream_finish_secagg(c, base, prec, sum_out, dec_out);
    RC(check_dtype(c, PGH_I64));
    DeviceGuard g(c->device);
    const double t0 = now_ms();
    RC(pgh_stream_finish_secagg_device(c, base, prec, sum_out ? c->d_sum.as<int64_t>() : nullptr, dec_out ? c->d_dec.as<float>() : nullptr,
                                       c->stream));
    return secagg_download(c, sum_out, dec_out, t0);
}

