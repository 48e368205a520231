// libpygrid_hip: top-k sparsification of the averaged update at the close (K18; SparseFed) -- the launches behind
// a FINAL fold (topk_launch, called by fold_launch alone), the setting, the error memory's planes, the commit,
// download and upload, and what the last close selected.  The state: TopkState in pgh_rules.h.
// (struct pgh_ctx and the shared helpers: pgh_ctx.h)
#include "pgh_ctx.h"

using namespace pgh_detail;

// (the public entry points take their C linkage from include/pgh_api.h)

namespace pgh_detail {

int check_topk_final(pgh_ctx* c, int64_t off, int64_t len) {
    if (off != 0 || (len >= 0 && len != c->pg))
        return fail(c, PGH_E_UNSUPPORTED, "top-k is set (pgh_set_topk): a FINAL over [%lld,+%lld) of %lld params cannot select, "
                    "the k largest are taken over all of them in one launch", (long long)off, (long long)len, (long long)c->pg);
    if (noise_on(c)) return fail(c, PGH_E_UNSUPPORTED, "top-k is set (pgh_set_topk): it takes no DP noise (pgh_set_dp_noise) beside it");
    return PGH_OK;
}

// K18 behind a FINAL fold of the whole shard: hist<0>, pick, hist<1>, pick, hist<2>, pick, apply -- each launch
// timed and accounted on its own.  Per param: 8 bytes (d in, u out; 12 with the error memory in), 4 and 4 (u in),
// then 12 (u and ckpt in, out out; 8 ahead of K10: u in, d out) and 4 more for the pending memory.
int topk_launch(pgh_ctx* c, const FinalArgs& fa, bool into_opt, hipStream_t s) {
    TopkState& tk = c->topk;
    if (tk.k > c->pg) return fail(c, PGH_E_STATE, "top-k: k = %lld exceeds the shard's %lld params", (long long)tk.k, (long long)c->pg);
    pgh::TopkArgs a{};
    a.d = into_opt ? c->opt.d_d.as<float>() : tk.d_u.as<float>();
    a.e = tk.feedback ? tk.d_e.as<float>() : nullptr;
    a.u = tk.d_u.as<float>();
    a.ckpt = into_opt ? nullptr : fa.ckpt;
    a.out = into_opt ? c->opt.d_d.as<float>() : fa.out;
    a.e2 = tk.feedback ? tk.d_e2.as<float>() : nullptr;
    a.blk = tk.d_blk.as<pgh::TopkBlock>();
    a.p = c->pg;
    a.k = (uint32_t)tk.k;
    const uint64_t pg = (uint64_t)c->pg, blk = sizeof(pgh::TopkBlock);
    if (!tk.blk_clean) RC(timed_launch(c, s, blk, [&] { return pgh::launch_topk_clear(a.blk, s); }));
    tk.blk_clean = false;
    for (int digit = 0; digit < 3; ++digit) {
        const uint64_t bytes = digit == 0 ? (tk.feedback ? 12ull : 8ull) * pg : 4ull * pg;
        RC(timed_launch(c, s, bytes, [&] { return pgh::launch_topk_hist(a, digit, s); }));
        RC(timed_launch(c, s, 2 * blk, [&] { return pgh::launch_topk_pick(a, digit, s); }));
    }
    tk.blk_clean = true;  // (the third pick cleared it)
    RC(timed_launch(c, s, ((into_opt ? 8ull : 12ull) + (tk.feedback ? 4ull : 0ull)) * pg, [&] { return pgh::launch_topk_apply(a, s); }));
    tk.pending = true;
    tk.ran = true;
    return PGH_OK;
}

namespace {
int check_topk_ctx(pgh_ctx* c, const char* what, bool on) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return fail(c, PGH_E_UNSUPPORTED, "%s: a group's shards each hold part of the update (a global k would need the histograms all-reduced)", what);
    if (on && !topk_on(c)) return fail(c, PGH_E_STATE, "%s: top-k is not set", what);
    return PGH_OK;
}
int check_feedback(pgh_ctx* c, const char* what) {
    RC(check_topk_ctx(c, what, true));
    if (!c->topk.feedback) return fail(c, PGH_E_STATE, "%s: top-k is set without an error memory", what);
    return PGH_OK;
}
}  // namespace

}  // namespace pgh_detail

int pgh_set_topk(pgh_ctx* c, int64_t k, int error_feedback) {
    if (c && c->grp && k == 0) return PGH_OK;  // off: always possible (a group never has it on)
    RC(check_topk_ctx(c, "pgh_set_topk", false));
    if (k < 0) return fail(c, PGH_E_ARG, "top-k: k = %lld is negative", (long long)k);
    TopkState& tk = c->topk;
    const bool fb = error_feedback != 0;
    if (k == 0) {
        if (!topk_on(c)) return PGH_OK;
        DeviceGuard g(c->device);
        RC(folds_quiesce(c));
        tk.release();
        return PGH_OK;
    }
    if (!c->layout) return fail(c, PGH_E_STATE, "pgh_set_layout has not been called");
    if (c->pg != c->P) return fail(c, PGH_E_UNSUPPORTED, "pgh_set_topk: the shard [%lld,%lld) is narrower than the model", (long long)c->lo, (long long)c->hi);
    if (c->d_slab && c->dtype != PGH_F32) return fail(c, PGH_E_UNSUPPORTED, "pgh_set_topk: the slab holds int64 shares");
    if (c->streaming) return fail(c, PGH_E_UNSUPPORTED, "pgh_set_topk: the context is streaming");
    if (k > c->P) return fail(c, PGH_E_ARG, "top-k: k = %lld exceeds the model's %lld params", (long long)k, (long long)c->P);
    if (c->P > 0xffffffffll) return fail(c, PGH_E_UNSUPPORTED, "top-k: the counts are 32-bit, the model has %lld params", (long long)c->P);
    if (k == tk.k && fb == tk.feedback) return PGH_OK;  // the same again: the error memory stays
    DeviceGuard g(c->device);
    RC(folds_quiesce(c));
    tk.release();
    const size_t bytes = 4 * (size_t)c->pvec;
    if (!tk.d_u.reserve(bytes) || !tk.d_blk.reserve(sizeof(pgh::TopkBlock)) ||
        (fb && (!tk.d_e.reserve(bytes) || !tk.d_e2.reserve(bytes)))) {
        tk.release();
        return fail(c, PGH_E_OOM, "allocation of the top-k planes (%zu bytes each) failed", bytes);
    }
    tk.pvec = c->pvec;
    int rc = c->nz.ensure(c, c->stream);
    // e = +0.0 in both planes: the pending one is written whole by every close
    hipError_t e = hipSuccess;
    if (!rc && fb) e = hipMemsetD32Async((hipDeviceptr_t)tk.d_e.as<void>(), 0, (size_t)c->pvec, c->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (!rc && e != hipSuccess) rc = fail(c, PGH_E_HIP, "clearing the error memory failed: %s", hipGetErrorString(e));
    if (rc) {
        tk.release();
        return rc;
    }
    tk.k = k;
    tk.feedback = fb;
    return PGH_OK;
}

int pgh_topk_commit(pgh_ctx* c) {
    RC(check_topk_ctx(c, "pgh_topk_commit", true));
    TopkState& tk = c->topk;
    if (!tk.pending) return fail(c, PGH_E_STATE, "pgh_topk_commit: no FINAL fold has run since the last commit or upload");
    // (a pointer swap: every FINAL with the setting on covers the whole shard, so nothing is copied; the next
    // close's apply pass writes the plane committed until now behind this close's on the same stream)
    std::swap(tk.d_e, tk.d_e2);
    tk.pending = false;
    return PGH_OK;
}

int pgh_topk_download(pgh_ctx* c, float* e) {
    RC(check_feedback(c, "pgh_topk_download"));
    if (!e) return fail(c, PGH_E_ARG, "e is NULL");
    DeviceGuard g(c->device);
    RC(folds_quiesce(c));
    CK(c, hipMemcpy(e, c->topk.d_e.as<float>(), 4 * (size_t)c->pg, hipMemcpyDeviceToHost));
    return PGH_OK;
}

int pgh_topk_upload(pgh_ctx* c, const float* e, size_t nbytes) {
    RC(check_feedback(c, "pgh_topk_upload"));
    if (!e) return fail(c, PGH_E_ARG, "e is NULL");
    if (nbytes != 4 * (size_t)c->pg) return fail(c, PGH_E_ARG, "error memory: %zu bytes given, the model has %lld params", nbytes, (long long)c->pg);
    DeviceGuard g(c->device);
    RC(folds_quiesce(c));
    CK(c, hipMemcpy(c->topk.d_e.as<float>(), e, nbytes, hipMemcpyHostToDevice));
    c->topk.pending = false;
    return PGH_OK;
}

int pgh_topk_stats(pgh_ctx* c, int64_t* k, uint32_t* tau_bits, int64_t* kept) {
    RC(check_topk_ctx(c, "pgh_topk_stats", false));
    if (k) *k = c->topk.k;
    if (tau_bits) *tau_bits = 0;
    if (kept) *kept = 0;
    if (!c->topk.ran) return PGH_OK;  // no close since the setting: nothing selected yet
    DeviceGuard g(c->device);
    RC(folds_quiesce(c));
    uint32_t st[6];  // TopkBlock past the histogram: prefix, rank, n_eq, pad, n_gt
    static_assert(sizeof(pgh::TopkBlock) == 4 * pgh::TOPK_BINS + sizeof(st), "the state words behind the histogram");
    CK(c, hipMemcpy(st, c->topk.d_blk.as<uint8_t>() + 4 * pgh::TOPK_BINS, sizeof(st), hipMemcpyDeviceToHost));
    uint64_t n_gt;
    std::memcpy(&n_gt, &st[4], 8);
    if (tau_bits) *tau_bits = st[0];
    if (kept) *kept = (int64_t)(n_gt + st[2]);
    return PGH_OK;
}
