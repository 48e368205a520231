// libpygrid_hip: server optimizers at the close (K10; FedAvgM, FedAdagrad, FedAdam, FedYogi) -- the launch
// behind a FINAL fold (server_opt_launch, called by fold_launch alone), the setting, the moment planes, the
// commit with its coverage ranges, download and upload.  The state: ServerOptState in pgh_rules.h.
// (struct pgh_ctx and the shared helpers: pgh_ctx.h)
#include "pgh_ctx.h"

#include <cmath>

using namespace pgh_detail;

// (the public entry points take their C linkage from include/pgh_api.h)

namespace pgh_detail {

// K10 behind a FINAL fold of [fa.off, fa.off + fa.len) on stream s: d, the real ckpt and the committed
// moments in; the real out and the pending moments out.  28 bytes per param (20 for FedAvgM, which has no v).
int server_opt_launch(pgh_ctx* c, const FinalArgs& fa, hipStream_t s) {
    if (!fa.ckpt || !fa.out) return fail(c, PGH_E_ARG, "a FINAL fold with a server optimizer needs ckpt and out");
    ServerOptState& so = c->opt;
    const bool adaptive = so.kind != PGH_OPT_MOMENTUM;
    pgh::ServerOptArgs o{};
    o.d = so.d_d.as<float>() + fa.off;
    o.ckpt = fa.ckpt + fa.off;
    o.out = fa.out + fa.off;
    o.m = so.d_m.as<float>() + fa.off;
    o.m2 = so.d_m2.as<float>() + fa.off;
    o.v = adaptive ? so.d_v.as<float>() + fa.off : nullptr;
    o.v2 = adaptive ? so.d_v2.as<float>() + fa.off : nullptr;
    o.p = fa.len;
    o.kind = so.kind;
    o.lr = so.lr; o.beta1 = so.beta1; o.beta2 = so.beta2;
    o.c1 = so.c1; o.c2 = so.c2; o.tau = so.tau;
    RC(timed_launch(c, s, (adaptive ? 28ull : 20ull) * (uint64_t)fa.len, [&] { return pgh::launch_server_opt(o, s); }));
    so.pending = true;
    const std::pair<int64_t, int64_t> r{fa.off, fa.off + fa.len};  // (a repeated FINAL lists its range once)
    if (std::find(so.cov.begin(), so.cov.end(), r) == so.cov.end()) so.cov.push_back(r);
    return PGH_OK;
}

void ServerOptState::release() {
    for (auto* v : {&d_d, &d_m, &d_v, &d_m2, &d_v2}) v->reset();
    kind = PGH_OPT_NONE;
    nothing_pending();
    steps = 0;
    pvec = 0;
}

namespace {
// Every launch that reads or writes the planes has finished: the context's reduction stream and the
// folds issued on callers' streams.
int opt_quiesce(pgh_ctx* c) {
    CK(c, hipStreamSynchronize(c->stream));
    CK(c, hipStreamSynchronize(c->aux));
    for (auto& fe : c->fold_evs) CK(c, hipEventSynchronize(fe.second));
    return PGH_OK;
}

// m = +0, v = tau * tau in the committed planes; nothing pending, no step counted.
int opt_init_state(pgh_ctx* c) {
    ServerOptState& so = c->opt;
    const size_t n = (size_t)so.pvec;
    const float v0 = so.tau * so.tau;
    uint32_t v0_bits;
    std::memcpy(&v0_bits, &v0, 4);
    // (the pending planes too: a first close that covers only part of the shard leaves the rest as it began)
    for (auto* b : {&so.d_m, &so.d_m2}) CK(c, hipMemsetD32Async((hipDeviceptr_t)b->as<void>(), 0, n, c->stream));
    for (auto* b : {&so.d_v, &so.d_v2})
        if (*b) CK(c, hipMemsetD32Async((hipDeviceptr_t)b->as<void>(), (int)v0_bits, n, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    so.nothing_pending();
    so.steps = 0;
    return PGH_OK;
}

int check_opt_on(pgh_ctx* c, const char* what) {
    if (c->opt.kind == PGH_OPT_NONE) return fail(c, PGH_E_STATE, "%s: no server optimizer is set", what);
    return PGH_OK;
}
}  // namespace

}  // namespace pgh_detail

int pgh_set_server_opt(pgh_ctx* c, int kind, float lr, float beta1, float beta2, float tau) {
    if (!c) return PGH_E_ARG;
    if (kind < PGH_OPT_NONE || kind > PGH_OPT_YOGI) return fail(c, PGH_E_ARG, "unknown server optimizer %d", kind);
    if (kind != PGH_OPT_NONE) {
        if (!std::isfinite(lr) || !(lr > 0.f)) return fail(c, PGH_E_ARG, "the server learning rate must be finite and > 0");
        if (!(beta1 >= 0.f && beta1 < 1.f)) return fail(c, PGH_E_ARG, "beta1 must be in [0, 1)");
        if (kind == PGH_OPT_MOMENTUM) {
            beta2 = 0.f;  // (not used: ignored)
            tau = 0.f;
        } else {
            if (kind == PGH_OPT_ADAGRAD) beta2 = 0.f;
            else if (!(beta2 >= 0.f && beta2 < 1.f)) return fail(c, PGH_E_ARG, "beta2 must be in [0, 1)");
            if (!std::isfinite(tau) || !(tau > 0.f)) return fail(c, PGH_E_ARG, "tau must be finite and > 0");
        }
    }
    if (c->grp) return pgh_group_api::set_server_opt(c, kind, lr, beta1, beta2, tau);
    ServerOptState& so = c->opt;
    if (kind == PGH_OPT_NONE) {
        if (so.kind == PGH_OPT_NONE) return PGH_OK;
        DeviceGuard g(c->device);
        RC(opt_quiesce(c));
        so.release();
        return PGH_OK;
    }
    if (!c->layout) return fail(c, PGH_E_STATE, "pgh_set_layout has not been called");
    if (kind == so.kind && lr == so.lr && beta1 == so.beta1 && beta2 == so.beta2 && tau == so.tau)
        return PGH_OK;  // the same again: the state stays
    DeviceGuard g(c->device);
    RC(opt_quiesce(c));
    so.release();
    const size_t bytes = 4 * (size_t)c->pvec;
    const bool adaptive = kind != PGH_OPT_MOMENTUM;
    if (!so.d_d.reserve(bytes) || !so.d_m.reserve(bytes) || !so.d_m2.reserve(bytes) ||
        (adaptive && (!so.d_v.reserve(bytes) || !so.d_v2.reserve(bytes)))) {
        so.release();
        return fail(c, PGH_E_OOM, "allocation of the server optimizer's planes (%zu bytes each) failed", bytes);
    }
    so.pvec = c->pvec;
    so.lr = lr; so.beta1 = beta1; so.beta2 = beta2; so.tau = tau;
    so.c1 = 1.0f - beta1;
    so.c2 = 1.0f - beta2;
    int rc = c->nz.ensure(c, c->stream);
    if (!rc) rc = opt_init_state(c);
    if (rc) {
        so.release();
        return rc;
    }
    so.kind = kind;
    return PGH_OK;
}

int pgh_server_opt_commit(pgh_ctx* c) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return pgh_group_api::server_opt_commit(c);
    RC(check_opt_on(c, "pgh_server_opt_commit"));
    ServerOptState& so = c->opt;
    if (!so.pending) return fail(c, PGH_E_STATE, "pgh_server_opt_commit: no FINAL fold has run since the last commit or upload");
    // K10 wrote only the ranges its FINAL launches covered: a param outside them (a cycle closed with
    // pgh_fedavg_device_range over part of the shard) keeps its committed moments, copied into the
    // pending planes before the swap.  A close over the whole shard copies nothing.
    std::sort(so.cov.begin(), so.cov.end());
    DeviceGuard g(c->device);
    bool copied = false;
    const auto keep = [&](int64_t a, int64_t b) -> int {
        if (a >= b) return PGH_OK;
        const size_t n = 4 * (size_t)(b - a);
        CK(c, hipMemcpyAsync(so.d_m2.as<float>() + a, so.d_m.as<float>() + a, n, hipMemcpyDeviceToDevice, c->stream));
        if (so.d_v) CK(c, hipMemcpyAsync(so.d_v2.as<float>() + a, so.d_v.as<float>() + a, n, hipMemcpyDeviceToDevice, c->stream));
        copied = true;
        return PGH_OK;
    };
    int64_t pos = 0;
    for (const auto& r : so.cov) {
        RC(keep(pos, r.first));
        pos = std::max(pos, r.second);
    }
    RC(keep(pos, c->pg));
    if (copied) CK(c, hipStreamSynchronize(c->stream));  // (a later K10 may read them on a caller's stream)
    // (a pointer swap: the next cycle's K10 writes the planes committed until now behind this cycle's
    // on the same stream; folds on different caller streams are the caller's to order, as for d_acc)
    std::swap(so.d_m, so.d_m2);
    std::swap(so.d_v, so.d_v2);
    so.nothing_pending();
    so.steps += 1;
    return PGH_OK;
}

int pgh_server_opt_steps(pgh_ctx* c, int64_t* committed) {
    if (!c || !committed) return c ? fail(c, PGH_E_ARG, "committed is NULL") : PGH_E_ARG;
    if (c->grp) return pgh_group_api::server_opt_steps(c, committed);
    *committed = c->opt.steps;
    return PGH_OK;
}

int pgh_server_opt_download(pgh_ctx* c, float* m, float* v) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return pgh_group_api::server_opt_download(c, m, v);
    RC(check_opt_on(c, "pgh_server_opt_download"));
    const bool adaptive = c->opt.kind != PGH_OPT_MOMENTUM;
    if (!m || (adaptive && !v)) return fail(c, PGH_E_ARG, "m / v is NULL");
    DeviceGuard g(c->device);
    RC(opt_quiesce(c));
    const size_t bytes = 4 * (size_t)c->pg;
    CK(c, hipMemcpy(m, c->opt.d_m.as<float>(), bytes, hipMemcpyDeviceToHost));
    if (adaptive) CK(c, hipMemcpy(v, c->opt.d_v.as<float>(), bytes, hipMemcpyDeviceToHost));
    return PGH_OK;
}

int pgh_server_opt_upload(pgh_ctx* c, const float* m, const float* v, size_t nbytes) {
    if (!c) return PGH_E_ARG;
    if (c->grp) return pgh_group_api::server_opt_upload(c, m, v, nbytes);
    RC(check_opt_on(c, "pgh_server_opt_upload"));
    const bool adaptive = c->opt.kind != PGH_OPT_MOMENTUM;
    if (!m || (adaptive && !v)) return fail(c, PGH_E_ARG, "m / v is NULL");
    size_t skip = 0;
    RC(shard_start(c, "optimizer state", nbytes, 4, &skip));
    const size_t shard = 4 * (size_t)c->pg;
    DeviceGuard g(c->device);
    RC(opt_quiesce(c));
    CK(c, hipMemcpy(c->opt.d_m.as<float>(), m + skip, shard, hipMemcpyHostToDevice));
    if (adaptive) CK(c, hipMemcpy(c->opt.d_v.as<float>(), v + skip, shard, hipMemcpyHostToDevice));
    c->opt.nothing_pending();
    return PGH_OK;
}
