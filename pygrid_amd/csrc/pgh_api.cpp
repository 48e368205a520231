// libpygrid_hip: C-ABI context around the gfx950 aggregation kernels.
//
// One pgh_ctx = one GPU = one parameter shard.  It owns
//   * the HBM slab: R slots x rows_per_client rows (fp32 diffs, or n_parties int64 share rows
//     per client), column-blocked: the shard is cut into blocks of bw columns (256 KiB of one
//     row by default) and each block stores all rows one after another (SlabMap in
//     pgh_kernels.h), so a kernel lane walking down the rows of its column stays in one block;
//   * the [P_shard] device vectors (checkpoint, output, running fold state, weights);
//   * a 2-slot pinned host ring through which pageable host bytes reach the slab
//     (multi-threaded host memcpy into a pinned slot overlapping the previous slot's DMA on a
//     dedicated copy stream); page-locked caller buffers are DMA'd directly;
//   * HIP event pairs around every reduction launch (pgh_stats reports kernel time).
//
// Two ways to use the slab:
//   RESIDENT  client k lives in slot k until the context is reset; pgh_fedavg / pgh_secagg fold
//             all clients [0, n) in one launch (repeatable: the diffs stay resident).
//   STREAM    (pgh_stream_begin .. pgh_stream_finish) client k goes to slot k % R; every run of
//             consecutive clients starting at the fold front is folded into the running state
//             (in client order, so fp32 results are bit-identical to RESIDENT) and its slots
//             freed.  Lets N x P exceed HBM and overlaps H2D ingest with reduction (SURVEY 8(d)
//             configs 3-5) and folds diffs as they are reported.
//
// Reference mapping: ingest = the N x unserialize_model_params loop of
// cycle_manager.py:247-250; fedavg = :252-296; secagg = PySyft share add + .get() + float_prec
// (test_basic_syft_operations.py:417-424).  Errors are negative status codes plus a message (the
// Python shim raises a PyGridError subclass, as tasks/cycle.py:33-37 expects).
//
// This file: errors and state checks, lifecycle, observability and the group driver's internals.
// The file map is at the top of pgh_ctx.h.
#include <sched.h>

#include <fstream>

#include "pgh_ctx.h"

namespace pgh_detail {

std::vector<int> gpu_local_cpus(int device) {
    std::vector<int> out;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return out; }
    std::string id(bus);
    for (auto& ch : id) ch = (char)std::tolower((unsigned char)ch);
    std::ifstream f("/sys/bus/pci/devices/" + id + "/local_cpulist");
    std::string list;
    if (!f || !std::getline(f, list)) return out;
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return out;
    size_t pos = 0;
    while (pos < list.size()) {
        size_t end = list.find(',', pos);
        if (end == std::string::npos) end = list.size();
        const std::string r = list.substr(pos, end - pos);
        const size_t dash = r.find('-');
        const int a = std::atoi(r.c_str()), b = dash == std::string::npos ? a : std::atoi(r.c_str() + dash + 1);
        for (int cpu = a; cpu <= b && cpu < CPU_SETSIZE; ++cpu)
            if (cpu >= 0 && CPU_ISSET(cpu, &allowed)) out.push_back(cpu);
        pos = end + 1;
    }
    return out;
}

thread_local std::string g_create_err;

int vfail(pgh_ctx* c, int code, const char* fmt, va_list ap) {
    char buf[1024];
    vsnprintf(buf, sizeof buf, fmt, ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

int fail(pgh_ctx* c, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int r = vfail(c, code, fmt, ap);
    va_end(ap);
    return r;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Everything issued on the context's streams, and every fold on a caller's stream, has finished.
static void sync_work(pgh_ctx* c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy) (void)hipStreamSynchronize(c->copy);
    if (c->vdec.s) (void)hipStreamSynchronize(c->vdec.s);  // a varint decode writes slab rows
    for (auto& fe : c->fold_evs) (void)hipEventSynchronize(fe.second);  // folds on caller streams
}

void free_slab(pgh_ctx* c) {
    sync_work(c);
    for (auto* v : {&c->d_slab, &c->d_ckpt, &c->d_out, &c->d_acc, &c->d_uacc, &c->d_sum, &c->d_dec}) v->reset();
    c->fw.slab_freed();
    c->ckpt_valid = false;
    clear_final_marks(c);
    rules_slab_freed(c);
    c->slots = 0;
    c->slot_mode = -1;
    c->slot_client.clear();
    clear_marks(c);
    c->streaming = false;
    c->folded = 0;
    for (auto& fe : c->fold_evs) c->ev_pool.give(fe.second);
    c->fold_evs.clear();
    release_slot_fold_events(c);
    c->slot_read_seq.clear();
}

int check_ready(pgh_ctx* c) {
    if (!c) return PGH_E_ARG;
    if (!c->layout) return fail(c, PGH_E_STATE, "pgh_set_layout has not been called");
    if (!c->d_slab) return fail(c, PGH_E_STATE, "pgh_reserve has not been called");
    return PGH_OK;
}

int check_dtype(pgh_ctx* c, int dtype) {
    RC(check_ready(c));
    if (c->dtype != dtype) return fail(c, PGH_E_STATE, "slab holds dtype %d, call needs %d", c->dtype, dtype);
    return PGH_OK;
}

int check_slot_list(pgh_ctx* c, const int32_t* slots, int n, bool no_twice) {
    std::vector<char> seen(no_twice ? (size_t)c->slots : 0, 0);
    for (int k = 0; k < n; ++k) {
        const int32_t sl = slots[k];
        if (sl < 0 || sl >= c->slots) return fail(c, PGH_E_ARG, "slot %d outside [0,%d)", sl, c->slots);
        if (c->slot_client[(size_t)sl] < 0) return fail(c, PGH_E_STATE, "slot %d holds no unfolded diff", sl);
        if (!no_twice) continue;
        if (seen[(size_t)sl]) return fail(c, PGH_E_ARG, "slot %d listed twice", sl);
        seen[(size_t)sl] = 1;
    }
    return PGH_OK;
}

int check_ckpt(pgh_ctx* c, const char* what) {
    if (!c->ckpt_valid)
        return fail(c, PGH_E_STATE, "%s: no checkpoint in HBM (pgh_ckpt_upload* since the last pgh_reserve / layout "
                    "change)", what);
    return PGH_OK;
}

int shard_start(pgh_ctx* c, const char* what, size_t nbytes, size_t unit, size_t* first) {
    const size_t whole = (size_t)c->P * unit, shard = (size_t)c->pg * unit;
    if (nbytes != whole && nbytes != shard)
        return fail(c, PGH_E_ARG, "%s: got %zu bytes, layout needs %zu (model) or %zu (shard)", what, nbytes, whole, shard);
    *first = nbytes == whole ? (size_t)c->lo : 0;  // the whole model: take the slice
    return PGH_OK;
}

// Columns per block for a shard of pg elements of es bytes: one block when the whole row fits
// in block_bytes (or blocking is off), else the widest power of two <= block_bytes whose
// padding of the last block stays within 1/16 of the row.
void slab_geometry(int64_t pg, size_t es, size_t block_bytes, int64_t* bw, int64_t* nb, int* bshift) {
    const int64_t whole = (pg + 63) & ~(int64_t)63;
    int64_t maxc = 64;
    while (maxc * 2 * (int64_t)es <= (int64_t)block_bytes) maxc *= 2;
    if (block_bytes == 0 || whole <= maxc) { *bw = whole; *nb = 1; *bshift = 62; return; }
    int64_t b = maxc;
    while (b > 64 && ((pg + b - 1) / b) * b - pg > pg / 16) b /= 2;
    *bw = b;
    *nb = (pg + b - 1) / b;
    int sh = 0;
    while ((int64_t(1) << sh) < b) ++sh;
    *bshift = sh;
}

}  // namespace pgh_detail

using namespace pgh_detail;

extern "C" {

int pgh_abi_version(void) { return PGH_ABI_VERSION; }

int pgh_device_count(int* n) {
    if (!n) return PGH_E_ARG;
    int k = 0;
    hipError_t e = hipGetDeviceCount(&k);
    if (e != hipSuccess) { *n = 0; return fail(nullptr, PGH_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n = k;
    return PGH_OK;
}

const char* pgh_last_error(const pgh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int pgh_create(int device, size_t pinned_bytes, pgh_ctx** out) {
    if (!out) return fail(nullptr, PGH_E_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(nullptr, PGH_E_HIP, "no HIP device: %s", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, PGH_E_ARG, "device %d out of range [0,%d)", device, ndev);
    auto* c = new pgh_ctx();
    c->device = device;
    DeviceGuard g(device);
    if (pinned_bytes == 0) pinned_bytes = 256ull << 20;
    c->ring.slot_bytes = (pinned_bytes / 2) & ~(size_t)4095;
    if (c->ring.slot_bytes < 4096) c->ring.slot_bytes = 4096;
    c->copy_threads = std::min(16, pgh_int::usable_cpus());
    if (const char* e = std::getenv("PGH_COPY_THREADS")) c->copy_threads = std::max(1, std::atoi(e));
    {
        const char* nu = std::getenv("PGH_NUMA");
        if (!nu || std::atoi(nu) != 0) c->local_cpus = gpu_local_cpus(device);
    }
    c->pool_copy.reset(new CopyPool(c->copy_threads, c->local_cpus));
    if (const char* e = std::getenv("PGH_BLOCK_BYTES")) c->block_bytes = (size_t)std::max(0LL, std::atoll(e));
    if (const char* e = std::getenv("PGH_FINAL_RANGES")) c->final_split = std::max(1, std::atoi(e));
    bool ok = c->stream.make() == hipSuccess && c->copy.make() == hipSuccess && c->aux.make() == hipSuccess;
    ok = ok && xfer_made(c);  // the D2H stream, the transfer owners' events and knobs
    for (pgh_ctx::Event* ev : {&c->copy_done, &c->xsync, &c->aux_ev}) ok = ok && ev->make() == hipSuccess;
    ok = ok && rules_made(c);
    if (!ok) { pgh_destroy(c); return fail(nullptr, PGH_E_HIP, "stream/event creation failed"); }
    {
        // the pinned ring on the GPU's socket: allocated by a thread bound there, pages placed by
        // its (local) memory policy
        bool pin_ok = true;
        auto alloc = [&] {
            bind_thread(c->local_cpus);
            const unsigned flags = c->local_cpus.empty() ? hipHostMallocDefault : hipHostMallocNumaUser;
            // a placement the runtime refuses is not worth failing the context for
            for (int k = 0; k < 2 && pin_ok; ++k)
                pin_ok = c->ring.h_pin[k].reserve(c->ring.slot_bytes, flags) ||
                         (flags != hipHostMallocDefault && c->ring.h_pin[k].reserve(c->ring.slot_bytes));
        };
        if (c->local_cpus.empty()) alloc();
        else std::thread([&] { DeviceGuard g2(device); alloc(); }).join();
        if (!pin_ok) {
            const size_t bytes = c->ring.slot_bytes;
            pgh_destroy(c);
            return fail(nullptr, PGH_E_OOM, "pinned host allocation of %zu bytes failed", bytes);
        }
    }
    // Warm-up (PGH_WARMUP=0 skips it): the first kernel launch loads the code object and the first
    // copies set up the runtime's copy engines (the first ~1 MB H2D from the pinned ring took 8.3 ms
    // of host time, r01ao) -- ~11 ms that would otherwise land on the node's first cycle close
    // (profiles/r01am).  One small launch plus an H2D and a D2H of up to 2 MiB on the two streams.
    const char* wu = std::getenv("PGH_WARMUP");
    if (!wu || std::atoi(wu) != 0) {
        const int64_t n = (int64_t)std::min(c->ring.slot_bytes, (size_t)2 << 20) / 8;  // int64 values
        void* d = nullptr;
        ok = hipMalloc(&d, 12 * n) == hipSuccess;
        if (ok) {
            int64_t* d_sum = (int64_t*)d;
            float* d_dec = (float*)((uint8_t*)d + 8 * n);
            void* const pin0 = c->ring.h_pin[0].as<void>();
            std::memset(pin0, 0, 8 * n);
            ok = hipMemcpyAsync(d_sum, pin0, 8 * n, hipMemcpyHostToDevice, c->copy) == hipSuccess &&
                 hipStreamSynchronize(c->copy) == hipSuccess &&
                 (!c->d2h.s || (hipMemcpyAsync(d_sum, pin0, 8 * n, hipMemcpyHostToDevice, c->d2h.s) == hipSuccess &&
                                hipStreamSynchronize(c->d2h.s) == hipSuccess)) &&
                 pgh::launch_secagg_decode(d_sum, d_dec, n, 1.0f, c->stream) == hipSuccess &&
                 hipMemcpyAsync(c->ring.h_pin[1].as<void>(), d_sum, 8 * n, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                 hipStreamSynchronize(c->stream) == hipSuccess;
            (void)hipFree(d);
        }
        if (!ok) {  // best effort: a latency optimisation must not cost the node its engine
            (void)hipGetLastError();
            (void)hipStreamSynchronize(c->copy);
            (void)hipStreamSynchronize(c->stream);
            c->warmup_skipped = true;
        }
    }
    *out = c;
    return PGH_OK;
}

void pgh_destroy(pgh_ctx* c) {
    if (!c) return;
    if (c->grp) { pgh_group_api::destroy(c); return; }
    DeviceGuard g(c->device);  // (alive across the delete: the owners release on this device)
    sync_work(c);
    if (c->d2h.s) (void)hipStreamSynchronize(c->d2h.s);
    delete c;
}

int pgh_set_layout(pgh_ctx* c, int n_tensors, const int64_t* numel) {
    if (c && c->grp) return pgh_group_api::set_layout(c, n_tensors, numel);
    if (!c) return PGH_E_ARG;
    if (n_tensors <= 0 || !numel) return fail(c, PGH_E_ARG, "need at least one tensor");
    int64_t P = 0;
    for (int k = 0; k < n_tensors; ++k) {
        if (numel[k] < 0) return fail(c, PGH_E_ARG, "tensor %d has negative numel", k);
        P += numel[k];
    }
    if (P <= 0) return fail(c, PGH_E_ARG, "model has no parameters");
    DeviceGuard g(c->device);
    free_slab(c);
    c->numel.assign(numel, numel + n_tensors);
    c->P = P;
    c->layout = true;
    return pgh_set_shard(c, 0, P);
}

int pgh_set_shard(pgh_ctx* c, int64_t lo, int64_t hi) {
    if (c && c->grp) return pgh_group_api::set_shard(c, lo, hi);
    if (!c) return PGH_E_ARG;
    return pgh_detail::set_shard(c, lo, hi, false);
}

}  // extern "C"

int pgh_detail::set_shard(pgh_ctx* c, int64_t lo, int64_t hi, bool keep_opt) {
    if (!c->layout) return fail(c, PGH_E_STATE, "pgh_set_layout has not been called");
    if (lo < 0 || hi > c->P || lo >= hi)
        return fail(c, PGH_E_ARG, "shard [%lld,%lld) outside [0,%lld)", (long long)lo, (long long)hi, (long long)c->P);
    DeviceGuard g(c->device);
    free_slab(c);
    const int64_t pvec = std::max((hi - lo + 63) & ~(int64_t)63, (c->vec_min + 63) & ~(int64_t)63);
    rules_shard_set(c, lo, hi, pvec, keep_opt);
    c->lo = lo;
    c->hi = hi;
    c->pg = hi - lo;
    c->pvec = pvec;
    c->st.p_shard = c->pg;
    return PGH_OK;
}

extern "C" {

int pgh_reserve(pgh_ctx* c, int max_clients, int dtype, int n_parties) {
    if (c && c->grp) return pgh_group_api::reserve(c, max_clients, dtype, n_parties);
    if (!c) return PGH_E_ARG;
    if (!c->layout) return fail(c, PGH_E_STATE, "pgh_set_layout has not been called");
    if (max_clients <= 0) return fail(c, PGH_E_ARG, "max_clients must be positive");
    if (dtype != PGH_F32 && dtype != PGH_I64) return fail(c, PGH_E_ARG, "unknown dtype %d", dtype);
    if (dtype == PGH_F32) n_parties = 1;
    if (n_parties < 1) return fail(c, PGH_E_ARG, "n_parties must be >= 1");
    DeviceGuard g(c->device);
    free_slab(c);
    const size_t rows = (size_t)max_clients * (size_t)n_parties;
    slab_geometry(c->pg, esize(dtype), c->block_bytes, &c->bw, &c->nb, &c->bshift);
    c->bmask = c->bshift == 62 ? (int64_t(1) << 62) - 1 : c->bw - 1;
    c->bstride = c->nb > 1 ? (int64_t)rows * c->bw : 0;
    const size_t bytes = rows * (size_t)(c->nb * c->bw) * esize(dtype);
    if (!c->d_slab.reserve(bytes)) {
        return fail(c, PGH_E_OOM, "slab allocation of %zu bytes (%zu rows x %lld) failed", bytes, rows,
                    (long long)(c->nb * c->bw));
    }
    c->st.ld = c->bw;
    const size_t v4 = (size_t)c->pvec * 4, v8 = (size_t)c->pvec * 8;
    const bool ok = c->d_ckpt.reserve(v4) && c->d_out.reserve(v4) && c->d_acc.reserve(v4) && c->d_uacc.reserve(v8) &&
                    c->d_sum.reserve(v8) && c->d_dec.reserve(v4);
    if (!ok) {
        free_slab(c);
        return fail(c, PGH_E_OOM, "device vector allocation failed");
    }
    c->slots = max_clients;
    c->dtype = dtype;
    c->parties = n_parties;
    c->slot_client.assign((size_t)max_clients, -1);
    c->slot_read_seq.assign((size_t)max_clients, 0);
    rules_reserved(c, max_clients);
    c->fw.clear();
    c->st.max_clients = max_clients;
    c->st.n_clients = 0;
    c->st.n_folded = 0;
    return PGH_OK;
}

int pgh_reset(pgh_ctx* c) {
    if (c && c->grp) return pgh_group_api::reset(c);
    if (!c) return PGH_E_ARG;
    DeviceGuard g(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& fe : c->fold_evs) (void)hipEventSynchronize(fe.second);  // folds issued on caller streams
    for (auto& fe : c->fold_evs) c->ev_pool.give(fe.second);
    c->fold_evs.clear();
    clear_marks(c);
    release_slot_fold_events(c);  // c->stream is idle (synchronised above)
    std::fill(c->slot_client.begin(), c->slot_client.end(), -1);
    rules_reset(c);
    c->fw.clear();
    c->streaming = false;
    c->slot_mode = -1;
    c->folded = 0;
    c->st.n_clients = 0;
    c->st.n_folded = 0;
    return PGH_OK;
}

// ---- observability -------------------------------------------------------------------------------

int pgh_set_variant(pgh_ctx* c, int variant) {
    if (c && c->grp) return pgh_group_api::set_variant(c, variant);
    if (!c) return PGH_E_ARG;
    if (variant < -1 || variant >= pgh::N_VARIANTS)
        return fail(c, PGH_E_ARG, "variant %d outside [-1,%d]", variant, pgh::N_VARIANTS - 1);
    c->variant = variant;
    return PGH_OK;
}

int pgh_effective_variant(pgh_ctx* c, int mode) {
    if (c && c->grp) return pgh_group_api::effective_variant(c, mode);
    if (!c) return PGH_E_ARG;
    if (!c->layout) return fail(c, PGH_E_STATE, "pgh_set_layout has not been called");
    if (mode == PGH_TRIMMED_MEAN) return trim_variant(c);  // K8's two column widths, whatever pgh_set_variant says
    if (mode == PGH_MEDIAN) {  // K9 or K9p by the diffs held now, whatever pgh_set_variant says
        int64_t n = 0;
        for (int64_t k : c->slot_client) n += k >= 0 ? 1 : 0;
        return median_variant(c, n);
    }
    if (c->variant >= 0) return c->variant;
    if (mode == PGH_STREAM_SECAGG) return pgh::SECAGG_AUTO_VARIANT;
    if (!valid_mode(mode)) return fail(c, PGH_E_ARG, "unknown averaging mode %d", mode);
    return pgh::auto_variant(c->pg, kernel_mode(mode));
}

int pgh_stats(pgh_ctx* c, pgh_stats_t* out) {
    if (c && c->grp) return pgh_group_api::stats(c, out);
    if (!c || !out) return PGH_E_ARG;
    DeviceGuard g(c->device);
    RC(collect_timings(c));
    *out = c->st;
    return PGH_OK;
}

int pgh_reset_stats(pgh_ctx* c) {
    if (c && c->grp) return pgh_group_api::reset_stats(c);
    if (!c) return PGH_E_ARG;
    DeviceGuard g(c->device);
    RC(collect_timings(c));
    pgh_stats_t keep = c->st;
    c->st = pgh_stats_t{};
    c->st.p_shard = keep.p_shard;
    c->st.ld = keep.ld;
    c->st.n_clients = keep.n_clients;
    c->st.max_clients = keep.max_clients;
    c->st.n_folded = keep.n_folded;
    return PGH_OK;
}

int pgh_slab(pgh_ctx* c, void** d_slab, int64_t* ld, int64_t* block_pitch) {
    if (c && c->grp) return fail(c, PGH_E_UNSUPPORTED, "%s takes device pointers, which name one GPU: call it on pgh_group_child", __func__);
    if (!c || !d_slab || !ld || !block_pitch) return PGH_E_ARG;
    *d_slab = c->d_slab.as<void>();
    *ld = c->bw;
    *block_pitch = c->bstride;
    return PGH_OK;
}

int pgh_sync(pgh_ctx* c) {
    if (c && c->grp) return pgh_group_api::sync(c);
    if (!c) return PGH_E_ARG;
    DeviceGuard g(c->device);
    CK(c, hipStreamSynchronize(c->copy));
    if (c->vdec.s) CK(c, hipStreamSynchronize(c->vdec.s));
    CK(c, hipStreamSynchronize(c->stream));
    return PGH_OK;
}

}  // extern "C"

// ---- internals for the multi-GPU group driver (pgh_internal.h) ------------------------------------

namespace pgh_int {
int fail(pgh_ctx* c, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int r = vfail(c, code, fmt, ap);
    va_end(ap);
    return r;
}
pgh_group* group_of(const pgh_ctx* c) { return c ? c->grp : nullptr; }
pgh_ctx* new_group_ctx(pgh_group* g, int device) {
    auto* c = new pgh_ctx();
    c->grp = g;
    c->device = device;
    return c;
}
void free_group_ctx(pgh_ctx* c) { delete c; }
int device_of(const pgh_ctx* c) { return c->device; }
hipStream_t stream_of(const pgh_ctx* c) { return c->stream; }
int fixed_point_divisor(pgh_ctx* c, int base, int prec, float* div) { return pgh_detail::fixed_point_divisor(c, base, prec, div); }
int set_vec_min(pgh_ctx* c, int64_t n) {
    if (n < 0) return fail(c, PGH_E_ARG, "negative vector length");
    c->vec_min = n;
    if (c->layout) c->pvec = std::max((c->pg + 63) & ~(int64_t)63, (c->vec_min + 63) & ~(int64_t)63);
    return PGH_OK;
}
int set_copy_threads(pgh_ctx* c, int n) {
    n = std::max(1, n);
    if (n == c->copy_threads && c->pool_copy) return PGH_OK;
    c->copy_threads = n;
    c->pool_copy.reset(new CopyPool(n, c->local_cpus));
    return PGH_OK;
}
int set_shard_keep_opt(pgh_ctx* c, int64_t lo, int64_t hi) { return pgh_detail::set_shard(c, lo, hi, true); }
int set_client_base(pgh_ctx* c, int64_t base) {
    c->client_base = base;
    return PGH_OK;
}
void* vec(pgh_ctx* c, int which) {
    switch (which) {
    case V_CKPT: return c->d_ckpt.as<void>();
    case V_SUM: return c->d_sum.as<void>();
    case V_DEC: return c->d_dec.as<void>();
    default: return nullptr;
    }
}
}  // namespace pgh_int
