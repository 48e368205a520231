// The single-GPU context (struct pgh_ctx) and the helpers its entry points share.  Not installed;
// the public surface is include/pgh_api.h.
//
// The context's code is split by what it does:
//   pgh_api.cpp     lifecycle, errors and state checks, observability, the group driver's internals
//   pgh_host.cpp    host code free of HIP (pgh_host.h): non-temporal copy, copy pool, pre-faulting, the walk over
//                   host pieces (PieceCursor), the chunk arithmetic of ranged ingest, the rules' host steps; in the
//                   header alone, the per-slot state machine of a cached row reduction (SlotCache)
//   pgh_xfer.cpp    host <-> HBM: the pinned staging ring, the D2H rings, page-locked host blocks; the methods of
//                   the transfer owners.  Their state: pgh_xfer.h
//   pgh_order.cpp   which stream waits for what, and the timing events
//   pgh_ingest.cpp  host bytes -> HBM slab rows (raw, State messages, int64 shares, synthetic)
//   pgh_reduce.cpp  the one fp32 fold launch (fold_prepare, fold_launch), the fold over listed slots (fold_listed);
//                   fold_run's ring walk and the share sum; the divisors; the weights' upload; RESIDENT and STREAM
//                   entry points, the resident checkpoint
//   pgh_rules.cpp   what a mode may do (check_mode_use) and what the rules add to the fold: the row reductions (RowSums:
//                   K7 and K14 through their per-slot caches, K12 and K14 over listed rows, K13), clipping (the scales,
//                   the tallies) and the Gaussian noise on the clipped close (K11 behind a FINAL launch), trimming
//                   (K8's planes), the median (K9, K9p), the geometric median and the trust rule (the included rows
//                   and resident weights they share; the iterations; the root), the Multi-Krum selection; the -0
//                   plane; the rules' lifecycle calls (rules_*), the fold plans the two drivers ask for
//                   (rules_slot_plan, rules_resident_plan) and the entry points.  Their state: pgh_rules.h
//   pgh_serveropt.cpp  the server optimizer: K10 behind a FINAL launch, its planes, commit, download, upload
//   pgh_slots.cpp   report-time slot folds (the certain prefix of the close-time order): slot_fold
// A new averaging rule adds its state struct to pgh_rules.h (a member of pgh_ctx), its lines to the lifecycle
// functions rules_* in pgh_rules.cpp -- the one call each event of the context makes: made, slab freed, shard
// set, reserved, reset, slot written, row ingested, folds restarted, cycle finished -- and to the two plan
// functions, and touches check_mode_use, fold_prepare and fold_launch; both fold drivers (fold_run, slot_fold)
// ask for the plan and reach the kernels through the last two alone.  A row-wise rule takes its sums from RowSums
// (a new cached value per slot is one more RowCache there and one RowOp in pgh_rules.cpp), its finite rows from
// finite_rows into an IncludedRows, writes its weights through FoldWeights::replace and folds against the one -0
// plane (NegZeroPlane).  The server optimizer (pgh_set_server_opt) hangs on fold_launch too: a FINAL
// launch with one set is followed by K10 (server_opt_launch).  The noise (pgh_set_dp_noise) is a second tenant of
// that mechanism: a clipped FINAL launch with it set is followed by K11 (dp_noise_launch), ahead of K10.
// A new transfer feature adds its state struct to pgh_xfer.h (a member of pgh_ctx), its events and knobs to
// xfer_made -- the one call pgh_create makes -- and goes through the owners that keep the shared protocols: a
// staging slot is taken and handed back through StagingRing (take, sent), every data operation on the copy stream
// is counted through RangedIngest::copy_issued (what lets a close wait per ingest chunk), a page-locked table is
// rewritten through HostTable::upload, an H2D is accounted by an H2DTimer, a pre-queued D2H is dropped through
// D2HState::drop_pre.
// The context's HIP resources are held by the owners of pgh_res.h: `delete` releases them all.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/pgh_api.h"
#include "pgh_host.h"
#include "pgh_internal.h"
#include "pgh_kernels.h"
#include "pgh_res.h"
#include "pgh_rules.h"
#include "pgh_state.h"
#include "pgh_xfer.h"

namespace pgh_detail {

constexpr int KIND_SECAGG = PGH_STREAM_SECAGG;  // fold kind besides the pgh_mode values (none of which it equals)
static_assert(KIND_SECAGG != PGH_MEAN && KIND_SECAGG != PGH_ITERATIVE_MEAN && KIND_SECAGG != PGH_WEIGHTED_MEAN &&
                  KIND_SECAGG != PGH_CLIPPED_MEAN && KIND_SECAGG != PGH_TRIMMED_MEAN && KIND_SECAGG != PGH_MEDIAN && KIND_SECAGG != PGH_GEOMETRIC_MEDIAN &&
                  KIND_SECAGG != PGH_TRUSTED_MEAN,
              "the secagg fold kind must not collide with an averaging mode");

// CPUs on the GPU's own socket (its PCI device's local_cpulist) that this process may run on; empty
// when unknown.  Staging copies and pinned buffers there keep the host side of every H2D / D2H off
// the socket interconnect (a 2-socket node: GPUs 0-3 on one socket, 4-7 on the other).
std::vector<int> gpu_local_cpus(int device);

}  // namespace pgh_detail

struct pgh_ctx {
    using CopyPool = pgh_detail::CopyPool;
    pgh_group* grp = nullptr;  // set: a multi-GPU group (pgh_create_group); the rest is unused
    int device = 0;
    using Event = pgh_detail::Event; using Stream = pgh_detail::Stream;
    using DeviceBuf = pgh_detail::DeviceBuf; using PinnedBuf = pgh_detail::PinnedBuf;
    Stream stream;  // reductions
    Stream copy;    // ingest H2D and on-device synthetic fill
    Event copy_done;
    Event xsync;    // caller-stream <-> context-stream ordering
    Stream aux;     // second reduction stream: alternate ranges of a split FINAL pass
    Event aux_ev;
    // Every ordering event that comes and goes (fold_evs, slab_evs, slot_ring, marks, final_marks,
    // d2h.ev, ranged.ev) is lent by ev_pool; the timing pairs (pending) by timing_pool, whose events
    // keep hipEventDisableSystemFence (take_event).
    pgh_detail::EventPool ev_pool{hipEventDisableTiming}, timing_pool{hipEventDisableSystemFence};
    // The last fold issued on each stream (folds may run on several caller streams at once, e.g.
    // the param ranges of the multi-GPU overlap): the copy stream waits on all before it
    // overwrites slots, and then forgets them (later copies are ordered after those waits).
    std::vector<std::pair<hipStream_t, hipEvent_t>> fold_evs;
    // Folds that read every slab row (resident / stream / secagg): an ingest into any slot waits for
    // them.  Slot folds (pgh_fold_slots*) read only their listed slots: each is numbered, a slot
    // remembers the last one that read it, and an ingest into the slot waits for that fold alone --
    // a report's DMA does not queue behind a fold of other slots (a speculative re-fold).
    std::vector<std::pair<hipStream_t, hipEvent_t>> slab_evs;
    std::vector<int64_t> slot_read_seq;                     // per slot; 0 = not read by a slot fold
    std::deque<std::pair<int64_t, hipEvent_t>> slot_ring;  // recent slot folds on c->stream, in order
    int64_t slot_seq = 0;
    // STREAM: one event per fold with the fold front after it, so overwriting a slot waits only
    // for the fold that consumed the slot's previous client (not for the latest fold).
    struct FoldMark { hipEvent_t ev; int64_t upto; };
    std::deque<FoldMark> marks;

    std::vector<int64_t> numel;
    int64_t P = 0, lo = 0, hi = 0, pg = 0;
    int64_t pvec = 0;  // length of the [P_shard] device vectors: pg rounded up to 64
    bool layout = false;
    // slab geometry (pgh_reserve): bw columns per block, nb blocks, bstride elements per block
    int64_t bw = 0, nb = 0, bstride = 0;
    int bshift = 62;
    int64_t bmask = 0;
    size_t block_bytes = 256u << 10;  // PGH_BLOCK_BYTES; 0 = one block (plain row-major rows)
    int synth_kind = 0;        // pgh_set_synth_kind: generator of synthetic diffs (0 Irwin-Hall, 1 fast)

    int slots = 0, dtype = PGH_F32, parties = 1;
    DeviceBuf d_slab;
    DeviceBuf d_ckpt, d_out;  // float [pvec]
    // d_ckpt holds a checkpoint (uploaded, or the output of a resident fold); a fresh slab's is
    // uninitialised memory, which a resident fold / download / patch must refuse to read
    bool ckpt_valid = false;
    DeviceBuf d_acc, d_uacc, d_sum, d_dec;  // [pvec]: float, uint64, int64, float
    // iterative plan: rec[k] = 1 / (double)(float)(k + 1), grown on demand, kept for the context's
    // life (a superseded table may still be read by an in-flight fold: freed at destroy)
    DeviceBuf d_rec;  // double per client
    std::vector<DeviceBuf> rec_old;

    // The transfer side (pgh_xfer.h): touched only by their own code (pgh_xfer.cpp) and the call sites named there.
    pgh_detail::StagingRing ring;     // pageable host bytes -> HBM; lends its slots to a D2H without own cells
    pgh_detail::D2HState d2h;         // HBM -> host: the piped ring's stream and cells, the pre-queued ring
    pgh_detail::RangedIngest ranged;  // chunk events of the last report, the count of copy-stream operations
    pgh_detail::VarintDecode vdec;    // int64 shares: byte buffers, the decode stream
    pgh_detail::PinnedGather gather;  // page-locked fp32 State messages

    int copy_threads = 8;
    std::vector<int> local_cpus;  // PGH_NUMA (default on): the GPU's socket, for the copy pool + pinned ring
    std::unique_ptr<CopyPool> pool_copy;
    bool warmup_skipped = false;  // pgh_create's warm-up failed (e.g. no device memory left): skipped
    int64_t vec_min = 0;      // [P_shard] device vectors at least this long (group collectives)
    // Pipelined close: a resident fold's FINAL pass runs as final_split param ranges, each followed by
    // an event; a D2H of the new checkpoint (patch / download) then runs on the copy stream, piece by
    // piece behind the range that wrote it, so the HBM -> host copy overlaps the rest of the fold
    // (PGH_FINAL_RANGES, shards of >= 1 M params; opt-in, see final_split below).
    struct RangeMark { int64_t end; hipEvent_t ev; };
    std::vector<RangeMark> final_marks;
    // PGH_FINAL_RANGES (opt-in): split the FINAL pass of resident folds into this many param ranges
    // with marks, so a following D2H starts behind the first range.  Off by default: each extra
    // launch costs its drain (ResNet-18 fold 7.45 ms as 4 ranges on two streams vs 6.91 ms as one,
    // r02r), about what the earlier D2H start saves in a close (report closes within noise, r02l/r02r).
    int final_split = 1;
    int64_t client_base = 0;  // synthetic client k is generated as global client client_base + k

    std::vector<int64_t> slot_client;  // client held by each slot and not yet folded, or -1
    // The fold's weights: every writer replaces them through FoldWeights::replace, fold_prepare uploads them.
    pgh_detail::FoldWeights fw;

    // What the averaging rules and the server optimizer keep (pgh_rules.h): touched only by their own code
    // (pgh_rules.cpp, pgh_serveropt.cpp) and by fold_launch's lines for the optimizer and noise tenants.  The
    // lifecycle files (pgh_api.cpp, pgh_ingest.cpp, pgh_slots.cpp, pgh_xfer.cpp, pgh_order.cpp) reach them
    // through rules_* and the fold plans below alone:
    //   grep -n 'c->\(clip\|geo\|trust\|krum\|noise\|trim\|med\|opt\)\.' of those five files finds nothing.
    pgh_detail::RowSums rowsums;   // the per-slot caches sq (K7) and dot (K14), the tile partials and the buffers of K12 and K13 (clip, geo, krum, trust)
    pgh_detail::NegZeroPlane nz;   // the one plane of -0.0f (opt, noise, geo)
    pgh_detail::ClipState clip;
    pgh_detail::NoiseState noise;
    pgh_detail::TrimState trim;
    pgh_detail::MedianState med;
    pgh_detail::GeomedState geo;
    pgh_detail::TrustState trust;
    pgh_detail::KrumState krum;
    pgh_detail::ServerOptState opt;

    bool streaming = false;
    int slot_mode = -1;  // pgh_fold_slots: averaging mode of the cycle being folded slot by slot
    int kind = 0;
    int fold_batch = 1;
    int64_t folded = 0;  // stream: clients [0, folded) are in the running state

    int variant = PGH_DEFAULT_VARIANT;
    struct Timed { hipEvent_t a, b; uint64_t bytes; };
    std::vector<Timed> pending;
    pgh_stats_t st{};
    std::string err;
};

#define CK(c, expr)                                                                            \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((c), PGH_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

#define RC(expr)            \
    do {                    \
        int r_ = (expr);    \
        if (r_) return r_;  \
    } while (0)

namespace pgh_detail {

// ---- errors, device selection, time ------------------------------------------------------------
// Set the context's (or, with c == NULL, the calling thread's creation) error message; returns code.
int fail(pgh_ctx* c, int code, const char* fmt, ...);
int vfail(pgh_ctx* c, int code, const char* fmt, va_list ap);

struct DeviceGuard {  // select the context's GPU for the call, restore the caller's after
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

double now_ms();

// ---- state checks and slab geometry -------------------------------------------------------------
inline size_t esize(int dtype) { return dtype == PGH_F32 ? 4 : 8; }
inline bool valid_mode(int m) {  // (pgh_effective_variant's alone: check_mode_use has its own switch)
    return m == PGH_MEAN || m == PGH_ITERATIVE_MEAN || m == PGH_WEIGHTED_MEAN || m == PGH_CLIPPED_MEAN ||
           m == PGH_TRIMMED_MEAN || m == PGH_MEDIAN || m == PGH_GEOMETRIC_MEDIAN || m == PGH_TRUSTED_MEAN;
}
static_assert(PGH_TRUSTED_MEAN == 7, "the mode numbers are ABI: engine.py and every caller hold them as integers");
static_assert(PGH_TRIMMED_MEAN == pgh::MODE_TRIMMED && PGH_TRIM_MAX == pgh::TRIM_MAX, "the kernels' numbering");
static_assert(PGH_MEDIAN == pgh::MODE_MEDIAN && PGH_MEDIAN_NCHIP == pgh::MEDIAN_NCHIP, "the kernels' numbering");
// The kernels' mode: a clipped mean is the weighted fold with the scales as weights, a geometric median the
// weighted fold with the last Weiszfeld weights, a trusted mean the weighted fold with the trust weights.
inline int kernel_mode(int m) {
    return m == PGH_CLIPPED_MEAN || m == PGH_GEOMETRIC_MEDIAN || m == PGH_TRUSTED_MEAN ? PGH_WEIGHTED_MEAN : m;
}
// May `mode` be folded this way on this context?  The one place that says so, in this order: an unknown
// mode (PGH_E_ARG); a rule that the use or a group cannot serve -- a stream neither clips, trims nor
// takes a median, a median folds nothing early, a group does not clip (PGH_E_UNSUPPORTED); a rule whose
// bound or trim count is not set (PGH_E_STATE; a group leaves that to its children).
enum ModeUse { USE_RESIDENT, USE_STREAM, USE_SLOT_EARLY, USE_SLOT_FINAL };
int check_mode_use(pgh_ctx* c, int mode, ModeUse use);
int check_ready(pgh_ctx* c);
int check_dtype(pgh_ctx* c, int dtype);
int check_ckpt(pgh_ctx* c, const char* what);
// Every listed slot is inside the slab and holds an unfolded diff; no_twice: and none is listed twice.
int check_slot_list(pgh_ctx* c, const int32_t* slots, int n, bool no_twice);
// A host vector of nbytes given as the whole model or as this shard alone, `unit` bytes per param: *first =
// the param of it at which this shard's part starts.  Any other length: PGH_E_ARG, `what` leading the message.
int shard_start(pgh_ctx* c, const char* what, size_t nbytes, size_t unit, size_t* first);
void free_slab(pgh_ctx* c);

// Slab geometry for kernels (off = 0) and the start of a slot's first row inside block 0.
inline pgh::SlabMap slab_map(const pgh_ctx* c) { return pgh::SlabMap{c->bw, c->bstride, c->bshift, c->bmask, 0}; }
inline uint8_t* slot_row(pgh_ctx* c, int slot, int party) {
    const size_t row = (size_t)slot * c->parties + party;
    return c->d_slab.as<uint8_t>() + row * (size_t)c->bw * esize(c->dtype);
}

// Where host bytes land: a slab row (blocked) or a [p] vector (one block).
struct Dest {
    uint8_t* base;       // row start in block 0 / vector start
    pgh::SlabMap map;
    size_t es;
    int64_t len = 0;     // a slab row: its elements (the last block's columns past it are padding)
};
inline Dest row_dest(pgh_ctx* c, int slot, int party) {
    return Dest{slot_row(c, slot, party), slab_map(c), esize(c->dtype), c->pg};
}
inline Dest vec_dest(void* v, int64_t n, size_t es) { return Dest{(uint8_t*)v, pgh::single_block(n), es}; }

// ---- kernel timing -------------------------------------------------------------------------------
hipEvent_t take_event(pgh_ctx* c);
int collect_timings(pgh_ctx* c);

// Bracket a launch with an event pair on `s`.
template <class F>
int timed_launch(pgh_ctx* c, hipStream_t s, uint64_t bytes, F&& launch) {
    if (c->pending.size() >= 4096) RC(collect_timings(c));
    hipEvent_t a = take_event(c), b = take_event(c);
    if (!a || !b) return fail(c, PGH_E_HIP, "hipEventCreate failed");
    CK(c, hipEventRecord(a, s));
    hipError_t e = launch();
    if (e != hipSuccess) {
        c->timing_pool.give(a); c->timing_pool.give(b);
        return fail(c, PGH_E_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    }
    CK(c, hipEventRecord(b, s));
    c->pending.push_back({a, b, bytes});
    return PGH_OK;
}

// ---- host <-> HBM --------------------------------------------------------------------------------
// (D2H_PIECE and INGEST_CHUNK, with the chunk arithmetic of ranged ingest: pgh_host.h)
// The two owner methods on the per-piece loops.
inline int StagingRing::sent(pgh_ctx* c, int slot, hipStream_t s) {
    CK(c, hipEventRecord(ev[slot], s));
    used[slot] = true;
    return PGH_OK;
}
inline int RangedIngest::mark(pgh_ctx* c, int k) {
    CK(c, hipEventRecord(ev[(size_t)k], c->copy));
    return PGH_OK;
}
// The accounting of one H2D: made where it starts; done, on success alone, adds the elapsed host time, the
// bytes moved and those of them that went through the staging ring.
struct H2DTimer {
    pgh_ctx* c;
    double t0;
    explicit H2DTimer(pgh_ctx* c_) : c(c_), t0(now_ms()) {}
    int done(size_t bytes, size_t staged = 0) {
        c->st.h2d_ms_total += now_ms() - t0;
        c->st.h2d_bytes_total += bytes;
        c->st.h2d_staged_bytes_total += staged;
        return PGH_OK;
    }
};

bool is_pinned(const void* p);
// src_room: bytes readable at src past the n elements (a staging slot's unused rest); a range that
// ends a slab row whose last block is partial then goes as full blocks in one 2D copy (the padding
// columns take whatever follows in the slot) instead of a 2D copy plus a tail copy.
int h2d_range(pgh_ctx* c, const Dest& d, int64_t i0, const uint8_t* src, int64_t n, hipStream_t s,
              size_t src_room = 0);
int stage_pieces_h2d(pgh_ctx* c, const Dest& dst, const std::vector<Piece>& pieces);
int stage_pieces_h2d_ranged(pgh_ctx* c, const Dest& dst, const std::vector<Piece>& pieces, size_t total);
int stage_h2d(pgh_ctx* c, const Dest& dst, const uint8_t* src, size_t n, bool pinned_src);
int stage_d2h_pieces(pgh_ctx* c, const uint8_t* src, const std::vector<OutPiece>& pieces, hipStream_t s,
                     const std::function<void()>& overlap = nullptr, bool marks = false);
// may_wait = false: both pinned slots still busy -> r->n_free == 0 (nothing set up) instead of waiting
int d2h_ring_begin(pgh_ctx* c, D2HRing* r, const uint8_t* src, size_t total, hipStream_t s, bool piped,
                   bool may_wait = true);
int state_shard_spans(pgh_ctx* c, const uint8_t* pb, size_t n, std::vector<std::pair<size_t, size_t>>* out,
                      const char* what);
// page-locked blocks marked async (pgh_host_async): DMAs from them are recorded, not waited for
bool host_async(const void* p, size_t n);
int host_dma_queued(pgh_ctx* c, const void* p, size_t n, hipStream_t s);

// ---- ordering between ingest copies and folds -----------------------------------------------------
int order_after_ingest(pgh_ctx* c, hipStream_t s);
void release_slot_fold_events(pgh_ctx* c);
int record_slot_fold(pgh_ctx* c, const int32_t* slots, int n);
int order_slot_overwrite(pgh_ctx* c, int slot);
int order_before_overwrite(pgh_ctx* c);
// the fold just issued on stream s joins `evs`: fold_evs, or slab_evs for one reading every slab row
int record_fold(pgh_ctx* c, std::vector<std::pair<hipStream_t, hipEvent_t>>& evs, hipStream_t s);
void clear_marks(pgh_ctx* c);
int order_stream_overwrite(pgh_ctx* c, int64_t last_client);
int record_mark(pgh_ctx* c, hipStream_t s, int64_t upto);
int join_in(pgh_ctx* c, hipStream_t cs);
int join_out(pgh_ctx* c, hipStream_t cs);

// ---- pipelined close: range marks of the last resident fold -----------------------------------------
void clear_final_marks(pgh_ctx* c);
int add_final_mark(pgh_ctx* c, hipStream_t s, int64_t end);
hipStream_t range_stream(const pgh_ctx* c, hipStream_t s, int k);
int fork_aux(pgh_ctx* c, hipStream_t s);
int join_aux(pgh_ctx* c, hipStream_t s);
int final_ranges(const pgh_ctx* c);
int64_t range_edge(const pgh_ctx* c, int k, int K);

// ---- folds ---------------------------------------------------------------------------------------
int fixed_point_divisor(pgh_ctx* c, int base, int prec, float* div);
int fedavg_divisor(pgh_ctx* c, int mode, int64_t n, float* div);

// ---- the rules at the context's lifecycle events (pgh_rules.cpp): the one call each event's site makes ----
bool rules_made(pgh_ctx* c);         // pgh_create: PGH_TRIM_VEC, PGH_MEDIAN_PATH, the rules' events; false fails it
void rules_slab_freed(pgh_ctx* c);   // free_slab: every buffer and cache sized by the slab or the shard goes
// set_shard, before the context takes [lo, hi) and pvec.  keep_opt: the optimizer's setting and state stay when
// neither the shard nor the length of the [P_shard] vectors changes; a sub-range shard clears the clipping bound
void rules_shard_set(pgh_ctx* c, int64_t lo, int64_t hi, int64_t pvec, bool keep_opt);
void rules_reserved(pgh_ctx* c, int slots);  // pgh_reserve: the per-slot caches at their new length
void rules_reset(pgh_ctx* c);                // pgh_reset: the cycle's sums, scales, tallies
// The diffs of slots [slot, slot + n) are about to be replaced (claim_slot, the synthetic fill).  The fill's
// runs begin with a claim_slot on a RESIDENT slab, and a STREAM slab never has valid resident scales
// (pgh_stream_begin resets; only a resident clipped fold sets them), so clearing them here for every slot of
// a run changes nothing a caller can see.
void rules_slot_written(pgh_ctx* c, int slot, int n = 1);
void rules_folds_restarted(pgh_ctx* c);         // pgh_fold_slots_restart (the caller clears the weights)
void rules_cycle_finished(pgh_ctx* c, int mode);  // a slot close: a clipped cycle's rows join the finished totals
int rules_row_ingested(pgh_ctx* c, int slot);   // the tail of an fp32 ingest: a rule that wants norms queues the row's K7

// What a fold driver asks the rules before its launches: which rows the fold of `mode` takes and with what.
// For PGH_MEAN, ITERATIVE, WEIGHTED, TRIMMED and MEDIAN (and a share sum) the plan is the input unchanged and
// nothing is launched.  A clipped fold gets its scales as the weights (K7 for the sums still missing); a
// geometric median its included rows, their final weights and W (the inner iterations are finished on return); a
// trusted mean its included rows, their trust weights and the divisor 1 (K7 and K14 for what is still missing).
struct FoldPlan {
    const int32_t* slots = nullptr;  // the rows to fold, in order: the given ones or the included ones.
                                     // rules_resident_plan: null = clients [0, n) where the slab holds them
    int n = 0;
    int64_t total = 0;               // the cycle's clients for fold_prepare, this fold included
    bool has_divisor = false;        // the rule supplies the FINAL divisor
    float divisor = 1.f;
    bool whole_rows = false;         // the rule read every row landed whole: no ranged wait
};
int rules_slot_plan(pgh_ctx* c, int mode, const int32_t* slots, int n, int64_t c0, FoldPlan* p);  // slot_fold
int rules_resident_plan(pgh_ctx* c, int mode, int64_t c0, int64_t n, FoldPlan* p);                // fold_run
// A rule that closes a cycle in one slot fold only (median, geometric median, trusted mean): its name for the refusal; else null.
const char* rules_one_fold_cycle(int mode);
int trim_divisor(pgh_ctx* c, int64_t n, float* div);  // n - 2b; PGH_E_STATE with fewer than 2b + 1 diffs

// ---- the row walker of RowSums and of every fold over listed slots ---------------------------------------
// f(rows, k0, m) for each run of the listed slots a launch can take: all of them when they are consecutive,
// else RowTabs of at most ROWTAB_MAX; k0 = the index in the list of the run's first row.
template <class F>
int for_row_runs(pgh_ctx* c, const int32_t* slots, size_t n, F&& f) {
    bool run = true;
    for (size_t k = 0; k < n; ++k) run = run && slots[k] == slots[0] + (int32_t)k;
    if (run) return f(pgh::Rows{nullptr, nullptr, slots[0] * c->parties}, (size_t)0, n);
    for (size_t done = 0; done < n; done += pgh::ROWTAB_MAX) {
        const size_t m = std::min(n - done, (size_t)pgh::ROWTAB_MAX);
        pgh::RowTab tab;
        for (size_t k = 0; k < m; ++k) tab.rows[k] = slots[done + k] * c->parties;
        RC(f(pgh::Rows{&tab}, done, m));
    }
    return PGH_OK;
}

// ---- clipped FedAvg (pgh_rules.cpp) ----------------------------------------------------------------
inline bool clip_on(const pgh_ctx* c) { return c->clip.c > 0.f && c->dtype == PGH_F32 && !c->streaming; }
// scale = norm <= C ? 1 : (float)(C / norm), norm = sqrt(sumsq) in f64 (IEEE: NaN -> NaN, inf -> 0)
float clip_scale_of(double sumsq, float c);

// ---- geometric-median FedAvg (pgh_rules.cpp) ---------------------------------------------------------
inline bool geomed_on(const pgh_ctx* c) { return c->geo.iters > 0 && c->dtype == PGH_F32 && !c->streaming; }
// ---- trust-bootstrapped FedAvg (pgh_rules.cpp) ---------------------------------------------------------
inline bool trust_on(const pgh_ctx* c) { return c->trust.on && c->dtype == PGH_F32 && !c->streaming; }
// K7 behind every ingest: clipping, the geometric median or the trust rule is on
inline bool norms_wanted(const pgh_ctx* c) { return clip_on(c) || geomed_on(c) || trust_on(c); }

// ---- Gaussian noise on the clipped close (pgh_rules.cpp) ---------------------------------------------
inline bool noise_on(const pgh_ctx* c) { return c->noise.z > 0.f; }
// A FINAL fp32 fold of `mode` is about to be issued: with noise on only PGH_CLIPPED_MEAN may close a cycle
// (PGH_E_STATE before anything is launched; an un-noised average never leaves a context that noise is set on).
int check_noise_final(pgh_ctx* c, int mode);
int noise_plane(pgh_ctx* c);  // the delta plane of a noised FINAL without a server optimizer, allocated on first use
struct FinalArgs;
// K11 behind a FINAL clipped launch of n clients over [fa.off, fa.off + fa.len) on stream s.  into_opt: the
// fold wrote the server optimizer's delta plane and K10 follows -- K11 noises that plane in place; else it
// reads the noise state's plane and writes the real out = ckpt - g'.
int dp_noise_launch(pgh_ctx* c, const FinalArgs& fa, int64_t n, bool into_opt, hipStream_t s);

// ---- trimmed-mean FedAvg (pgh_rules.cpp) ------------------------------------------------------------
// K8's arguments on top of a filled FedavgArgs (map.off = the launch's first shard param): the mode,
// b, the column width and -- unless the launch is FIRST and FINAL -- the state planes, allocated here.
int trim_args(pgh_ctx* c, pgh::FedavgArgs* a);
// HBM bytes of K8's state a launch with these flags moves over rp params
inline uint64_t trim_state_bytes(const pgh_ctx* c, int flags, uint64_t rp) {
    const uint64_t planes = 2ull * (uint64_t)c->trim.b;  // (the acc plane is counted like the other modes')
    return ((flags & pgh::FL_FIRST) ? 0 : 4 * planes * rp) + ((flags & pgh::FL_FINAL) ? 0 : 4 * planes * rp);
}
// The form a trimmed fold takes: 40 (K8, 4 columns per lane) or 41 (1 column), whatever pgh_set_variant says.
inline int trim_variant(const pgh_ctx* c) {
    return (c->trim.vec ? c->trim.vec : pgh::auto_trim_vec(c->pg, c->trim.b)) == 4 ? 40 : 41;
}

// ---- median FedAvg (pgh_rules.cpp) -------------------------------------------------------------------
// The path a median fold of n rows takes: 50 (K9, on chip) or 51 (K9p, one pass per bit).
inline int median_variant(const pgh_ctx* c, int64_t n) { return c->med.passes || n > pgh::MEDIAN_NCHIP ? 51 : 50; }
// The whole median fold of a filled FedavgArgs (diffs, map, n_rows, p, ckpt, out; every row of the
// cycle) on stream s: K9's one launch or K9p's 32 or 33.
int median_fold(pgh_ctx* c, const pgh::FedavgArgs& a, const pgh::Rows& rows, hipStream_t s);
// slots[k] * parties for k < n, uploaded to d_rowidx on stream s (waits for the copy)
int median_row_table(pgh_ctx* c, const int32_t* slots, int n, hipStream_t s);
inline const int32_t* median_rows(const pgh_ctx* c) { return c->med.d_rowidx.as<int32_t>(); }  // that table

// ---- server optimizer (pgh_serveropt.cpp) --------------------------------------------------------------
struct FinalArgs;
int server_opt_launch(pgh_ctx* c, const FinalArgs& fa, hipStream_t s);  // K10 behind a FINAL launch (fold_launch)
// pgh_set_shard; keep_opt (rules_shard_set): a group's pgh_reserve lays its children's shards out again
int set_shard(pgh_ctx* c, int64_t lo, int64_t hi, bool keep_opt);

// What a FINAL fold pass writes (fedavg: ckpt - avg; secagg: sum/dec) and over which param range.
struct FinalArgs {
    const float* ckpt = nullptr;  // shard base pointers; the launch touches [off, off + len)
    float* out = nullptr;
    int64_t* sum = nullptr;
    float* dec = nullptr;
    float divisor = 1.f;
    int64_t off = 0;   // param range within the shard
    int64_t len = -1;  // -1 = to the end of the shard
    bool plain = false;  // a FINAL that is an inner step (the geometric median's iterate): no K10 / K11 behind it
};
// The two steps every fp32 fold driver takes (fold_run, slot_fold; nothing else calls them).
// Before the launches of a fold that brings the cycle to `total` clients, on the fold's stream: the
// weights of all of them on the device (weighted, clipped, geometric median: FoldWeights::upload), the reciprocal
// table covering them (iterative).
int fold_prepare(pgh_ctx* c, int mode, int64_t total, hipStream_t s);
// The rows of one launch: n contiguous slab rows from `diffs`, or, with diffs = the slab at row 0,
// the rows of a RowTab or (a median of more rows than a RowTab carries) of a device table.
struct FoldRows {
    const float* diffs;
    int n;
    pgh::Rows src;
};
// One launch (the median: all of its launches) of `mode` over the shard params [fa.off, fa.off + fa.len)
// on stream s, timed and accounted; client0 = the fold index of row 0.
int fold_launch(pgh_ctx* c, int mode, const FoldRows& rows, int64_t client0, int flags, const FinalArgs& fa, hipStream_t s);
// One launch per run of the listed slots (for_row_runs) of `mode` over [fa.off, fa.off + fa.len) on stream s:
// FIRST on the first, FINAL (when `final`) on the last; fold client k = the k-th listed slot.
int fold_listed(pgh_ctx* c, int mode, const int32_t* slots, size_t n, bool final, const FinalArgs& fa, hipStream_t s);
int fold_run(pgh_ctx* c, int kind, int64_t c0, int64_t n, bool final, const FinalArgs& fa, hipStream_t s);
int64_t ready_run(pgh_ctx* c, int64_t from);
int check_no_gaps(pgh_ctx* c, int64_t from, int64_t run);
int maybe_fold(pgh_ctx* c, bool force);
int claim_slot(pgh_ctx* c, int64_t client, int* slot_out);
int mark_ingested(pgh_ctx* c, int64_t client, int slot);
int resident_count(pgh_ctx* c, int64_t* n_out);

}  // namespace pgh_detail
