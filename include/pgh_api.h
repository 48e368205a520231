/* libpygrid_hip -- C ABI of the MI355X (gfx950) aggregation engine behind PyGrid Node's
 * model-centric cycle close.
 *
 * What it replaces (reference = /root/reference, read-only):
 *   CycleManager._average_plan_diffs, apps/node/src/app/main/model_centric/cycles/
 *   cycle_manager.py:219-323, the slice :240-303 -- checkpoint unserialize (:240), per-diff
 *   unserialize (:247-250), hosted iterative avg plan (:266-269), hard-coded mean
 *   (:276-288), apply (:293-296) -- plus the PySyft 0.2.9 Z_2^64 share sum + fixed-point
 *   decode exercised by tests/data_centric/test_basic_syft_operations.py:388-454.
 *   The reference has no FFI of its own; this ABI is what a ctypes binding in the node
 *   process binds (INTEGRATION.md shows the stub).
 *
 * Conventions: every int-returning entry point returns PGH_OK (0) or a negative pgh_status;
 * pgh_last_error() then holds the message.  Plain pointers and sizes only.  Host buffers
 * passed in are borrowed for the duration of the call.  A context is single-owner and not
 * re-entrant (the reference serialises cycle close with run_task_once,
 * apps/node/src/app/main/model_centric/tasks/cycle.py:9-25).  A context drives one GPU
 * (pgh_create) or several GPUs of one node from one process (pgh_create_group); the
 * alternative is one process (and one context) per GPU, each owning a parameter shard.
 */
#ifndef PGH_API_H
#define PGH_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_ABI_VERSION 10

typedef struct pgh_ctx pgh_ctx;

typedef enum {
    PGH_OK = 0,
    PGH_E_ARG = -1,        /* bad argument (null, size mismatch, out of range) */
    PGH_E_HIP = -2,        /* HIP runtime / kernel launch error */
    PGH_E_STATE = -3,      /* call order / missing clients / layout not set */
    PGH_E_OOM = -4,        /* device or pinned allocation failed */
    PGH_E_PARSE = -5,      /* malformed State protobuf bytes */
    PGH_E_UNSUPPORTED = -6
} pgh_status;

/* Averaging mode.  PGH_MEAN: hard-coded path, cycle_manager.py:276-288.
 * PGH_ITERATIVE_MEAN: hosted iterative avg_plan, cycle_manager.py:266-269 with the plan of
 * examples/model-centric/01-Create-plan.ipynb:450-454.  PGH_WEIGHTED_MEAN: north_star's
 * weighted FedAvg (no reference counterpart; equals PGH_MEAN bit for bit at w == 1).
 * PGH_CLIPPED_MEAN: the mean of the diffs after each is scaled down to an L2 norm of at most the
 * bound of pgh_set_clip_norm (norm-bounded FedAvg; no reference counterpart; equals PGH_MEAN bit for
 * bit when no diff exceeds the bound).
 * PGH_TRIMMED_MEAN: per parameter, the mean of the N reported values without the b largest and the
 * b smallest (coordinate-wise trimmed mean, Yin et al. 2018; b from pgh_set_trim; no reference
 * counterpart).
 * PGH_MEDIAN: per parameter, the median of the N reported values (coordinate-wise median, Yin et al.
 * 2018; no parameter; no reference counterpart; defined below, before the reductions).
 * PGH_GEOMETRIC_MEDIAN: the smoothed Weiszfeld approximation of the geometric median of the N diffs
 * (Pillutla, Kakade, Harchaoui, "Robust Aggregation for Federated Learning"; settings from
 * pgh_set_geomed; no reference counterpart; defined below).
 * PGH_TRUSTED_MEAN: FLTrust (Cao, Fang, Liu, Gong, NDSS 2021): every diff rescaled to the norm of a server
 * root update and weighted by its clipped cosine to it (pgh_set_trust, pgh_trust_root; no reference
 * counterpart; defined below). */
typedef enum {
    PGH_MEAN = 0,
    PGH_ITERATIVE_MEAN = 1,
    PGH_WEIGHTED_MEAN = 2,
    PGH_CLIPPED_MEAN = 3,
    PGH_TRIMMED_MEAN = 4,
    PGH_MEDIAN = 5,
    PGH_GEOMETRIC_MEDIAN = 6,
    PGH_TRUSTED_MEAN = PGH_GEOMETRIC_MEDIAN + 1 /* mode 7 */
} pgh_mode;
/* Stream kind for pgh_stream_begin besides the three averaging modes. */
#define PGH_STREAM_SECAGG 16

typedef enum { PGH_F32 = 0, PGH_I64 = 1 } pgh_dtype;

typedef struct {
    double kernel_ms_last;     /* duration of the last reduction kernel (HIP events) */
    double kernel_ms_total;    /* sum over timed launches since the last reset */
    uint64_t kernel_launches;  /* timed launches since the last reset */
    uint64_t kernel_bytes_last;/* algorithmic bytes of the last reduction launch */
    uint64_t kernel_bytes_total;/* algorithmic bytes over timed launches since the last reset */
    double h2d_ms_total;       /* ingest wall time (host buffer -> HBM), ms */
    uint64_t h2d_bytes_total;  /* bytes moved host -> HBM by ingest */
    double close_ms_last;      /* wall time of the last pgh_fedavg / pgh_secagg (host in/out) */
    int64_t p_shard;           /* params in this context's shard */
    int64_t ld;                /* slab block width = row stride inside a block (elements) */
    int64_t n_folded;          /* stream mode: clients folded into the running state */
    int32_t n_clients;         /* clients ingested since the last reset */
    int32_t max_clients;       /* slab capacity (slots) */
    double kernel_busy_ms_total;/* union of the timed launches' [start, end] intervals: launches
                                 * running concurrently on several streams count once */
    uint64_t h2d_staged_bytes_total; /* of h2d_bytes_total: bytes host threads first copied into
                                 * the pinned staging ring (pageable sources); page-locked sources
                                 * (pgh_host_alloc) are DMA'd as they lie and do not count */
    uint64_t d2h_bytes_total;   /* ABI 10: bytes moved HBM -> host through the D2H ring (results) */
    uint64_t d2h_kernel_bytes_total; /* ABI 10: of d2h_bytes_total, moved by a kernel instead of an
                                 * SDMA copy -- 0 since K6 k_copy_to_host was removed (r06s: it
                                 * read FINAL ranges before they had run); kept for the layout */
} pgh_stats_t;

/* ---- context lifecycle ------------------------------------------------------------------ */
int pgh_abi_version(void);
int pgh_device_count(int* n);
/* Bind a context to GPU `device`, with a pinned host staging ring of `pinned_bytes` total
 * (0 = default 256 MiB, split into 2 slots).  Also warms the device up (one small kernel launch
 * and a host -> HBM -> host copy; PGH_WARMUP=0 skips it) so the node's first cycle close does not
 * pay for the code-object load and the copy engines' first use. */
int pgh_create(int device, size_t pinned_bytes, pgh_ctx** out);
void pgh_destroy(pgh_ctx* ctx);

/* ---- several GPUs of one node in ONE process ----------------------------
 * The node closes a cycle from one thread of one process (apps/node/src/app/__init__.py:196-199,
 * tasks/cycle.py:9-25), so the library itself drives every GPU: one context over n_gpus GPUs
 * (devices[i], or 0 .. n_gpus - 1 when devices is NULL), one child context and one host thread per
 * GPU.  The parameter axis is cut into contiguous 64-aligned shards, one per GPU; each GPU holds
 * every client for its shard, so every ingest sends each GPU its slice over its own PCIe link,
 * every fold runs on all GPUs at once, host outputs are written slice by slice, and fp32 results
 * are bit-identical to one GPU.  Secure aggregation may shard the CLIENTS instead
 * (pgh_set_client_sharding before pgh_reserve of an int64 slab): client k lives on GPU
 * k / ceil(max_clients / n_gpus), each GPU sums its clients over the whole model, the Z_2^64 sums
 * are reduce-scattered (ncclReduceScatter, uint64 SUM: exact) and each GPU decodes its slice.
 * Every entry point above and below accepts a group context, except the ones taking device
 * pointers or returning slab geometry (PGH_E_UNSUPPORTED: they name one GPU -- call them on
 * pgh_group_child).  Collectives go over RCCL (librccl.so.1, loaded at first use: ncclCommInitAll
 * over the group's devices) when the devices are distinct, else (or with PGH_RCCL=0) over peer
 * copies. */
int pgh_create_group(int n_gpus, const int* devices, size_t pinned_bytes, pgh_ctx** out);
int pgh_group_size(const pgh_ctx* ctx, int* n);              /* 1 for a single-GPU context */
int pgh_group_child(pgh_ctx* ctx, int i, pgh_ctx** child);    /* borrowed context of GPU i */
int pgh_set_client_sharding(pgh_ctx* ctx, int on);
/* All-gather the resident checkpoint into a full copy on every GPU (ncclAllGather of equal shards
 * of S = ceil(P / n_gpus) rounded up to 64 floats, or peer copies): GPU g's copy holds shard r at
 * [r * S, r * S + len_r).  d_full_out (nullable) receives one device pointer per GPU. */
int pgh_group_allgather_resident(pgh_ctx* ctx, void** d_full_out);
/* The exchange in use: 1 RCCL, 0 peer copies, -1 none yet (or not a group). */
int pgh_group_backend(pgh_ctx* ctx, int* rccl);
const char* pgh_last_error(const pgh_ctx* ctx);   /* ctx may be NULL (creation errors) */
/* Page-locked host buffers: ingest DMAs them straight to HBM (no staging copy). */
int pgh_host_alloc(size_t bytes, void** out);
int pgh_host_free(void* p);
/* Mark (on = 1) a pgh_host_alloc block of n bytes as ASYNC: an ingest of State bytes lying in it
 * returns once its DMA is queued instead of waiting for it, so the caller must pgh_host_wait(p, n)
 * before writing to or reusing the block (pgh_host_free waits by itself).  on = 0 waits, then
 * unmarks.  Unmarked page-locked memory keeps the synchronous contract. */
int pgh_host_async(void* p, size_t n, int on);
/* Wait for every DMA still reading host memory [p, p + n), queued by any context. */
int pgh_host_wait(const void* p, size_t n);
/* Fault in the pages of a (fresh, pageable) host buffer now, on up to 8 threads, so that a later
 * copy into it -- the new checkpoint's payloads at a cycle close -- takes no page faults.  Best
 * effort (Linux 5.14+ MADV_POPULATE_WRITE); always returns PGH_OK for a valid range. */
int pgh_host_prefault(void* p, size_t n);

/* ---- layout ------------------------------------------------------------------------------
 * Flat parameter vector = tensors concatenated in State order
 * (model_manager.py:94-103 state.tensors()); P = sum(numel). */
int pgh_set_layout(pgh_ctx* ctx, int n_tensors, const int64_t* numel);
/* Restrict this context to the flat range [lo, hi) (param-axis shard).  Default: [0, P). */
int pgh_set_shard(pgh_ctx* ctx, int64_t lo, int64_t hi);
/* Allocate the HBM slab: max_clients slots of the shard, dtype PGH_F32 (fp32 diffs) or
 * PGH_I64 (n_parties int64 share rows per client).  Forgets previously ingested clients.
 * RESIDENT use: client k lives in slot k (k < max_clients).  STREAM use (pgh_stream_begin):
 * client k goes to slot k % max_clients, so the slab is a ring and N may exceed it. */
int pgh_reserve(pgh_ctx* ctx, int max_clients, int dtype, int n_parties);
/* Forget ingested clients and weights (start of a new cycle); keeps allocations. */
int pgh_reset(pgh_ctx* ctx);

/* ---- ingest (the diffs of cycle_manager.py:243-250) -------------------------------------- */
/* Client `client`'s already-decoded flat diff.  PGH_F32: `flat` holds P float32 (the whole
 * model; the shard slice is taken) or P_shard float32 (this shard only).  PGH_I64: n_parties x
 * P (or x P_shard) int64 shares, party-major.  Pageable memory is staged through the pinned
 * ring; page-locked memory (pgh_host_alloc, hipHostRegister) is DMA'd directly. */
int pgh_ingest_raw(pgh_ctx* ctx, int client, const void* flat, size_t nbytes, int dtype);
/* Client diff as syft State protobuf bytes (model_manager.py:94-103 wire format, build-owned
 * schema restatement: DESIGN.md "State codec"); fp32 tensors only. */
int pgh_ingest_state(pgh_ctx* ctx, int client, const uint8_t* pb, size_t n);
/* One client's secure-aggregation shares as State bytes, one message per party (n_parties ==
 * the parties of pgh_reserve): every tensor a packed-varint contents_int64 payload, the State
 * order of pgh_set_layout (PySyft 0.2.9 int64 share tensors, test_basic_syft_operations.py:
 * 388-454; wire schema restated, parity unpinned like pgh_ingest_state).  The payload bytes go
 * to HBM as they are (PCIe carries the varints) and are decoded there (k_varint_decode); the
 * host only checks the framing, counts the values per 16 KiB chunk and rejects varints longer
 * than 10 bytes, cut-off payloads and count/layout mismatches (PGH_E_PARSE). */
int pgh_ingest_state_shares(pgh_ctx* ctx, int client, int n_parties, const uint8_t* const* pbs, const size_t* ns);
/* Fill slab rows [0, n_clients) with the deterministic synthetic diffs (or shares) of
 * SURVEY.md 8(d) for this shard, generated on the GPU (oracle/oracle.py restates them). */
int pgh_synth_fill(pgh_ctx* ctx, uint64_t seed, int n_clients);
/* Generator of the synthetic fp32 diffs for later pgh_synth_fill / pgh_synth_ingest calls:
 * 0 = one splitmix64 word per param, Irwin-Hall(4 x u16) (default); 1 = one word
 * per 4 params, a u16 each, uniform (config 4's on-device data source: write-bound instead of
 * integer-bound).  Both restated bit for bit by oracle/oracle.py. */
int pgh_set_synth_kind(pgh_ctx* ctx, int kind);
/* Ingest synthetic clients [client0, client0 + n) generated on the GPU (either use). */
int pgh_synth_ingest(pgh_ctx* ctx, uint64_t seed, int client0, int n);
/* Per-client weights for PGH_WEIGHTED_MEAN (n == clients ingested at reduction time). */
int pgh_set_weights(pgh_ctx* ctx, const float* w, int n);

/* ---- per-client L2 clipping (PGH_CLIPPED_MEAN) -----------------------------------------------
 * out = ckpt - (sum_c s_c * d_c) / float(N), s_c = 1 when ||d_c|| <= C, else (float)(C / ||d_c||):
 * each product rounded to f32, then added, in fold order (the weighted fold with the scales as
 * weights and the divisor N).  ||d_c|| = sqrt(sumsq_c) in f64; sumsq_c is accumulated in f64 in ONE
 * fixed order (tiles of 4,096 params, 256 lane partials, a shuffle tree per
 * wave, the four wave sums left to right, the tile partials left to right), so results are
 * bit-reproducible whatever the launch shape, slot or slab block width.  Non-finite diffs are not
 * sanitised: a NaN norm gives a NaN scale, an infinite norm the scale 0, and the fold follows IEEE.
 *
 * c > 0 (finite) turns clipping on for later ingests and folds of this context, 0 turns it off.
 * With clipping on, every ingest queues the row's norm pass behind its copy, and a fold in
 * PGH_CLIPPED_MEAN computes the sums still missing in one batch, waits for them, and runs the
 * weighted kernels; pgh_set_weights is not used.  PGH_CLIPPED_MEAN with clipping off is
 * PGH_E_STATE.  PGH_E_UNSUPPORTED on a group context, a context whose shard is narrower than the
 * layout (the norm needs the whole row), an int64 slab and a streaming context; pgh_stream_begin
 * refuses PGH_CLIPPED_MEAN the same way. */
int pgh_set_clip_norm(pgh_ctx* ctx, float c);
/* Sums of squares (f64, the order above) of the diffs held by the n listed occupied slots (fp32
 * RESIDENT slab of one GPU): computes the ones not cached since the slot's last ingest.  out
 * non-NULL: waits and returns them (n doubles).  out NULL: only queues the work on the GPU. */
int pgh_row_sumsq(pgh_ctx* ctx, const int32_t* slots, int n, double* out);
/* The scale expression above, on the host (needs no GPU, ctx-free). */
int pgh_clip_scale(double sumsq, float c, float* scale);
/* Over the rows folded in PGH_CLIPPED_MEAN since the last pgh_reset / pgh_reserve (a row counts once
 * per computation of its scale; pgh_fold_slots_restart drops the restarted rows): how many, how many
 * got a scale other than 1, and the largest norm (NaN if any was NaN).  Each pointer may be NULL. */
int pgh_clip_stats(pgh_ctx* ctx, int64_t* n_rows, int64_t* n_clipped, double* max_norm);

/* ---- Gaussian noise on the clipped close (DP-FedAvg; kernel K11) --------------------------------
 * The published recipe: clip every diff to C, add N(0, (z C)^2 I) to the sum, divide by N.  With a noise
 * multiplier z set, a PGH_CLIPPED_MEAN FINAL computes g = acc / float(N) exactly as without it and then,
 * per parameter with flat model index i,
 *   sigma = ((double)z * (double)C) / (double)N    (on the host, f64, N = the fold's divisor count);
 *   n_i = (float)(sigma * Z_i)                     (one f64 product, one rounding to f32);
 *   g'_i = g_i + n_i                               (f32);
 *   out = ckpt - g'; with a server optimizer K10's formulas take g' for g.
 * The result depends on (key, round, z, C, N, diffs) and on nothing else -- not on the launch shape, the
 * range split, the entry point or how often the FINAL runs: a repeated close releases the same noise,
 * never a second draw (two draws would average the noise away).
 *
 * The sampler.  All arithmetic is IEEE, every operation rounded on its own (no FMA); f64 / and sqrt are
 * correctly rounded; no libm call.
 * Generator: Philox4x32-10 (Salmon et al. 2011), multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key
 * increments 0x9E3779B9, 0xBB67AE85.  One round, with (h0, l0) = mulhilo(M0, c0) and (h1, l1) =
 * mulhilo(M1, c2): c = (h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0); ten rounds, the key bumped between rounds.
 * (Counter 0 0 0 0, key 0 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.)
 * Standard normals, two per pair (Marsaglia's polar method).  Parameter i belongs to pair p = i >> 1; an
 * even i takes Z0, an odd i Z1.  The key words are (key & 0xffffffff, key >> 32).  For attempt a = 0 .. 31:
 *   counter (p & 0xffffffff, p >> 32, round, a) -> (x0, x1, x2, x3);
 *   q1 = (int64)((x1 << 32) | x0) >> 11 (arithmetic), v1 = ((double)q1 + 0.5) * 2^-52 (exact, symmetric,
 *   never 0); q2, v2 the same from (x3 << 32) | x2;
 *   s = v1 * v1 + v2 * v2; the first attempt with s < 1.0 is accepted:
 *   L = plog(s), f = sqrt((-2.0 * L) / s), Z0 = v1 * f, Z1 = v2 * f.
 * If all 32 attempts are rejected (probability below 2^-70 per pair; the bound is there so that the
 * kernel's loop provably ends) both normals are +0.0.
 * plog(s), s a normal f64 in (0, 1) (the fdlibm form): b = bits(s), e = ((b >> 52) & 0x7ff) - 1023,
 * mb = b & 0xfffffffffffff; if mb >= 0x6a09e667f3bcd: e += 1, m = bits(mb | 0x3fe0000000000000), else
 * m = bits(mb | 0x3ff0000000000000); f = m - 1.0, t = f / (2.0 + f), w = t * t; R = Lg7, then for c in
 * Lg6 .. Lg1: R = R * w + c, then R = R * w; plog = (double)e * ln2 + (f - t * (f - R)) with
 * ln2 = 0x1.62e42fefa39efp-1, Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
 * Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01,
 * Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01.
 * Philox with a 64-bit key is a statistical generator, not a cryptographic one; a floating-point
 * Gaussian has the known low-bit weakness (Mironov 2012); privacy accounting is the operator's.
 *
 * pgh_set_dp_noise: z = 0 turns the noise off and is always accepted; otherwise z must be finite and > 0
 * (PGH_E_ARG).  PGH_E_UNSUPPORTED with z > 0 wherever pgh_set_clip_norm refuses: a group, a context whose
 * shard is narrower than the layout, an int64 slab, a streaming context.  pgh_set_layout and pgh_set_shard
 * clear the setting; pgh_reset and pgh_reserve keep it.  With noise on, an fp32 FINAL fold in any mode
 * other than PGH_CLIPPED_MEAN is PGH_E_STATE: nothing is launched, the context stays usable, and no
 * un-noised average leaves it.  Folds that are not FINAL, secure aggregation and pgh_stream_begin are not
 * affected.  The fold runs against a plane of -0.0f into a delta plane (the server optimizer's when one is
 * set, else two [P_shard] float planes of the noise's own, allocated by the first noised FINAL), and K11
 * follows on the same stream over the same range, ahead of K10.
 * pgh_dp_normals runs K11's sampler on the GPU and returns Z_i for i in [i0, i0 + n) as f64 (tests,
 * debugging); pgh_dp_normals_host is the same in plain C++, ctx-free, without a GPU.  pgh_dp_stats reports
 * z and what the last noised FINAL used (sigma, N); each pointer may be NULL. */
int pgh_set_dp_noise(pgh_ctx* ctx, float z, uint64_t key, uint32_t round);
int pgh_dp_normals(pgh_ctx* ctx, uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out);
int pgh_dp_normals_host(uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out);
int pgh_dp_stats(pgh_ctx* ctx, float* z, double* sigma_last, int64_t* n_last);

/* ---- coordinate-wise trimmed mean (PGH_TRIMMED_MEAN) ----------------------------------------
 * Per parameter: drop the b largest and the b smallest of the N values, average the other N - 2b.
 * Up to b arbitrary rows (NaN, infinities, 1e30) then cannot move any parameter outside the range
 * of the others' values.  The definition is a streaming one, so the result
 * does not depend on the launch shape, the slots or how the rows are split over launches:
 *   values are ordered by the int32 key(x) = bits(x) ^ ((bits(x) >> 31) & 0x7fffffff) (arithmetic
 *   shift, signed compare: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN; unkey = key);
 *   state per parameter: lo[0..b) = INT32_MAX, hi[0..b) = INT32_MIN, acc (f32);
 *   fold client k = 0, 1, ... (fold order): e = key(x_k);
 *     for j < b: t = max(lo[j], e), lo[j] = min(lo[j], e), e = t;      stop if k < b;
 *     for j < b: t = min(hi[j], e), hi[j] = max(hi[j], e), e = t;      stop if k < 2b;
 *     v = unkey(e);  acc = v when k == 2b, else acc + v (f32);
 *   close: out = ckpt - acc / float(N - 2b), an IEEE f32 division; it needs N >= 2b + 1.
 * The kept multiset is sort(values)[b : N - b] whatever the order; only the f32 additions follow
 * the fold order.
 *
 * pgh_set_trim: b = 0 turns trimming off, 1 .. PGH_TRIM_MAX turns it on, anything else is
 * PGH_E_ARG; changing b while slot folds of a cycle are under way is PGH_E_STATE.  A group hands b
 * to its children.  PGH_TRIMMED_MEAN with trimming off is PGH_E_STATE, and so is a closing fold of
 * fewer than 2b + 1 diffs (nothing is launched; the context stays usable).  Every RESIDENT fold
 * and slot fold accepts the mode, on shards and groups too (nothing in it looks along a row);
 * pgh_stream_begin refuses it (PGH_E_UNSUPPORTED).  A fold that is not a whole cycle in one launch
 * keeps lo, hi and acc in 2b + 1 planes of P_shard words in HBM.  pgh_set_variant does not affect
 * trimmed folds: PGH_TRIM_VEC=4|1 (read by pgh_create) forces 16-byte columns or one parameter
 * per lane, and pgh_effective_variant(ctx, PGH_TRIMMED_MEAN) reports 40 or 41 for them. */
#define PGH_TRIM_MAX 8
int pgh_set_trim(pgh_ctx* ctx, int b);

/* ---- coordinate-wise median (PGH_MEDIAN) -------------------------------------------------------
 * Per parameter, with the trimmed mean's total order on bit patterns (key above; unkey = key; equal
 * keys are identical bits, so ties need no rule) and s = sort(keys of the N reported values):
 *   N odd:  m = unkey(s[(N - 1) / 2]);
 *   N even: a = unkey(s[N / 2 - 1]), b = unkey(s[N / 2]), m = 0.5f * a + 0.5f * b -- two f32
 *           products, each rounded, added once in f32, no FMA (two middles of 3e38 give 3e38; a -inf
 *           and a +inf middle give NaN);
 *   out = ckpt - m, one f32 subtraction.
 * Fewer than ceil(N / 2) rows of arbitrary content cannot move a parameter outside the range of the
 * others' values; a majority of NaNs of one sign leaves a NaN.  The median is pure selection: the
 * result does not depend on the order of the rows, the slots, the launch shape, the slab's block
 * width, the range split or the kernel path.
 * The mode takes every row of the cycle in one call: pgh_fedavg, pgh_fedavg_device[_range],
 * pgh_fedavg_resident and pgh_fold_slots_finish_resident (any n up to the slab's capacity, no
 * earlier slot fold in the cycle: PGH_E_STATE otherwise) accept it, on shards and groups too
 * (nothing in it looks along a row).  pgh_fold_slots and pgh_stream_begin refuse it
 * (PGH_E_UNSUPPORTED): nothing can be folded before every row is there.
 * Two kernel paths with the same results: up to PGH_MEDIAN_NCHIP rows the selection runs on chip in
 * one pass over the slab (K9); more rows, or PGH_MEDIAN_PATH=passes (read by pgh_create), take one
 * pass per key bit with a plane of P_shard words in HBM (K9p).  pgh_effective_variant(ctx,
 * PGH_MEDIAN) reports 50 or 51 for the diffs currently held; pgh_set_variant does not affect
 * median folds. */
#define PGH_MEDIAN_NCHIP 1024

/* ---- geometric-median FedAvg (PGH_GEOMETRIC_MEDIAN, RFA; kernel K12) ----------------------------
 * The geometric median of the diffs -- the point with the smallest sum of L2 distances to them --
 * approximated by a fixed number of smoothed Weiszfeld steps.  It tolerates any hostile minority in norm
 * (not per coordinate), is rotation invariant and returns a point in the convex hull of the diffs.
 * All arithmetic is IEEE, every operation rounded on its own (no FMA contraction); f64 / and sqrt are
 * correctly rounded; no libm call besides sqrt.  Rows d_0 .. d_{N-1} in fold order, iters and nu from
 * pgh_set_geomed:
 *   1. Included rows.  s_c = the sum of squares of row c in the order of "clipped FedAvg" above (K7,
 *      cached at ingest).  A row whose s_c is not finite (a NaN, an infinity, an overflow) is excluded:
 *      no fold and no distance pass reads it (0 * inf cannot poison a parameter).  The included rows
 *      keep their relative order; the k-th of them is fold client k.  No row included: PGH_E_STATE,
 *      nothing is launched, the context stays usable.
 *   2. Iterate.  v^(0) = +0.0.  For t = 0 .. iters - 1, on the host in f64, over the included rows:
 *        D_c = s_c for t = 0, else K12's sum against v^(t) (below);
 *        dist_c = sqrt(D_c);
 *        beta_c = D_c finite ? 1.0 / max((double)nu, dist_c) : 0.0;
 *        B = the left fold of beta_c in fold order (f64); B == 0 is PGH_E_STATE;
 *        w_c = (float)(beta_c / B);  W = the f32 left fold of w_c;
 *        acc = d_0 * w_0; acc = acc + d_c * w_c (the product rounded to f32, then the sum, fold order:
 *        the weighted fold);  v^(t+1) = acc / W (f32).
 *      Iteration 0 needs no distance pass (the norms are there from ingest), and a row of 1e30 cannot
 *      overflow the starting point the way a plain mean would.
 *   3. Close.  out = ckpt - v^(iters); with a server optimizer K10 takes g = v^(iters).
 *   4. K12.  D_c = K7's sum in K7's exact order (tiles of 4,096 params, 256 lane partials over j and e,
 *      the shuffle tree per wave, the four wave sums left to right, the tile partials left to right) over
 *      x_i = d_c[i] - v[i], ONE f32 subtraction, so that the square is exact in f64.  The engine holds -v
 *      (the fold against a -0.0 plane yields it exactly) and adds: d + (-v) is the same IEEE operation.
 * The result is a function of the rows and (iters, nu) alone: not of the launch shape, the slots, the
 * slab's block width, the range split or the entry point; a repeated close gives identical bits.
 *
 * pgh_set_geomed: iters = 0 turns the rule off (always accepted), 1 .. PGH_GEOMED_MAX_ITERS turns it on
 * with nu finite and > 0; anything else is PGH_E_ARG.  PGH_E_UNSUPPORTED wherever pgh_set_clip_norm
 * refuses (a group, a shard narrower than the layout, an int64 slab, a streaming context).
 * pgh_set_layout and pgh_set_shard clear the setting; pgh_reset and pgh_reserve keep it.  With the rule
 * on every ingest queues the row's K7 behind its copy, as clipping does.  The mode takes every row of
 * the cycle in one call: pgh_fedavg, pgh_fedavg_device[_range], pgh_fedavg_resident and
 * pgh_fold_slots_finish_resident (any slot list, no earlier slot fold in the cycle: PGH_E_STATE
 * otherwise) accept it on one GPU holding whole rows; pgh_fold_slots, pgh_stream_begin, groups and
 * narrower shards refuse it (PGH_E_UNSUPPORTED); the mode without the setting is PGH_E_STATE, and so
 * is the mode beside DP noise.  pgh_set_weights is not used (the close replaces the weights).  The
 * inner iterations run whole-shard on the context's stream and are finished when the call that
 * computed them returns; the final weights are computed once per state of the slab (range calls and
 * repeated closes reuse them), and only the last fold is a FINAL one.  Two [P_shard] float planes in
 * HBM (-0.0 and -v), allocated by the first close with iters >= 2.  pgh_effective_variant(ctx,
 * PGH_GEOMETRIC_MEDIAN) reports what the weighted fold would run.
 * pgh_row_distsq: K12 alone against `point` (host, P floats), the counterpart of pgh_row_sumsq: the n
 * listed occupied slots' D_c into out (n doubles).
 * pgh_geomed_stats: the setting's iters and, of the last computation of the weights: the rows given, how
 * many were excluded, the f64 left fold of dist_c over the included rows in the last iteration
 * (the objective) and the largest w_c of it.  Each pointer may be NULL. */
#define PGH_GEOMED_MAX_ITERS 16
int pgh_set_geomed(pgh_ctx* ctx, int iters, float nu);
int pgh_row_distsq(pgh_ctx* ctx, const int32_t* slots, int n, const float* point, double* out);
int pgh_geomed_stats(pgh_ctx* ctx, int* iters, int64_t* n_rows, int64_t* n_excluded, double* objective,
                     float* max_weight);

/* ---- trust-bootstrapped FedAvg (PGH_TRUSTED_MEAN, FLTrust; kernel K14) ---------------------------
 * Every other robust rule here assumes that the hostile workers are a minority.  This one does not: the
 * server computes an update g0 of its own from a small clean root dataset and the cycle's checkpoint, and
 * every reported diff is scored against it.  A diff pointing away from g0 gets trust 0; every other diff is
 * rescaled to g0's norm and weighted by its cosine to g0.  The result stays inside the ball of radius |g0|
 * whatever the number of hostile workers.  All arithmetic is IEEE, every operation rounded on its own (no
 * FMA contraction); / and sqrt are correctly rounded; no libm call besides sqrt.  Rows d_0 .. d_{n-1} in
 * fold order and the root g0 of P float32 (pgh_trust_root):
 *   1. Root.  s0 = the sum of squares of g0 in the order of "clipped FedAvg" above (K7's exact order: the
 *      same bits as pgh_row_sumsq of a slot holding g0).  s0 must be finite and > 0: a NaN, an infinity or an
 *      all-zero root is PGH_E_ARG and no root is set.
 *   2. Included rows.  s_c = K7's sum of row c, cached at ingest.  A row whose s_c is not finite is excluded,
 *      as in the geometric median: no fold and no K14 pass of the close reads it.  The k-th included row is
 *      fold client k.  No row included: PGH_E_STATE, nothing is launched, the context stays usable.
 *   3. K14.  p_c = K7's sum in K7's exact order over (double)d_c[i] * (double)g0[i]: tiles of 4,096 params,
 *      256 lane partials over j and e starting at +0.0, the shuffle tree per wave, ((w0 + w1) + w2) + w3, the
 *      tile partials left to right.  The product of two f32 values is exact in f64, so fma(x, y, acc) is the
 *      rounded add of the definition.  Params at or past P contribute +0.0 (the product is masked, not one
 *      factor: 0 x NaN is NaN).  p_c is finite for every included row.
 *   4. Weights, on the host in f64 unless said otherwise.  n0 = sqrt(s0), n_c = sqrt(s_c).
 *        s_c > 0:  cos_c = p_c / (n0 * n_c);  ts_c = cos_c > 0 ? cos_c : 0.0;  a_c = ts_c * (n0 / n_c);
 *        s_c == 0: ts_c = a_c = 0.0;
 *        T = the left fold of ts_c in fold order; T == 0 is PGH_E_STATE (no row is trusted), nothing is folded;
 *        w_c = (float)min(a_c / T, (double)FLT_MAX)  (the clamp keeps a hostile row of subnormal norm from
 *        turning its rescale into +inf).
 *   5. Fold and close.  acc = d_0 * w_0; acc = acc + d_c * w_c (the product rounded to f32, then the sum: the
 *      weighted fold, with the divisor 1.0f); out = ckpt - acc; with a server optimizer K10 takes g = acc.
 *      Rows of weight zero stay in the fold.
 * The result is a function of the rows, their order and the root alone: not of the slots, the launch shape,
 * the slab's block width, the range split or the entry point, nor of whether the dots were computed at
 * ingest or at the close; a repeated close gives identical bits.
 *
 * pgh_set_trust: on != 0 switches the rule on, 0 off (always accepted).  PGH_E_UNSUPPORTED wherever
 * pgh_set_clip_norm refuses (a group, a shard narrower than the layout, an int64 slab, a streaming
 * context).  pgh_set_layout and pgh_set_shard clear the setting; pgh_reset and pgh_reserve keep it.  With the
 * rule on every ingest queues the row's K7 behind its copy, as clipping does.
 * pgh_trust_root: the cycle's root, P floats (nbytes = 4 P, else PGH_E_ARG), uploaded to a [P_shard] plane of
 * its own; it needs the rule on (PGH_E_STATE).  The root belongs to the cycle: pgh_reset and pgh_reserve
 * drop its validity (the plane stays), and a close without a root set since then is PGH_E_STATE.  A call
 * that fails leaves no root set.  A new root makes the cached dots and the weights stale.  While a root is
 * valid every ingest also queues the row's K14 behind its K7, so a report-time close is the host step plus
 * one weighted fold; a close computes the dots still missing in one batch.
 * The mode takes every row of the cycle in one call: pgh_fedavg, pgh_fedavg_device[_range],
 * pgh_fedavg_resident and pgh_fold_slots_finish_resident (any slot list, no earlier slot fold in the cycle:
 * PGH_E_STATE otherwise) accept it on one GPU holding whole rows; pgh_fold_slots, pgh_stream_begin, groups
 * and narrower shards refuse it (PGH_E_UNSUPPORTED); the mode with the rule off or without a valid root is
 * PGH_E_STATE, and so is the mode beside DP noise.  pgh_set_weights is not used (the close replaces the
 * weights).  The weights are computed once per state of the slab and root: range calls and repeated closes
 * reuse them.  pgh_effective_variant(ctx, PGH_TRUSTED_MEAN) reports what the weighted fold would run.
 * pgh_row_dot: K14 alone against `point` (host, P floats), the counterpart of pgh_row_distsq: the n listed
 * occupied slots' p_c into out (n doubles).  It does not sanitise, a slot may repeat, and it uses a scratch
 * plane of its own: the root, the cached dots and K7's cache are untouched.
 * pgh_trust_weights_host: steps 2 and 4 in plain C++, no context and no GPU: from s0 and the n rows' s_c and
 * p_c (p_c is not read where s_c is not finite), the positions of the included rows into `included` and
 * their w_c into `weights` (room for n each), their count and T.  s0 not finite or <= 0 is PGH_E_ARG; no row
 * included or T == 0 is PGH_E_STATE (n_included and total_trust are written all the same).
 * pgh_trust_stats: whether the rule is on and, of the last computation of the weights: the rows given, how
 * many were excluded, how many had ts > 0, T, the largest w_c, and n0 of the valid root (0 without one).
 * Each pointer may be NULL. */
int pgh_set_trust(pgh_ctx* ctx, int on);
int pgh_trust_root(pgh_ctx* ctx, const float* root, size_t nbytes);
int pgh_row_dot(pgh_ctx* ctx, const int32_t* slots, int n, const float* point, double* out);
int pgh_trust_weights_host(double s0, const double* sumsq, const double* dot, int n, float* weights,
                           int32_t* included, int* n_included, double* total_trust);
int pgh_trust_stats(pgh_ctx* ctx, int* on, int64_t* n_rows, int64_t* n_excluded, int64_t* n_trusted,
                    double* total_trust, float* max_weight, double* root_norm);

/* ---- Multi-Krum selection of diffs ahead of the average (Blanchard et al. 2017; kernel K13) --------
 * A stage, not an averaging mode: it decides WHICH diffs a cycle averages.  Each diff is scored by its
 * distance to its nearest neighbours, the m most central diffs are kept and the others leave the cycle;
 * the cycle's mode (any of pgh_mode, with or without a server optimizer) then runs over the picked slots
 * through pgh_fold_slots_finish_resident exactly as if they were the only reports.  The selection is a
 * call, not a context setting.  All arithmetic is IEEE, every operation rounded on its own, no libm call.
 * Rows d_0 .. d_{n-1} in the caller's list order (distinct occupied slots), an assumed hostile count
 * f >= 0 and a keep count m:
 *   1. Included rows.  s_c = the sum of squares of row c (K7, cached at ingest or computed now, as
 *      pgh_row_sumsq does).  A row whose s_c is not finite -- exactly the rows holding a NaN or an
 *      infinity -- is excluded: no distance pass reads it.  The n' included rows keep their relative
 *      order.  f is not reduced by the excluded rows (the conservative reading).  n' >= 2f + 3, else
 *      PGH_E_STATE: nothing is launched after the sums and the context stays usable.
 *   2. Distances.  For included a != b, D[a][b] = K7's sum in K7's exact order (tiles of 4,096 params,
 *      256 lane partials over j and e, the shuffle tree per wave, ((w0 + w1) + w2) + w3, the tile partials
 *      left to right, params at or past P as +0.0) over x_i = d_a[i] - d_b[i], ONE f32 subtraction, so
 *      that the square is exact in f64.  d_a - d_b = -(d_b - d_a) exactly, so D is symmetric by
 *      construction: the kernel computes one triangle.  D[a][a] = +0.0.  Between included rows D is never
 *      NaN; it may be +inf (the f32 difference of 3e38 and -3e38 overflows), which orders like any other
 *      value.  D[a][b] is the same f64 bits as pgh_row_distsq of row a against the point d_b.
 *   3. Scores.  k = n' - f - 2; score_a = the f64 left fold, in ascending order of value, of the k
 *      smallest of the n' - 1 values D[a][b], b != a.
 *   4. Selection.  The included rows ordered by (score, list position) ascending -- equal scores break
 *      towards the earlier row, +inf included -- and the first m taken.  m = 0 means n' - f (Multi-Krum);
 *      m = 1 is Krum; m > n' - f is PGH_E_STATE.  The picked rows are reported in list order, so the fold
 *      order of the close is the cycle's order with the others left out.
 * The result is a function of the rows, their order, f and m alone: not of the slots, the slab's block
 * width or the batching of the distance passes.
 *
 * pgh_row_pairdist: the raw n x n matrix (row-major) over the listed occupied slots: K13 alone.  Like
 * pgh_row_distsq it does not sanitise and a slot may repeat.
 * pgh_krum_select_host: steps 3 and 4 over the n x n matrix of the included rows, no context and no GPU:
 * positions into picked (room for n), their count, and the n scores when `scores` is not NULL.  A NaN or
 * negative off-diagonal entry, f < 0 or m < 0 is PGH_E_ARG; n < 2f + 3 or m > n - f is PGH_E_STATE.
 * pgh_krum_select: steps 1 to 4 over the listed slots; the picked SLOTS in list order into picked (room
 * for n).  A duplicate or unoccupied slot, f < 0 or m < 0 is PGH_E_ARG.
 * Both context calls: n > PGH_KRUM_MAX_ROWS is PGH_E_UNSUPPORTED, and so is every context pgh_row_sumsq
 * refuses (a group, a shard narrower than the layout, an int64 slab, a streaming context).  The tile
 * partials of the distance passes take at most 1 GiB of HBM whatever n and the model: the anchors go in
 * batches (PGH_PAIRDIST_BUDGET, bytes, read at pgh_create, lowers the budget).
 * pgh_krum_stats: of the last pgh_krum_select that selected: the rows given, how many were excluded, how
 * many were picked, the largest score among the picked and the smallest among the dropped (+inf when
 * none was dropped).  Each pointer may be NULL. */
#define PGH_KRUM_MAX_ROWS 1024
int pgh_row_pairdist(pgh_ctx* ctx, const int32_t* slots, int n, double* out);
int pgh_krum_select_host(const double* dist, int n, int f, int m, int32_t* picked, int* n_picked,
                         double* scores);
int pgh_krum_select(pgh_ctx* ctx, const int32_t* slots, int n, int f, int m, int32_t* picked,
                    int* n_picked);
int pgh_krum_stats(pgh_ctx* ctx, int64_t* n_rows, int64_t* n_excluded, int64_t* n_picked,
                   double* max_picked_score, double* min_dropped_score);

/* ---- server optimizers: how the average is applied (FedAvgM, FedAdagrad, FedAdam, FedYogi) ------
 * Without one, a close writes out = ckpt - g, g being the cycle's average as its mode defines it
 * (acc / divisor; the iterative mean's acc; the trimmed mean; the median).  With one set, every
 * fp32 FINAL fold (pgh_fedavg, pgh_fedavg_device[_range], pgh_fedavg_resident,
 * pgh_fold_slots_finish_resident, pgh_stream_finish*; every mode; shards and groups) applies, per
 * parameter and in f32, each operation rounded on its own (no FMA; sqrt and / correctly rounded):
 *   c1 = 1.0f - beta1, c2 = 1.0f - beta2, v0 = tau * tau (computed once, in f32);
 *   state: m starts at +0.0f, v at v0;
 *   PGH_OPT_MOMENTUM (Hsu et al. 2019):  m' = beta1 * m + g;  out = ckpt - lr * m'            (no v)
 *   PGH_OPT_ADAGRAD (Reddi et al. 2021): m' = beta1 * m + c1 * g;  q = g * g;  v' = v + q;
 *                                        out = ckpt - (lr * m') / (sqrt(v') + tau)
 *   PGH_OPT_ADAM:   as Adagrad with v' = beta2 * v + c2 * q
 *   PGH_OPT_YOGI:   as Adagrad with s = v > q ? 1.0f : v < q ? -1.0f : 0.0f (a NaN gives 0) and
 *                   v' = v - (c2 * q) * s
 * There is no bias correction.  Non-finite values follow IEEE and are not sanitised: a NaN in g stays
 * in that parameter's m / v until the state is uploaded again (PGH_TRIMMED_MEAN and PGH_MEDIAN keep
 * a minority's NaN out of g).  The fold kernels run unchanged, against a plane of -0.0f into a delta
 * plane d = (-0.0f) - g = -g (exact for every non-NaN g, signed zeros included), and kernel K10
 * follows on the same stream over the same parameter range.  Secure aggregation is not affected.
 *
 * pgh_set_server_opt: PGH_E_ARG unless lr is finite and > 0, beta1 in [0, 1), and -- for the kinds that
 * use them, ignored otherwise -- beta2 in [0, 1) and tau finite and > 0.  The same kind and values again
 * keep the state; any change initialises it again; PGH_OPT_NONE frees the planes and restores the plain
 * path.  It needs a layout (PGH_E_STATE).  The planes are six [P_shard] float vectors in HBM (four for
 * PGH_OPT_MOMENTUM): -0, d, and m and v twice.  The state belongs to the model: it survives pgh_reset
 * and pgh_reserve; pgh_set_layout and pgh_set_shard drop it and the setting, and so does a group's
 * pgh_reserve of a client-sharded int64 slab (pgh_set_client_sharding), which shards its children anew.
 * A FINAL never updates the state in place: it reads the committed m / v and writes pending ones, so a
 * repeated FINAL gives identical bits.  pgh_server_opt_commit makes the pending state the committed one
 * (a pointer swap) and counts a step; PGH_E_STATE when no FINAL has run since the last commit or
 * upload.  Where the FINAL launches since the last commit covered only part of the shard
 * (pgh_fedavg_device_range), the commit leaves the moments of every other parameter as they were.
 * The library never commits by itself.  pgh_server_opt_download copies the committed state
 * out (P_shard floats each; v may be NULL for PGH_OPT_MOMENTUM); pgh_server_opt_upload replaces it
 * (each array the whole model or this shard, like pgh_ckpt_upload) and clears anything pending.  A
 * group hands the setting and the commit to its children and scatters / gathers the state by slice. */
typedef enum {
    PGH_OPT_NONE = 0,
    PGH_OPT_MOMENTUM = 1,
    PGH_OPT_ADAGRAD = 2,
    PGH_OPT_ADAM = 3,
    PGH_OPT_YOGI = 4
} pgh_server_opt;
int pgh_set_server_opt(pgh_ctx* ctx, int kind, float lr, float beta1, float beta2, float tau);
int pgh_server_opt_commit(pgh_ctx* ctx);
int pgh_server_opt_steps(pgh_ctx* ctx, int64_t* committed);
int pgh_server_opt_download(pgh_ctx* ctx, float* m, float* v);
int pgh_server_opt_upload(pgh_ctx* ctx, const float* m, const float* v, size_t nbytes);

/* ---- reduction ----------------------------------------------------------------------------
 * out = ckpt - avg(diffs), over this context's shard.  Host pointers, P_shard floats each. */
int pgh_fedavg(pgh_ctx* ctx, int mode, const float* ckpt, float* out);
/* Same with device pointers (16-byte aligned, P_shard floats) on caller stream `stream`
 * (a hipStream_t; NULL = the HIP default stream, ordered with other blocking streams).  Nothing
 * is copied to the host. */
int pgh_fedavg_device(pgh_ctx* ctx, int mode, const float* d_ckpt, float* d_out, void* stream);
/* Only the shard-relative param range [off, off + len) (off a multiple of 4): lets a caller
 * overlap the collective that ships finished ranges with the fold of the next one.  d_ckpt and
 * d_out are the shard base pointers. */
int pgh_fedavg_device_range(pgh_ctx* ctx, int mode, int64_t off, int64_t len, const float* d_ckpt, float* d_out,
                            void* stream);
/* ---- resident checkpoint: keep the model in HBM across cycles ---------
 * Upload the current checkpoint once (flat floats: the whole model or this shard; or straight
 * from its State bytes), fold with pgh_fedavg_resident -- the result replaces the resident
 * checkpoint, so the next cycle needs no checkpoint upload -- and read it back as floats or as
 * State bytes (the template's payload spans overwritten, like pgh_state_patch). */
int pgh_ckpt_upload(pgh_ctx* ctx, const float* ckpt, size_t nbytes);
int pgh_ckpt_upload_state(pgh_ctx* ctx, const uint8_t* pb, size_t n);
int pgh_fedavg_resident(pgh_ctx* ctx, int mode);
int pgh_ckpt_download(pgh_ctx* ctx, float* out);  /* P_shard floats */
/* out (n bytes) = tmpl with this shard's slice of every payload taken from the resident checkpoint. */
int pgh_ckpt_patch_state(pgh_ctx* ctx, const uint8_t* tmpl, size_t n, uint8_t* out);

/* ---- report-time folds of scattered slots -----------------------------
 * RESIDENT slab.  Diffs are ingested into whichever slot is free when they are reported (client
 * index = slot); the fold order is the reference's close-time order -- completed WorkerCycles in
 * assignment (row id) order, cycle_manager.py:243-245 -- which the caller gives as slot lists:
 * pgh_fold_slots folds `slots` (n entries, in list order) into the running fold state as soon as
 * their positions are certain, and frees them for new ingests; the k-th slot folded since
 * pgh_reset / pgh_reserve is fold client k (the iterative plan's k, weight index k; weights are set
 * in fold order with pgh_set_weights).  pgh_fold_slots_finish_resident folds the rest (n may be 0)
 * and writes ckpt - avg into the resident checkpoint (pgh_ckpt_upload*), like
 * pgh_fedavg_resident: bit-identical to folding every diff contiguously at close.  `mode` stays the
 * same within a cycle. */
int pgh_fold_slots(pgh_ctx* ctx, int mode, const int32_t* slots, int n);
int pgh_fold_slots_finish_resident(pgh_ctx* ctx, int mode, const int32_t* slots, int n);
/* Discard the running fold state of this cycle's slot folds (the diffs folded so far are gone
 * from it; the next pgh_fold_slots starts again at fold client 0, and weights must be set again).
 * Slots holding unfolded diffs keep them.  Used when the close-time order of the
 * completed WorkerCycles (cycle_manager.py:243-245) differs from the order the early folds
 * assumed, or a folded worker re-reported (submit_worker_diff overwrites its diff, :162-174):
 * the caller then re-folds every diff in the query's order, bit-identical to the reference. */
int pgh_fold_slots_restart(pgh_ctx* ctx);
/* Report-time ingest (on != 0; default off): every State diff of a shard of >= 1M params is
 * copied to HBM in param ranges with an event each, and the close's fold
 * (pgh_fold_slots_finish_resident) starts each range as soon as the LAST report's copy of that
 * range has landed instead of waiting for the whole copy -- the close overlaps the tail of the
 * last report's DMA.  Costs a few % of H2D throughput per diff (more, smaller copies), so it is
 * for report-time aggregation, not for a close that ingests every diff at once. */
int pgh_set_ingest_ranges(pgh_ctx* ctx, int on);

/* Z_2^64 share sum over all clients x parties, then decode float32(sum) / base**prec.
 * sum_out (int64) and dec_out (float32) are host arrays of P_shard; either may be NULL. */
int pgh_secagg(pgh_ctx* ctx, int base, int prec, int64_t* sum_out, float* dec_out);
int pgh_secagg_device(pgh_ctx* ctx, int base, int prec, int64_t* d_sum, float* d_dec, void* stream);
/* Only the shard-relative param range [off, off + len) (off % 4 == 0); d_sum / d_dec are the
 * shard-sized outputs, of which only that range is written (multi-GPU gather overlap). */
int pgh_secagg_device_range(pgh_ctx* ctx, int base, int prec, int64_t off, int64_t len, int64_t* d_sum,
                            float* d_dec, void* stream);
/* Decode only: d_dec[i] = float32(int64 d_sum[i]) / base**prec for i < n, on `stream` (device
 * pointers; needs no slab).  Client-sharded secure aggregation: every rank sums the shares of its
 * own clients (pgh_secagg_device with d_dec = NULL), the [P] sums are reduce-scattered with an
 * int64 SUM (wrap-add is associative: exact), and each rank decodes its param shard here -- the
 * same expression as pgh_secagg's decode.  Replaces the decode half of PySyft 0.2.9's
 * FixedPrecisionTensor.float_precision (test_basic_syft_operations.py:417-424). */
int pgh_secagg_decode_device(pgh_ctx* ctx, int base, int prec, const int64_t* d_sum, int64_t n, float* d_dec,
                             void* stream);
/* Fill a device buffer with the synthetic checkpoint of this shard (P_shard floats). */
int pgh_synth_ckpt_device(pgh_ctx* ctx, uint64_t seed, float* d_ckpt, void* stream);

/* ---- STREAM use: fold clients in order as they arrive ---------------------------------------
 * After pgh_stream_begin, every run of >= fold_batch consecutive clients at the fold front is
 * folded into the running state (same op order as RESIDENT: bit-identical results) and its slots
 * are freed; H2D of later clients overlaps those folds.  kind = a pgh_mode or PGH_STREAM_SECAGG;
 * fold_batch <= 0 means half the slots.  Clients may arrive out of order within the ring.
 * PGH_CLIPPED_MEAN, PGH_TRIMMED_MEAN and PGH_MEDIAN are refused (PGH_E_UNSUPPORTED). */
int pgh_stream_begin(pgh_ctx* ctx, int kind, int fold_batch);
int pgh_stream_flush(pgh_ctx* ctx);               /* fold the ready run now */
/* Fold what is left and write out = ckpt - avg (all clients [0, n) must have arrived). */
int pgh_stream_finish(pgh_ctx* ctx, const float* ckpt, float* out);
int pgh_stream_finish_device(pgh_ctx* ctx, const float* d_ckpt, float* d_out, void* stream);
/* Finish into the resident checkpoint (pgh_ckpt_upload / pgh_ckpt_upload_state, possibly uploaded
 * while clients were still arriving): afterwards it IS the new checkpoint, ready for
 * pgh_ckpt_patch_state / pgh_ckpt_download and the next cycle. */
int pgh_stream_finish_resident(pgh_ctx* ctx);
int pgh_stream_finish_secagg(pgh_ctx* ctx, int base, int prec, int64_t* sum_out, float* dec_out);
int pgh_stream_finish_secagg_device(pgh_ctx* ctx, int base, int prec, int64_t* d_sum, float* d_dec, void* stream);

/* ---- tuning and observability -------------------------------------------------------------- */
/* Kernel variant for A/B measurement (table in csrc/pgh_variants.def); -1 = the default, which
 * picks by shard size (auto_variant in csrc/pgh_kernels.hip). */
#define PGH_DEFAULT_VARIANT (-1)
int pgh_set_variant(pgh_ctx* ctx, int variant);
/* The variant the next fold of this context's shard runs for `mode` (a pgh_mode, or
 * PGH_STREAM_SECAGG for the share sum): >= 0, or an error status. */
int pgh_effective_variant(pgh_ctx* ctx, int mode);
int pgh_stats(pgh_ctx* ctx, pgh_stats_t* out);     /* synchronises pending timing events */
int pgh_reset_stats(pgh_ctx* ctx);
/* Device pointer and geometry of the slab, for callers that drive the kernels.  The slab is
 * column-blocked: element (row r, shard param i) is at
 *   d_slab[(i / ld) * block_pitch + r * ld + i % ld]
 * (row r = slot * n_parties + party).  A shard of at most one block has block_pitch 0 and is
 * plain row-major [rows][ld]. */
int pgh_slab(pgh_ctx* ctx, void** d_slab, int64_t* ld, int64_t* block_pitch);
int pgh_sync(pgh_ctx* ctx);                       /* wait for the context's streams */

/* ---- State codec (host only; replaces syft serde at model_manager.py:79-103) ------------- */
/* Locate each tensor's packed float32 payload in a State message: byte offset and element
 * count, State order.  Up to `cap` entries are written; *n_tensors = tensors found. */
int pgh_state_scan(const uint8_t* pb, size_t n, int cap, int64_t* offsets, int64_t* counts, int* n_tensors);
/* New checkpoint (serialize_model_params, model_manager.py:79-92, as used at
 * cycle_manager.py:303): `tmpl` with every payload overwritten by `values` (P floats).  `out`
 * has n bytes; out == tmpl patches in place. */
int pgh_state_patch(const uint8_t* tmpl, size_t n, const float* values, int64_t n_values, uint8_t* out);

/* Framing of the new checkpoint as serialize_model_params emits it (model_manager.py:79-92:
 * State(state_placeholders=[PlaceHolder().instantiate(p) for p in params]) of plain tensors): per
 * tensor of `tmpl` (State order, its shapes) a Placeholder{id = ids[2k]} and a
 * StateTensor.torch_tensor{id = ids[2k + 1], serializer, contents_data{shape, "float32", payload}};
 * no tags.  *needed = message bytes; with out (cap >= *needed) the framing is written and every
 * payload span left for pgh_ckpt_patch_state(ctx, out, n, out) (in place) or the caller.  n_ids must
 * be 2 x the tensors of tmpl. */
int pgh_state_fresh(const uint8_t* tmpl, size_t n, const int64_t* ids, int n_ids, uint8_t* out, size_t cap,
                    size_t* needed);

/* Secure-aggregation shares as State bytes: every tensor a TensorData.contents_int64 (packed
 * varint; build-owned schema restatement, field 10).  Per tensor: payload byte offset, payload
 * bytes and the number of int64 values, validated as protobuf's parser would (varints of at most
 * 10 bytes, none cut off, count == shape numel when a shape is present).  PGH_E_PARSE otherwise. */
int pgh_state_scan_i64(const uint8_t* pb, size_t n, int cap, int64_t* offsets, int64_t* nbytes, int64_t* counts,
                       int* n_tensors);

/* ---- report path (host only): base64 of the diff (fl_events.py:257) ----------------------- */
size_t pgh_b64_decoded_cap(size_t n);
/* Python base64.b64decode semantics (non-validating); threads <= 0 = auto.  PGH_E_PARSE on bad
 * padding. */
int pgh_b64_decode(const char* in, size_t n, uint8_t* out, size_t* written, int threads);
/* Decoded size, computed from the text after the last whole quad of the '='-free prefix alone,
 * valid IF that prefix is all alphabet characters (the common case; not checked).  PGH_E_PARSE when
 * that tail is not clean: use pgh_b64_decode(out = NULL) for the exact size then. */
int pgh_b64_clean_size(const char* in, size_t n, size_t* size);
/* One pass for a clean string (every character before the first '=' in the alphabet): `out` holds
 * `cap` = pgh_b64_clean_size bytes.  PGH_E_STATE when the text is not clean (or decodes to more than
 * cap): take pgh_b64_decode then. */
int pgh_b64_decode_clean(const char* in, size_t n, uint8_t* out, size_t cap, size_t* written, int threads);

#ifdef __cplusplus
}
#endif
#endif /* PGH_API_H */
