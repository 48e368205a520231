// HIP-free host code of libpygrid_hip (not installed): the non-temporal copy, the copy pool, the
// scatter out of a landed piece, the walk over concatenated host pieces, the chunk arithmetic of ranged ingest,
// page pre-faulting, the CPU count, the DP noise sampler's restatement, the host steps of the geometric median,
// the Multi-Krum selection and the trust rule, the per-slot state machine of a cached row reduction (SlotCache).
// Nothing here may include HIP.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace pgh_int { int usable_cpus(); }  // (documented in pgh_internal.h)

namespace pgh_detail {

// memcpy with non-temporal 16-byte stores for big copies into staging / output buffers (no
// read-for-ownership of the destination, which is written once and then read by the DMA engine or
// handed to the caller; r01ab).
void copy_stream(uint8_t* dst, const uint8_t* src, size_t n);
// Bind the calling thread to `cpus` (no-op when empty or refused).
void bind_thread(const std::vector<int>& cpus);

// Host copy engine: a persistent pool that splits one batch of (dst, src, n) segments evenly
// by bytes across its threads (the caller's thread takes the first share).  Used to fill and
// drain the pinned staging slots, where payload pieces are many and mostly small.
class CopyPool {
  public:
    struct Seg {
        uint8_t* dst;
        const uint8_t* src;
        size_t n;
    };
    explicit CopyPool(int threads, std::vector<int> cpus = {}) : nthreads_(std::max(1, threads)) {
        for (int t = 1; t < nthreads_; ++t)
            workers_.emplace_back([this, t, cpus] {
                bind_thread(cpus);
                loop(t);
            });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
            ++gen_;
        }
        cv_.notify_all();
        for (auto& w : workers_) w.join();
    }
    int threads() const { return nthreads_; }
    void run(const std::vector<Seg>& segs) {
        size_t total = 0;
        for (auto& sg : segs) total += sg.n;
        if (total < (4u << 20) || nthreads_ == 1) { copy_range(segs, 0, total); return; }
        {
            std::lock_guard<std::mutex> lk(m_);
            segs_ = &segs;
            total_ = total;
            pending_ = nthreads_ - 1;
            ++gen_;
        }
        cv_.notify_all();
        copy_range(segs, 0, share(total, 0));
        std::unique_lock<std::mutex> lk(m_);
        done_cv_.wait(lk, [this] { return pending_ == 0; });
        segs_ = nullptr;
    }

    // f(i) for every i in [0, n), items split into contiguous runs over the threads (the caller's
    // thread takes the first run).  Small jobs stay on the caller's thread.
    void run_items(int n, bool parallel, const std::function<void(int)>& f) {
        if (!parallel || nthreads_ == 1 || n < 2) { for (int i = 0; i < n; ++i) f(i); return; }
        const int per = (n + nthreads_ - 1) / nthreads_;
        std::function<void(int)> job = [&](int t) {
            for (int i = t * per; i < std::min(n, (t + 1) * per); ++i) f(i);
        };
        {
            std::lock_guard<std::mutex> lk(m_);
            fn_ = &job;
            pending_ = nthreads_ - 1;
            ++gen_;
        }
        cv_.notify_all();
        job(0);
        std::unique_lock<std::mutex> lk(m_);
        done_cv_.wait(lk, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }

  private:
    size_t share(size_t total, int t) const {  // [begin, end) of thread t, 4 KiB granules
        const size_t per = ((total + nthreads_ - 1) / nthreads_ + 4095) & ~(size_t)4095;
        return std::min(total, per * (size_t)(t + 1));
    }
    static void copy_range(const std::vector<Seg>& segs, size_t a, size_t b) {
        size_t base = 0;
        for (auto& sg : segs) {
            const size_t lo = std::max(a, base), hi = std::min(b, base + sg.n);
            if (lo < hi) copy_stream(sg.dst + (lo - base), sg.src + (lo - base), hi - lo);
            base += sg.n;
            if (base >= b) break;
        }
    }
    void loop(int t) {
        uint64_t seen = 0;
        for (;;) {
            const std::vector<Seg>* segs;
            const std::function<void(int)>* fn;
            size_t total;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                segs = segs_;
                fn = fn_;
                total = total_;
            }
            if (fn) {
                (*fn)(t);
            } else {
                const size_t a = t == 0 ? 0 : share(total, t - 1);
                copy_range(*segs, std::min(a, total), share(total, t));
            }
            std::lock_guard<std::mutex> lk(m_);
            if (--pending_ == 0) done_cv_.notify_one();
        }
    }
    int nthreads_;
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    const std::vector<Seg>* segs_ = nullptr;
    const std::function<void(int)>* fn_ = nullptr;
    size_t total_ = 0;
    int pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

struct Piece {
    const uint8_t* src;
    size_t n;
};
struct OutPiece {
    uint8_t* dst;
    size_t n;
};
// The walk over concatenated host pieces: take appends to `segs` the copies that fill `room` bytes at
// dst, or what is left of the pieces, and returns the bytes taken.  A zero-length piece yields an empty
// segment when the walk reaches it before the room is full; a piece that ends exactly at the edge is
// finished by the take that reaches the edge.
struct PieceCursor {
    const std::vector<Piece>& pieces;
    size_t pi = 0, poff = 0;
    size_t take(uint8_t* dst, size_t room, std::vector<CopyPool::Seg>* segs) {
        size_t fill = 0;
        while (fill < room && pi < pieces.size()) {
            const size_t m = std::min(pieces[pi].n - poff, room - fill);
            segs->push_back({dst + fill, pieces[pi].src + poff, m});
            fill += m;
            poff += m;
            if (poff == pieces[pi].n) { ++pi; poff = 0; }
        }
        return fill;
    }
};
void scatter_out(const uint8_t* src, size_t off, size_t len, const std::vector<OutPiece>& pieces, CopyPool& pool);

// HBM -> host results move in pieces of at most D2H_PIECE, the later pieces' DMAs beside the host
// copy-out of the earlier ones (r01ac: 4, 8, 16 MiB within the noise of the 47 MB report-time close;
// with the parallel pre-fault, r01ak, 8 MiB pieces closed in 2.3-2.4 ms vs 2.6-2.7 for one piece).
constexpr size_t D2H_PIECE = 8u << 20;
// Ranged report ingest (pgh_set_ingest_ranges): one chunk = the params of one D2H piece = two
// 4 MiB FINAL ranges of a report-time close (pgh_slots.cpp).
constexpr int64_t INGEST_CHUNK = (int64_t)(D2H_PIECE / 4);
inline int ingest_chunks(int64_t pg) { return (int)((pg + INGEST_CHUNK - 1) / INGEST_CHUNK); }  // of a row of pg floats
// the bytes [*a, *b) of chunk k of a row of pg floats
inline void ingest_chunk_bytes(int64_t pg, int k, size_t* a, size_t* b) {
    *a = (size_t)k * INGEST_CHUNK * 4;
    *b = std::min((size_t)pg * 4, (size_t)(k + 1) * INGEST_CHUNK * 4);
}
// params from `at` up to the next chunk boundary: a gather chunk of a ranged ingest is cut there
inline int64_t ingest_chunk_room(int64_t at) { return (at / INGEST_CHUNK + 1) * INGEST_CHUNK - at; }

void prefault_small_any(uint8_t* p, size_t n);
void prefault_parallel(uint8_t* p, size_t n, CopyPool& pool);

// The DP noise sampler of include/pgh_api.h ("Gaussian noise on the clipped close") in plain C++, operation
// by operation: what kernel K11 computes on the GPU (pgh_dp_normals_host; built with -ffp-contract=off).
void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
double dp_plog(double s);  // a normal s in (0, 1)
void dp_pair_normals(uint64_t key, uint32_t round, uint64_t pair, double* z0, double* z1);
// Z_i for the flat model indices [i0, i0 + n) (i0 >= 0): pair i >> 1, even i takes Z0, odd i Z1
void dp_normals(uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out);
// ((double)z * (double)C) / (double)N
inline double dp_sigma(float z, float c, int64_t n) { return ((double)z * (double)c) / (double)n; }

// One host step of the geometric median (include/pgh_api.h, "Geometric-median FedAvg"): from the squared
// distances D[0, n) of the included rows, in fold order, the weights w[0, n), their f32 left fold *W, the
// f64 left fold of sqrt(D) (*objective) and the largest weight (*max_w; both nullable).  False when the
// f64 left fold of the betas is 0 (every D non-finite): w and *W are not written then.
bool geomed_step(const double* D, int64_t n, float nu, float* w, float* W, double* objective, float* max_w);

// Steps 3 and 4 of the Multi-Krum selection (include/pgh_api.h, "Multi-Krum selection"): from the n x n matrix
// of squared distances among the included rows, score[a] = the f64 left fold, in ascending order of value, of
// the n - f - 2 smallest D[a][b], b != a; the m rows first in (score, position) order, reported as ascending
// positions in picked[0, *n_picked).  m = 0 means n - f.  Returns 0, or -1 when an off-diagonal entry is NaN
// or negative (an argument error), -3 when n < 2f + 3 or m > n - f (a state error); `scores` (n, nullable) is
// written whenever the matrix was acceptable and n >= 2f + 3.
int krum_select(const double* D, int n, int f, int m, int32_t* picked, int* n_picked, double* scores);

// K7's sum in K7's exact order (pgh_kernels.h) over (double)x[i] * (double)y[i], i < p, on the host: what K14
// returns for a row x against the plane y, and with y == x what K7 returns for x.  The trust root's s0 comes from
// here (pgh_trust_root): the same bits as pgh_row_sumsq of a slot holding the root.
double row_dot_host(const float* x, const float* y, int64_t p);

// Steps 2 and 4 of trust-bootstrapped FedAvg (include/pgh_api.h, "Trust-bootstrapped FedAvg"): from the root's
// sum of squares s0 and, per row in fold order, K7's sum sumsq[k] and K14's dot[k] (not read where sumsq[k] is
// not finite), the positions of the included rows (included[0, *n_included)), their fold weights
// (w[0, *n_included)) and T.  Returns 0, or -1 when s0 is not finite and > 0 (an argument error), -2 when no row
// is included, -3 when T == 0 (state errors; *n_included and, for -3, `included` are written all the same).
// n_trusted (rows with ts > 0) and max_w are nullable.
int trust_weights(double s0, const double* sumsq, const double* dot, int64_t n, float* w, int32_t* included,
                  int64_t* n_included, double* T, int64_t* n_trusted, float* max_w);

// The host side of a per-slot cache of one f64 that a kernel computes from the slot's diff (K7's sum of squares,
// K14's dot; RowCache in pgh_rules.h adds the buffers and the event).  A slot is NONE (no value of its present
// diff), QUEUED (the kernel and the D2H of its value are issued: the value is in the host image once the
// owner's event has passed) or VALID (at() holds it).  Whoever queues asks missing() first, launches, and
// marks what it launched; whoever reads waits for the event and harvests first.
struct SlotCache {
    enum : uint8_t { NONE = 0, QUEUED = 1, VALID = 2 };
    std::vector<uint8_t> state;   // per slot
    std::vector<double> value;    // per slot: what at() returns for a VALID one
    std::vector<int32_t> queued;  // the slots that went QUEUED since the last harvest

    double at(int slot) const { return value[(size_t)slot]; }  // after a harvest: the value of a slot queued before it
    bool anything_queued() const { return !queued.empty(); }
    void reserved(int slots) {  // the slab at a new length: every slot NONE, nothing queued
        state.assign((size_t)slots, (uint8_t)NONE);
        value.assign((size_t)slots, 0.0);
        queued.clear();
    }
    // The diffs in slots [slot, slot + n) are being replaced: their values were the old diffs'.  The one place a
    // value goes to NONE slot by slot; one that is QUEUED stays in the queued list and its harvest skips it.
    void written(int slot, int n) { std::fill_n(state.begin() + slot, n, (uint8_t)NONE); }
    // those of slots[0, n) that are NONE: once each, in list order
    std::vector<int32_t> missing(const int32_t* slots, int n) {
        std::vector<int32_t> todo;
        for (int k = 0; k < n; ++k)
            if (state[(size_t)slots[k]] == NONE) {
                todo.push_back(slots[k]);
                state[(size_t)slots[k]] = QUEUED;  // (a slot listed twice is taken once; put back below)
            }
        for (int32_t sl : todo) state[(size_t)sl] = NONE;
        return todo;
    }
    void mark_queued(const std::vector<int32_t>& todo) {  // their kernel and D2H are issued
        for (int32_t sl : todo) {
            state[(size_t)sl] = QUEUED;
            queued.push_back(sl);
        }
    }
    // The queued values have landed in host_image (indexed by slot): QUEUED -> VALID.  A slot that was written
    // after it was queued is NONE (or QUEUED again, and then listed again behind this entry, its new value
    // the one the image holds): its old value is never taken, a harvest resurrects nothing.
    void harvest(const double* host_image) {
        for (int32_t sl : queued)
            if (state[(size_t)sl] == QUEUED) {
                value[(size_t)sl] = host_image[sl];
                state[(size_t)sl] = VALID;
            }
        queued.clear();
    }
    // Every slot back to NONE and nothing to harvest.  all_stale: what the values were computed against has
    // changed (the owner has waited for what was in flight); forget: the diffs themselves are gone.
    void all_stale() {
        std::fill(state.begin(), state.end(), (uint8_t)NONE);
        queued.clear();
    }
    void forget() { all_stale(); }
    void clear() {  // the slab is freed: no slot at all
        state.clear();
        value.clear();
        queued.clear();
    }
};

}  // namespace pgh_detail
