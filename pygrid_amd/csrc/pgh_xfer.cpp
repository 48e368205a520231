// libpygrid_hip: host <-> HBM movement -- H2D through the pinned staging ring (or straight from
// page-locked memory), the D2H rings, the shard's spans of a State message, and the page-locked host
// blocks whose DMAs may outlive the call; the methods of the transfer owners (pgh_xfer.h).
// (struct pgh_ctx and the shared helpers: pgh_ctx.h)
#include "pgh_ctx.h"

namespace pgh_detail {

// Elements [i0, i0 + n) of one row from contiguous host memory: the partial first block, the
// whole blocks as ONE 2-D copy (block rows bstride apart), the partial last block.
int h2d_range(pgh_ctx* c, const Dest& d, int64_t i0, const uint8_t* src, int64_t n, hipStream_t s,
              size_t src_room) {
    const size_t es = d.es;
    if (n <= 0) return PGH_OK;
    c->ranged.copy_issued();
    if (d.map.bshift == 62) {
        CK(c, hipMemcpyAsync(d.base + (size_t)i0 * es, src, (size_t)n * es, hipMemcpyHostToDevice, s));
        return PGH_OK;
    }
    const int64_t bw = d.map.ld, i1 = i0 + n;
    int64_t i = i0;
    if (i & (bw - 1)) {  // head
        const int64_t e = std::min(i1, (i | (bw - 1)) + 1);
        CK(c, hipMemcpyAsync(d.base + (size_t)d.map.at(i) * es, src, (size_t)(e - i) * es, hipMemcpyHostToDevice, s));
        src += (size_t)(e - i) * es;
        i = e;
    }
    int64_t full = (i1 - i) / bw;
    const int64_t rest = (i1 - i) - full * bw;
    const bool pad = rest > 0 && d.len > 0 && i1 == d.len && src_room >= (size_t)(bw - rest) * es;
    if (pad) ++full;  // the row's partial last block as a whole one: one copy less per row
    if (full > 0) {
        CK(c, hipMemcpy2DAsync(d.base + (size_t)d.map.at(i) * es, (size_t)d.map.bstride * es, src, (size_t)bw * es,
                               (size_t)bw * es, (size_t)full, hipMemcpyHostToDevice, s));
        src += (size_t)(full * bw) * es;
        i = std::min(i1, i + full * bw);
    }
    if (i < i1)  // tail
        CK(c, hipMemcpyAsync(d.base + (size_t)d.map.at(i) * es, src, (size_t)(i1 - i) * es, hipMemcpyHostToDevice, s));
    return PGH_OK;
}

bool is_pinned(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeHost;
}

// ---- the transfer owners (pgh_xfer.h) ---------------------------------------------------------------
bool xfer_made(pgh_ctx* c) {
    if (const char* e = std::getenv("PGH_PINNED_GATHER")) c->gather.on = std::atoi(e) != 0;
    if (const char* e = std::getenv("PGH_D2H_STREAM")) c->d2h.mode = std::max(0, std::min(1, std::atoi(e)));
    c->d2h.own = c->d2h.mode > 0;
    bool ok = !c->d2h.own || c->d2h.s.make() == hipSuccess;  // (vdec.s, a fifth stream, only on first use)
    for (Event* ev : {&c->ring.ev[0], &c->ring.ev[1], &c->gather.tab.ev, &c->gather.dma_ev, &c->vdec.tab.ev,
                      &c->vdec.in, &c->vdec.buf[0].done, &c->vdec.buf[1].done})
        ok = ok && ev->make() == hipSuccess;
    return ok;
}

int StagingRing::take(pgh_ctx* c, int* slot) {
    *slot = next;
    next ^= 1;
    if (used[*slot]) CK(c, hipEventSynchronize(ev[*slot]));
    c->d2h.drop_pre();
    return PGH_OK;
}

int StagingRing::poll_free(pgh_ctx* c, int out[2], int* n) {
    for (int k = 0; k < 2; ++k) {
        if (used[k]) {
            const hipError_t q = hipEventQuery(ev[k]);
            if (q == hipErrorNotReady) continue;
            CK(c, q);
            used[k] = false;
        }
        out[(*n)++] = k;
    }
    return PGH_OK;
}

int StagingRing::wait_all(pgh_ctx* c) {
    for (int k = 0; k < 2; ++k) {
        CK(c, hipEventSynchronize(ev[k]));
        used[k] = false;
    }
    return PGH_OK;
}

int HostTable::upload(pgh_ctx* c, void* dev_dst, const void* src, size_t bytes, hipStream_t s) {
    if (used) CK(c, hipEventSynchronize(ev));  // the previous upload read the image
    if (bytes > h.cap()) {
        if (!h.reserve(bytes)) return fail(c, PGH_E_OOM, "%s of %zu bytes failed", what, bytes);
        used = false;
    }
    std::memcpy(h.as<void>(), src, bytes);
    c->ranged.copy_issued();
    CK(c, hipMemcpyAsync(dev_dst, h.as<void>(), bytes, hipMemcpyHostToDevice, s));
    CK(c, hipEventRecord(ev, s));
    used = true;
    return PGH_OK;
}

int RangedIngest::begin(pgh_ctx* c, int64_t pg, int* K) {
    *K = chunks(pg);
    if (!c->ev_pool.fill(ev, (size_t)*K)) return fail(c, PGH_E_HIP, "hipEventCreate failed");
    return PGH_OK;
}

int RangedIngest::wait_range(pgh_ctx* c, hipStream_t s, int64_t lo, int64_t hi) {
    for (int64_t k = lo / INGEST_CHUNK; k <= (hi - 1) / INGEST_CHUNK; ++k) CK(c, hipStreamWaitEvent(s, ev[(size_t)k], 0));
    return PGH_OK;
}

int RangedIngest::wait_all(pgh_ctx* c, hipStream_t s) {
    CK(c, hipStreamWaitEvent(s, ev[(size_t)(n - 1)], 0));
    return PGH_OK;
}

// Ranged report ingest (pgh_set_ingest_ranges) of concatenated fp32 host pieces holding the whole
// shard row: one pinned slot, filled and DMA'd chunk by chunk (INGEST_CHUNK params each, the host
// copy of chunk k + 1 beside the DMA of chunk k), the chunk's event behind its DMA.
int stage_pieces_h2d_ranged(pgh_ctx* c, const Dest& dst, const std::vector<Piece>& pieces, size_t total) {
    H2DTimer t(c);
    int K = 0, slot = 0;
    RC(c->ranged.begin(c, c->pg, &K));
    RC(c->ring.take(c, &slot));
    uint8_t* const pin = c->ring.at(slot);
    PieceCursor cur{pieces};
    for (int k = 0; k < K; ++k) {
        size_t a, b;
        ingest_chunk_bytes(c->pg, k, &a, &b);  // (total == 4 pg: the caller's condition)
        std::vector<CopyPool::Seg> segs;
        cur.take(pin + a, b - a, &segs);
        c->pool_copy->run(segs);
        RC(h2d_range(c, dst, (int64_t)(a / 4), pin + a, (int64_t)((b - a) / 4), c->copy,
                     b == total ? c->ring.slot_bytes - b : 0));
        RC(c->ranged.mark(c, k));
    }
    RC(c->ring.sent(c, slot, c->copy));
    c->ranged.commit(K);
    return t.done(total, total);
}

// Concatenated host pieces -> HBM at `dst`, through the pinned ring: each slot is filled by
// (multi-threaded) host copies of as many pieces as fit, then DMA'd while the next slot fills.
int stage_pieces_h2d(pgh_ctx* c, const Dest& dst, const std::vector<Piece>& pieces) {
    H2DTimer t(c);
    size_t total = 0, done = 0;
    for (auto& p : pieces) total += p.n;
    PieceCursor cur{pieces};
    while (done < total) {
        int slot = 0;
        RC(c->ring.take(c, &slot));
        std::vector<CopyPool::Seg> segs;
        const size_t fill = cur.take(c->ring.at(slot), c->ring.slot_bytes, &segs);
        c->pool_copy->run(segs);
        // slot fills are whole multiples of 4 KiB but the last, so `done` stays element-aligned
        RC(h2d_range(c, dst, (int64_t)(done / dst.es), c->ring.at(slot), (int64_t)(fill / dst.es), c->copy,
                     c->ring.slot_bytes - fill));
        RC(c->ring.sent(c, slot, c->copy));
        done += fill;
    }
    return t.done(total, total);
}

// host bytes -> HBM on the copy stream.  Page-locked sources are DMA'd directly (the call
// then waits for the copy: the caller's buffer is only borrowed); pageable sources go through
// the pinned ring, so the host memcpy of one slot overlaps the DMA of the other.
int stage_h2d(pgh_ctx* c, const Dest& dst, const uint8_t* src, size_t n, bool pinned_src) {
    if (!pinned_src) return stage_pieces_h2d(c, dst, {Piece{src, n}});
    H2DTimer t(c);
    RC(h2d_range(c, dst, 0, src, (int64_t)(n / dst.es), c->copy));
    CK(c, hipStreamSynchronize(c->copy));
    return t.done(n);
}

// The page-locked cells of piped rings on their own stream (d2h.own): at least `bytes` of cells.  Made
// on first use; grown only after every piece already on the stream has landed.  (The stream itself is made
// with the context -- pgh_create fails without it -- and primed by its warm-up.)
static int ensure_d2h_cells(pgh_ctx* c, size_t bytes) {
    if (c->d2h.h.cap() >= bytes) return PGH_OK;
    CK(c, hipStreamSynchronize(c->d2h.s));
    if (!c->d2h.h.reserve(bytes)) return fail(c, PGH_E_OOM, "page-locked D2H cells of %zu bytes failed", bytes);
    return PGH_OK;
}

int d2h_ring_begin(pgh_ctx* c, D2HRing* r, const uint8_t* src, size_t total, hipStream_t s, bool piped, bool may_wait) {
    *r = D2HRing{};
    r->src = src;
    r->total = total;
    r->piped = piped;
    if (piped && c->d2h.own) {  // up to D2H_OWN_CELLS pieces in flight, none of the staging slots held
        r->piece = D2H_PIECE;
        r->n_pieces = (total + r->piece - 1) / r->piece;
        RC(ensure_d2h_cells(c, std::min(r->n_pieces, D2H_OWN_CELLS) * r->piece));
        r->base = c->d2h.h.as<uint8_t>();
        r->cells = c->d2h.h.cap() / r->piece;
        r->per_slot = r->cells;
        r->s = c->d2h.s;
        if (!c->ev_pool.fill(c->d2h.ev, std::min(r->cells, r->n_pieces)))
            return fail(c, PGH_E_HIP, "hipEventCreate failed");
        return PGH_OK;
    }
    r->s = piped ? c->copy : s;
    r->piece = std::min(c->ring.slot_bytes, D2H_PIECE);
    r->per_slot = c->ring.slot_bytes / r->piece;  // >= 1 (slot_bytes >= 4096)
    // an earlier staged ingest may still read a slot: use the free ones, wait only if neither is
    RC(c->ring.poll_free(c, r->free_slot, &r->n_free));
    if (r->n_free == 0 && !may_wait) return PGH_OK;
    if (r->n_free == 0) {
        RC(c->ring.wait_all(c));
        r->n_free = 2;  // (free_slot is {0, 1} still)
    }
    r->cells = (size_t)r->n_free * r->per_slot;  // ring cells, one piece each
    r->n_pieces = (total + r->piece - 1) / r->piece;
    if (!c->ev_pool.fill(c->d2h.ev, std::min(r->cells, r->n_pieces))) return fail(c, PGH_E_HIP, "hipEventCreate failed");
    return PGH_OK;
}

static uint8_t* d2h_cell(const pgh_ctx* c, const D2HRing& r, size_t j) {
    if (r.base) return r.base + (j % r.cells) * r.piece;
    return c->ring.at(r.free_slot[(j % r.cells) / r.per_slot]) + (j % r.per_slot) * r.piece;
}

// Piece j of a piped ring: have all the fold ranges its floats come from finished?  (wait: block
// until they have.)  Marks may come from two streams (a split resident FINAL pass): every mark
// overlapping the piece is checked.
static int d2h_piece_ready(pgh_ctx* c, const D2HRing& r, size_t j, bool wait, bool* ready) {
    *ready = true;
    if (!r.piped) return PGH_OK;
    const size_t off = j * r.piece, len = std::min(r.piece, r.total - off);
    const int64_t first = (int64_t)(off / 4), last = (int64_t)((off + len + 3) / 4);
    int64_t start = 0;
    for (auto& m : c->final_marks) {
        if (start >= last) break;
        if (m.end > first) {
            if (wait) {
                CK(c, hipEventSynchronize(m.ev));
            } else {
                const hipError_t q = hipEventQuery(m.ev);
                if (q == hipErrorNotReady) { *ready = false; return PGH_OK; }
                CK(c, q);
            }
        }
        start = m.end;
    }
    return PGH_OK;
}

static int d2h_issue(pgh_ctx* c, D2HRing* r) {
    const size_t j = r->queued, off = j * r->piece, len = std::min(r->piece, r->total - off);
    CK(c, hipMemcpyAsync(d2h_cell(c, *r, j), r->src + off, len, hipMemcpyDeviceToHost, r->s));
    c->st.d2h_bytes_total += len;
    CK(c, hipEventRecord(c->d2h.ev[j % r->cells], r->s));
    ++r->queued;
    return PGH_OK;
}

static int d2h_issue_ready(pgh_ctx* c, D2HRing* r) {  // piped: every piece whose marks have fired, no wait
    while (r->queued < r->n_pieces && r->queued < r->done + r->cells) {
        bool ok = false;
        RC(d2h_piece_ready(c, *r, r->queued, false, &ok));
        if (!ok) break;
        RC(d2h_issue(c, r));
    }
    return PGH_OK;
}

// HBM bytes at `src` (after the work already on stream `s`) -> host pieces, through the pinned
// ring, in pieces of at most D2H_PIECE; the host copies piece k out as soon as it has landed while
// the later pieces' DMAs run.  `overlap`, if given, is host work run while the first DMA is in
// flight (the checkpoint template's framing copy).
//   Not piped: every piece that fits the ring (2 x 128 MiB by default) is queued at once on `s`.
//   marks (src is the resident checkpoint and its last fold left range marks): the pieces go on the
// copy stream, each issued once the host sees the ranges that wrote it finished (hipEventQuery /
// hipEventSynchronize), the first before the framing copy.  Issued that way the D2H runs on the
// SDMA engines beside the fold: queued with device-side waits on the marks, the runtime ran them as
// blit kernels (__amd_rocclr_copyBuffer) -- on the copy stream only after a stall, on any other
// stream always -- and each blit held the fold range beside it to a quarter of its speed (48 ->
// 182 us, profiles/r05d/, r05k/-r05m/).  The FINAL pass of a report-time close starts this itself
// (d2h.pre), issuing the pieces whose ranges are done while it issues the rest.
int stage_d2h_pieces(pgh_ctx* c, const uint8_t* src, const std::vector<OutPiece>& pieces, hipStream_t s,
                     const std::function<void()>& overlap, bool marks) {
    size_t total = 0;
    for (auto& p : pieces) total += p.n;
    if (total == 0) return PGH_OK;
    const bool piped = marks && !c->final_marks.empty();
    D2HRing r;
    if (piped && c->d2h.adopts(src, total)) {
        r = c->d2h.pre;  // started by the FINAL pass (its slots marked busy until now)
    } else {
        RC(d2h_ring_begin(c, &r, src, total, s, piped));
    }
    c->d2h.drop_pre();
    auto copy_out = [&](size_t j) {
        const size_t off = j * r.piece, len = std::min(r.piece, total - off);
        scatter_out(d2h_cell(c, r, j), off, len, pieces, *c->pool_copy);
    };
    const int rc = [&]() -> int {  // (on failure: drain the stream below)
        if (!piped) {
            while (r.queued < r.n_pieces && r.queued < r.cells) RC(d2h_issue(c, &r));
            if (overlap) overlap();
            for (; r.done < r.n_pieces; ++r.done) {
                CK(c, hipEventSynchronize(c->d2h.ev[r.done % r.cells]));
                copy_out(r.done);
                if (r.queued < r.n_pieces) RC(d2h_issue(c, &r));  // into the cell just copied out
            }
        } else {
            RC(d2h_issue_ready(c, &r));
            if (r.queued == r.done) {  // the first piece before the framing copy
                bool ok = false;
                RC(d2h_piece_ready(c, r, r.queued, true, &ok));
                RC(d2h_issue(c, &r));
            }
            if (overlap) overlap();
            while (r.done < r.n_pieces) {
                RC(d2h_issue_ready(c, &r));  // whatever finished, before a copy-out takes the thread
                if (r.done < r.queued) {
                    const hipError_t q = hipEventQuery(c->d2h.ev[r.done % r.cells]);
                    if (q == hipSuccess) {
                        copy_out(r.done++);
                        continue;
                    }
                    if (q != hipErrorNotReady) CK(c, q);
                    std::this_thread::yield();
                } else {  // nothing in flight: wait for the next piece's ranges
                    bool ok = false;
                    RC(d2h_piece_ready(c, r, r.queued, true, &ok));
                    RC(d2h_issue(c, &r));
                }
            }
        }
        return PGH_OK;
    }();
    if (rc != PGH_OK) (void)hipStreamSynchronize(r.s);  // no piece may still land in a slot handed out later
    for (int k = 0; k < r.n_free; ++k) c->ring.release(r.free_slot[k]);  // every piece landed
    return rc;
}

int D2HState::issue_pre(pgh_ctx* c) {
    const size_t before = pre.queued;
    RC(d2h_issue_ready(c, &pre));
    if (pre.queued > before)  // its slots are busy until these pieces land
        for (int k = 0; k < pre.n_free; ++k) RC(c->ring.sent(c, pre.free_slot[k], pre.s));
    return PGH_OK;
}

// The shard's slice of every tensor payload of a State message, as byte ranges of the message.
int state_shard_spans(pgh_ctx* c, const uint8_t* pb, size_t n, std::vector<std::pair<size_t, size_t>>* out,
                      const char* what) {
    std::vector<pgh_state::Span> spans;
    std::string msg;
    int rc = pgh_state::scan(pb, n, &spans, &msg);
    if (rc) return fail(c, rc, "%s State: %s", what, msg.c_str());
    if (spans.size() != c->numel.size())
        return fail(c, PGH_E_PARSE, "%s State holds %zu tensors, layout has %zu", what, spans.size(), c->numel.size());
    out->clear();
    int64_t off = 0;
    for (size_t t = 0; t < spans.size(); ++t) {
        if (spans[t].count != c->numel[t])
            return fail(c, PGH_E_PARSE, "%s tensor %zu holds %lld floats, layout %lld", what, t,
                        (long long)spans[t].count, (long long)c->numel[t]);
        const int64_t a = std::max(off, c->lo), b = std::min(off + spans[t].count, c->hi);
        if (a < b) out->push_back({spans[t].offset + 4 * (size_t)(a - off), 4 * (size_t)(b - a)});
        off += spans[t].count;
    }
    return PGH_OK;
}

// ---- page-locked blocks whose DMAs may outlive the ingest call -------------------------------------
// pgh_host_async marks a pgh_host_alloc block: an ingest from it then returns once the DMA is queued
// (not done), and records the DMA's event here; pgh_host_wait(p, n) waits for every DMA still reading
// [p, p + n) (any context, any GPU) before the owner reuses or frees the block.  Unmarked page-locked
// memory keeps the synchronous contract (the call waits for its copies).
struct HostDma { uintptr_t lo, hi; Event ev; };
std::mutex g_host_mu;
std::vector<std::pair<uintptr_t, uintptr_t>> g_async_blocks;  // [lo, hi)
std::vector<HostDma> g_host_dmas;

bool host_async(const void* p, size_t n) {
    const uintptr_t a = (uintptr_t)p, b = a + n;
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (auto& r : g_async_blocks)
        if (a >= r.first && b <= r.second) return true;
    return false;
}

// Record that a DMA reading [p, p + n) was queued on stream s (the event is recorded here).
int host_dma_queued(pgh_ctx* c, const void* p, size_t n, hipStream_t s) {
    Event ev;
    CK(c, ev.make());
    CK(c, hipEventRecord(ev, s));
    std::lock_guard<std::mutex> lk(g_host_mu);
    // forget DMAs that have finished (a block held elsewhere for long would otherwise collect them)
    auto keep = g_host_dmas.begin();
    for (auto& d : g_host_dmas)
        if (hipEventQuery(d.ev) != hipSuccess) *keep++ = std::move(d);
    g_host_dmas.erase(keep, g_host_dmas.end());
    (void)hipGetLastError();  // hipErrorNotReady from the queries above
    g_host_dmas.push_back({(uintptr_t)p, (uintptr_t)p + n, std::move(ev)});
    return PGH_OK;
}

}  // namespace pgh_detail

using namespace pgh_detail;

// (the public entry points take their C linkage from include/pgh_api.h)
int pgh_host_async(void* p, size_t n, int on) {
    if (!p || !n) return fail(nullptr, PGH_E_ARG, "bad block");
    if (!on) RC(pgh_host_wait(p, n));
    std::lock_guard<std::mutex> lk(g_host_mu);
    const std::pair<uintptr_t, uintptr_t> r{(uintptr_t)p, (uintptr_t)p + n};
    auto it = std::find(g_async_blocks.begin(), g_async_blocks.end(), r);
    if (on && it == g_async_blocks.end()) g_async_blocks.push_back(r);
    if (!on && it != g_async_blocks.end()) g_async_blocks.erase(it);
    return PGH_OK;
}

int pgh_host_wait(const void* p, size_t n) {
    const uintptr_t a = (uintptr_t)p, b = a + n;
    std::vector<Event> evs;  // destroyed on return, waited for or not
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto keep = g_host_dmas.begin();
        for (auto& d : g_host_dmas) {
            if (d.lo < b && a < d.hi) evs.push_back(std::move(d.ev));
            else *keep++ = std::move(d);
        }
        g_host_dmas.erase(keep, g_host_dmas.end());
    }
    int rc = PGH_OK;
    for (auto& ev : evs) {
        const hipError_t e = hipEventSynchronize(ev);
        if (e != hipSuccess && rc == PGH_OK) rc = fail(nullptr, PGH_E_HIP, "DMA from host buffer failed: %s",
                                                       hipGetErrorString(e));
    }
    return rc;
}

int pgh_host_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return fail(nullptr, PGH_E_ARG, "bad pinned allocation request");
    *out = nullptr;
    if (hipHostMalloc(out, bytes, hipHostMallocPortable) != hipSuccess) {  // DMA-able by every GPU of a group
        (void)hipGetLastError();
        *out = nullptr;
        return fail(nullptr, PGH_E_OOM, "pinned host allocation of %zu bytes failed", bytes);
    }
    return PGH_OK;
}

int pgh_host_prefault(void* p, size_t n) {
    if (!p || !n) return PGH_OK;
    const size_t per = (size_t)8 << 20;
    const int k = (int)std::min<size_t>(8, (n + per - 1) / per);
    if (k <= 1) {
        prefault_small_any((uint8_t*)p, n);
        return PGH_OK;
    }
    std::vector<std::thread> ts;
    const size_t step = (n + (size_t)k - 1) / (size_t)k;
    for (int i = 0; i < k; ++i) {
        const size_t a = (size_t)i * step, b = std::min(n, a + step);
        if (a < b) ts.emplace_back([=] { prefault_small_any((uint8_t*)p + a, b - a); });
    }
    for (auto& t : ts) t.join();
    return PGH_OK;
}

int pgh_host_free(void* p) {
    if (p) {
        size_t n = 0;
        {
            std::lock_guard<std::mutex> lk(g_host_mu);
            for (auto it = g_async_blocks.begin(); it != g_async_blocks.end(); ++it)
                if (it->first == (uintptr_t)p) {
                    n = it->second - it->first;
                    g_async_blocks.erase(it);
                    break;
                }
        }
        if (n) (void)pgh_host_wait(p, n);  // a DMA from the block may still be running
    }
    if (p && hipHostFree(p) != hipSuccess) return fail(nullptr, PGH_E_HIP, "hipHostFree failed");
    return PGH_OK;
}

namespace pgh_int {
int patch_payloads(pgh_ctx* c, const uint8_t* tmpl, size_t n, uint8_t* out) {
    RC(check_dtype(c, PGH_F32));
    if (!tmpl || !out) return fail(c, PGH_E_ARG, "tmpl / out is NULL");
    RC(check_ckpt(c, "pgh_ckpt_patch_state"));
    std::vector<std::pair<size_t, size_t>> spans;
    RC(state_shard_spans(c, tmpl, n, &spans, "checkpoint template"));
    DeviceGuard g(c->device);
    std::vector<OutPiece> pieces;
    for (auto& sp : spans) pieces.push_back(OutPiece{out + sp.first, sp.second});
    RC(order_after_ingest(c, c->stream));
    RC(stage_d2h_pieces(c, c->d_ckpt.as<uint8_t>(), pieces, c->stream, [&] {
        if (!spans.empty()) {  // this shard's part of the (fresh) output
            const size_t a = spans.front().first, b = spans.back().first + spans.back().second;
            if (b > a) prefault_parallel(out + a, b - a, *c->pool_copy);
        }
    }, true));
    return collect_timings(c);
}
}  // namespace pgh_int
