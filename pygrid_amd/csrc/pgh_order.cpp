// libpygrid_hip: every rule about which stream waits for what -- folds after ingest copies, ingest
// copies after the folds that read a slot, the STREAM fold marks, the range marks of a FINAL pass,
// the aux and caller-stream joins -- and the timing events around the launches.
// (struct pgh_ctx and the shared helpers: pgh_ctx.h)
#include "pgh_ctx.h"

namespace pgh_detail {

// Timing events (timed_launch) only measure: no system-scope fence when they complete.  With the
// default flags each one made the kernel after it start 15-22 us after the one before, against 5-7
// without (tools/exp_close_pipeline.hip, profiles/r05e/): 12 range launches of a report-time close
// lost ~0.15 ms to them.  Every host read of a result still goes through a copy with its own sync.
hipEvent_t take_event(pgh_ctx* c) { return c->timing_pool.take(); }

int collect_timings(pgh_ctx* c) {
    // busy time: union of the launches' intervals, placed on one clock relative to the first start
    std::vector<std::pair<double, double>> iv;
    iv.reserve(c->pending.size());
    for (auto& t : c->pending) {
        CK(c, hipEventSynchronize(t.b));
        float ms = 0.f, t0 = 0.f;
        CK(c, hipEventElapsedTime(&ms, t.a, t.b));
        CK(c, hipEventElapsedTime(&t0, c->pending.front().a, t.a));
        iv.push_back({(double)t0, (double)t0 + ms});
        c->st.kernel_ms_last = ms;
        c->st.kernel_ms_total += ms;
        c->st.kernel_launches += 1;
        c->st.kernel_bytes_last = t.bytes;
        c->st.kernel_bytes_total += t.bytes;
        c->timing_pool.give(t.a);
        c->timing_pool.give(t.b);
    }
    c->pending.clear();
    std::sort(iv.begin(), iv.end());
    double busy = 0, lo = 0, hi = 0;
    bool open = false;
    for (auto& x : iv) {
        if (open && x.first <= hi) { hi = std::max(hi, x.second); continue; }
        if (open) busy += hi - lo;
        lo = x.first; hi = x.second; open = true;
    }
    if (open) busy += hi - lo;
    c->st.kernel_busy_ms_total += busy;
    return PGH_OK;
}

// ---- pipelined close: range marks of the last resident fold ---------------------------------------
void clear_final_marks(pgh_ctx* c) {
    for (auto& m : c->final_marks) c->ev_pool.give(m.ev);
    c->final_marks.clear();
    c->d2h.drop_pre();
}

int add_final_mark(pgh_ctx* c, hipStream_t s, int64_t end) {
    hipEvent_t e = c->ev_pool.take();
    if (!e) return fail(c, PGH_E_HIP, "hipEventCreate failed");
    CK(c, hipEventRecord(e, s));
    c->final_marks.push_back({end, e});
    return PGH_OK;
}

// The ranges of a split FINAL pass alternate over `s` and the aux stream, so range k + 1 starts
// while range k drains its last workgroups instead of after (one stream costs the drain once per
// range: r02n group line, 4 launches 7.38 ms vs one 6.80 ms).  fork: aux after everything issued
// on s; join: s after everything issued on aux.
hipStream_t range_stream(const pgh_ctx* c, hipStream_t s, int k) {
    return (k & 1) ? c->aux : s;
}
int fork_aux(pgh_ctx* c, hipStream_t s) {
    CK(c, hipEventRecord(c->aux_ev, s));
    CK(c, hipStreamWaitEvent(c->aux, c->aux_ev, 0));
    return PGH_OK;
}
int join_aux(pgh_ctx* c, hipStream_t s) {
    CK(c, hipEventRecord(c->aux_ev, c->aux));
    CK(c, hipStreamWaitEvent(s, c->aux_ev, 0));
    return PGH_OK;
}

// Ranges of a FINAL fold pass: 1, or final_split 4-aligned ranges of the shard.
int final_ranges(const pgh_ctx* c) { return c->final_split > 1 && c->pg >= (1 << 20) ? c->final_split : 1; }
int64_t range_edge(const pgh_ctx* c, int k, int K) { return k >= K ? c->pg : (c->pg * k / K) & ~(int64_t)3; }

// Stream `s` waits for every ingest copy / synthetic fill / varint decode issued so far.
int order_after_ingest(pgh_ctx* c, hipStream_t s) {
    CK(c, hipEventRecord(c->copy_done, c->copy));
    CK(c, hipStreamWaitEvent(s, c->copy_done, 0));
    if (hipEvent_t dec = c->vdec.last_decode()) CK(c, hipStreamWaitEvent(s, dec, 0));
    return PGH_OK;
}

void release_slot_fold_events(pgh_ctx* c) {
    for (auto& fe : c->slab_evs) c->ev_pool.give(fe.second);
    c->slab_evs.clear();
    for (auto& r : c->slot_ring) c->ev_pool.give(r.second);
    c->slot_ring.clear();
    std::fill(c->slot_read_seq.begin(), c->slot_read_seq.end(), 0);
}

// A slot fold reading `slots` was issued on c->stream.
int record_slot_fold(pgh_ctx* c, const int32_t* slots, int n) {
    hipEvent_t ev = c->ev_pool.take();
    if (!ev) return fail(c, PGH_E_HIP, "hipEventCreate failed");
    CK(c, hipEventRecord(ev, c->stream));
    const int64_t seq = ++c->slot_seq;
    c->slot_ring.push_back({seq, ev});
    for (int k = 0; k < n; ++k) c->slot_read_seq[(size_t)slots[k]] = seq;
    while (c->slot_ring.size() > 64) {  // an older fold is done when a newer one on its stream is
        c->ev_pool.give(c->slot_ring.front().second);
        c->slot_ring.pop_front();
    }
    return PGH_OK;
}

// RESIDENT: before the copy stream overwrites `slot`, it waits for the folds that may still read it.
int order_slot_overwrite(pgh_ctx* c, int slot) {
    for (auto& fe : c->slab_evs) CK(c, hipStreamWaitEvent(c->copy, fe.second, 0));
    for (auto& fe : c->slab_evs) c->ev_pool.give(fe.second);
    c->slab_evs.clear();
    const int64_t seq = c->slot_read_seq[(size_t)slot];
    if (seq == 0 || c->slot_ring.empty()) return PGH_OK;
    hipEvent_t ev = c->slot_ring.back().second;
    for (auto& r : c->slot_ring)
        if (r.first >= seq) { ev = r.second; break; }  // that fold, or a later one on c->stream
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return PGH_OK;
    if (q != hipErrorNotReady) return fail(c, PGH_E_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
    (void)hipGetLastError();
    CK(c, hipStreamWaitEvent(c->copy, ev, 0));
    return PGH_OK;
}

// Before the copy stream overwrites a slot, it waits for every fold issued so far (the last one
// on each stream that ran folds).
int order_before_overwrite(pgh_ctx* c) {
    for (auto& fe : c->fold_evs) CK(c, hipStreamWaitEvent(c->copy, fe.second, 0));
    for (auto& fe : c->fold_evs) c->ev_pool.give(fe.second);
    c->fold_evs.clear();
    return PGH_OK;
}

// Remember the fold just issued on stream s: the stream's event in `evs` (fold_evs / slab_evs).
int record_fold(pgh_ctx* c, std::vector<std::pair<hipStream_t, hipEvent_t>>& evs, hipStream_t s) {
    hipEvent_t ev = nullptr;
    for (auto& fe : evs)
        if (fe.first == s) ev = fe.second;
    if (!ev) {
        if (!(ev = c->ev_pool.take())) return fail(c, PGH_E_HIP, "hipEventCreate failed");
        evs.push_back({s, ev});
    }
    CK(c, hipEventRecord(ev, s));
    return PGH_OK;
}

void clear_marks(pgh_ctx* c) {
    for (auto& m : c->marks) c->ev_pool.give(m.ev);
    c->marks.clear();
}

// STREAM: the slots of clients up to `last_client` held clients up to last_client - R before;
// the copy stream waits for the fold that consumed those.
int order_stream_overwrite(pgh_ctx* c, int64_t last_client) {
    const int64_t prev = last_client - c->slots;
    while (!c->marks.empty() && c->marks.front().upto <= c->folded - c->slots) {
        c->ev_pool.give(c->marks.front().ev);  // no future claim needs it
        c->marks.pop_front();
    }
    if (prev < 0) return PGH_OK;  // first pass over the ring (pgh_stream_begin drained older folds)
    for (auto& m : c->marks)
        if (m.upto > prev) {
            CK(c, hipStreamWaitEvent(c->copy, m.ev, 0));
            return PGH_OK;
        }
    return order_before_overwrite(c);
}

int record_mark(pgh_ctx* c, hipStream_t s, int64_t upto) {
    hipEvent_t e = c->ev_pool.take();
    if (!e) return fail(c, PGH_E_HIP, "hipEventCreate failed");
    CK(c, hipEventRecord(e, s));
    c->marks.push_back({e, upto});
    return PGH_OK;
}

// caller stream `cs` -> context stream ordering, and back
int join_in(pgh_ctx* c, hipStream_t cs) {
    if (cs == c->stream) return PGH_OK;
    CK(c, hipEventRecord(c->xsync, cs));
    CK(c, hipStreamWaitEvent(c->stream, c->xsync, 0));
    return PGH_OK;
}
int join_out(pgh_ctx* c, hipStream_t cs) {
    if (cs == c->stream) return PGH_OK;
    CK(c, hipEventRecord(c->xsync, c->stream));
    CK(c, hipStreamWaitEvent(cs, c->xsync, 0));
    return PGH_OK;
}

}  // namespace pgh_detail
