// What the transfer side of a single-GPU context keeps: one struct per protocol, members of struct pgh_ctx
// (pgh_ctx.h) as ring, d2h, ranged, vdec and gather.  Each keeps its own invariant; only its methods (pgh_xfer.cpp;
// the two on the per-piece loops inline in pgh_ctx.h) and the call sites named here touch its fields.
// xfer_made (pgh_create) makes their events and reads their knobs.  Not installed.
#pragma once
#include "pgh_host.h"
#include "pgh_res.h"

struct pgh_ctx;

namespace pgh_detail {

// The pinned staging ring: two page-locked slots through which pageable host bytes reach HBM, and which a
// D2H without cells of its own borrows.  A slot is busy from the DMA that reads or writes it (sent) until
// that event has fired (take, poll_free, wait_all) or its borrower has copied every piece out (release).
// The slots themselves are read by the staging loops, pgh_create (allocation on the GPU's socket, warm-up)
// and d2h_cell.
struct StagingRing {
    PinnedBuf h_pin[2];
    size_t slot_bytes = 0;
    Event ev[2];
    bool used[2] = {false, false};
    int next = 0;

    uint8_t* at(int slot) const { return h_pin[slot].as<uint8_t>(); }
    // the next slot, free of earlier DMAs; drops a pre-queued D2H ((conservative) its cells may be overwritten now)
    int take(pgh_ctx* c, int* slot);
    int sent(pgh_ctx* c, int slot, hipStream_t s);  // a DMA on `s` uses the slot: busy until it is done
    // an earlier staged ingest may still read a slot: the ones that are free now, without waiting
    int poll_free(pgh_ctx* c, int out[2], int* n);
    int wait_all(pgh_ctx* c);  // both slots free
    void release(int slot) { used[slot] = false; }  // every piece of the borrower has landed
};

// A page-locked host image of a small device table.  It may be rewritten only after its last upload:
// upload waits for that upload's event, grows the image, copies `src` in, issues the H2D (a counted copy
// on the copy stream), records the event.
struct HostTable {
    const char* what;  // leads the message of a failed allocation
    PinnedBuf h;
    Event ev;
    bool used = false;
    explicit HostTable(const char* what_) : what(what_) {}
    int upload(pgh_ctx* c, void* dev_dst, const void* src, size_t bytes, hipStream_t s);
};

// Ranged report ingest (pgh_set_ingest_ranges): a State diff goes to HBM in chunks of INGEST_CHUNK params
// (pgh_host.h), each followed by ev[k] on the copy stream, so that the FINAL pass of a report-time close
// that starts while the last report's DMA is still in flight folds each param range as soon as its bytes
// have landed.  copy_ops counts the data operations issued on the copy stream -- every one of them gets
// there through copy_issued: h2d_range, the table uploads, a share message's DMA, the synthetic fill (on
// the fold stream in STREAM mode too: conservative) -- and the ranged close applies only while
// seq == copy_ops (nothing issued since the latest ranged ingest) and n chunks cover the shard.
struct RangedIngest {
    bool on = false;
    std::vector<hipEvent_t> ev;  // ev_pool's
    uint64_t copy_ops = 0, seq = ~0ull;
    int n = 0;

    static int chunks(int64_t pg) { return ingest_chunks(pg); }
    void copy_issued() { ++copy_ops; }
    int begin(pgh_ctx* c, int64_t pg, int* K);  // events for the K = chunks(pg) chunks of an ingest
    int mark(pgh_ctx* c, int k);                // chunk k is on the copy stream
    void commit(int K) { seq = copy_ops; n = K; }  // every chunk marked
    // Whether the FINAL pass of a slot fold may wait per param range on the latest ranged ingest instead
    // of on every copy issued (order_after_ingest): nothing else went to the copy stream since.
    bool valid(int64_t pg) const { return on && seq == copy_ops && n == chunks(pg); }
    int wait_range(pgh_ctx* c, hipStream_t s, int64_t lo, int64_t hi);  // every chunk params [lo, hi) lie in
    int wait_all(pgh_ctx* c, hipStream_t s);                            // the last chunk: all of them
};

constexpr size_t D2H_OWN_CELLS = 8;  // a piped ring's own cells: 64 MiB at most (ResNet-18: 6 pieces)

// A staged D2H through the pinned ring: pieces of `piece` bytes of [src, src + total) into the
// cells of the free pinned slots, each followed by D2HState::ev[cell].  piped: src is a fold's result
// with range marks; each piece is issued (on the copy stream) once the host sees every mark
// covering it complete -- no cross-stream wait on the device, which sent the pieces to blit
// kernels that slowed the ranges beside them (profiles/r05k/-r05m/, r05aa/).
struct D2HRing {
    const uint8_t* src = nullptr;
    size_t total = 0, piece = 0, per_slot = 0, cells = 0, n_pieces = 0, queued = 0, done = 0;
    int free_slot[2] = {0, 1};
    int n_free = 0;
    hipStream_t s = nullptr;
    bool piped = false;
    uint8_t* base = nullptr;  // (not owned) the cells of a piped ring: D2HState::h (own), else the free pinned slots
};

struct D2HState {
    std::vector<hipEvent_t> ev;  // one per ring cell of a staged D2H (stage_d2h_pieces); ev_pool's
    // The new checkpoint's D2H as the FINAL pass of a report-time close starts it: the pieces whose
    // ranges finished while the later ranges were still being issued (pgh_slots.cpp); the patch /
    // download that follows adopts the ring.  Dropped with the marks (clear_final_marks), when a
    // staging copy takes a pinned slot (StagingRing::take) or when a D2H begins (stage_d2h_pieces).
    D2HRing pre;
    bool pre_valid = false;
    // A piped ring's pieces on a stream and in page-locked cells of their own (PGH_D2H_STREAM,
    // default 1): on the copy stream they queued behind the last reports' H2D, and they waited for
    // a staging slot those reports still held -- with reports back to back, until every report had
    // landed.  The stream is made with the context and primed by its warm-up with a small H2D, so the
    // runtime sends its D2H to an SDMA engine (r05ae; an unprimed stream's D2H went to blit kernels that
    // share the CUs with the fold, r05k/-r05x/).  (Rounds 6's K6 k_copy_to_host, pieces copied out by a
    // kernel beside an H2D backlog, was removed: copying a piece right behind the FINAL ranges that wrote
    // it on another stream, it read ranges that had not run yet -- profiles/r06s/.)
    bool own = true;
    int mode = 1;
    Stream s;
    PinnedBuf h;

    void drop_pre() { pre_valid = false; }
    // the pre-queued ring survives its FINAL pass if it read what is the resident checkpoint now
    void keep_pre(bool queued, const void* ckpt) { pre_valid = queued && pre.src == ckpt; }
    bool adopts(const uint8_t* src, size_t total) const { return pre_valid && pre.src == src && pre.total == total; }
    // After a range mark of the FINAL pass: the pieces of `pre` whose ranges are done go out; the staging
    // slots it borrowed are busy until they land.
    int issue_pre(pgh_ctx* c);
};

// secagg shares as State bytes: varint payloads in HBM + their chunk table (k_varint_decode).
// Each decode runs on its own stream (s) behind its message's DMAs, so the copy stream's next
// DMA does not queue behind it; the HBM bytes and chunk table alternate between two buffers (the
// DMA of one message beside the decode of the one before).
struct VarintBuf {
    DeviceBuf bytes;
    DeviceBuf tab;  // pgh::VChunk
    Event done;     // the last decode that read this buffer
    bool used = false;
};
struct VarintDecode {
    VarintBuf buf[2];
    int next = 0;
    Stream s;                            // made on first use: a context's fifth stream
    Event in;                            // copy stream -> s: a message's bytes and table have landed
    hipEvent_t last = nullptr;           // (a buf's `done`, not owned) the last decode issued
    HostTable tab{"pinned chunk table"};  // host image of a chunk table (pgh::VChunk)

    VarintBuf& take() { VarintBuf& b = buf[next]; next ^= 1; return b; }
    hipEvent_t last_decode() const { return last; }  // folds wait for it; nullptr: none issued yet
};

// page-locked fp32 State messages (pgh_ingest_state): DMA'd whole into d_bytes, gathered into the
// slab row by k_gather_f32 with the chunk table d_tab (PGH_PINNED_GATHER=0: one DMA per payload piece)
struct PinnedGather {
    bool on = true;
    DeviceBuf d_bytes;
    DeviceBuf d_tab;  // pgh::GChunk
    HostTable tab{"gather chunk table"};
    Event dma_ev;     // the last message DMA (the caller's buffer is free after it)
};

// pgh_create, after the context's streams: the owners' events, PGH_PINNED_GATHER and PGH_D2H_STREAM, the D2H
// stream; false fails it
bool xfer_made(pgh_ctx* c);

}  // namespace pgh_detail
