"""GPU: a context's whole life, twenty times over.  Each context is taken through every resource it
makes lazily (clip buffers, the gather tables of a page-locked State message, the varint buffers and
their decode stream, a superseded reciprocal table, range marks and the page-locked D2H cells), with
every result bit-exact against the oracle, and is then destroyed: device memory must come back."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
from oracle import coracle  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MEAN, ITERATIVE, CLIPPED, I64 = 0, 1, 3, 1
NUMEL = [4096, 3]          # P = 4,099: one float past a SUMSQ_TILE, not a multiple of 64
P_STREAM = 67
STREAM_N = (4_100, 8_200)  # clients: past the first reciprocal table (4,096), then past the second (8,192)
P_REPORT = (1 << 20) + 3   # the smallest shard whose report-time close runs as ranges with marks
SEED, BOUND = 91, 1.0


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def split(flat, numel):
    out, o = [], 0
    for n in numel:
        out.append(flat[o:o + n])
        o += n
    return out


@pytest.fixture(scope="module")
def case():
    """Inputs and what the oracle makes of them, computed once for all twenty contexts."""
    from pygrid_amd.state_schema import build_state_fast, build_state_i64_fast

    rng = np.random.default_rng(SEED)
    P = sum(NUMEL)
    k = {"ckpt": rng.standard_normal(P).astype(F)}
    # norms of about 0.64, 1.28, 1.92: the bound of 1 leaves row 0 alone and clips rows 1 and 2
    k["diffs"] = np.stack([(rng.standard_normal(P) * 1e-2 * (i + 1)).astype(F) for i in range(3)])
    scales = CO.scales(k["diffs"], BOUND)
    assert [bool(s == 1) for s in scales] == [True, False, False]
    k["mean"] = coracle.fedavg(MEAN, k["diffs"], k["ckpt"])
    k["clipped"] = CO.fedavg_clipped(k["ckpt"], list(k["diffs"]), BOUND)
    pinned_diff = (rng.standard_normal(P) * 1e-2).astype(F)
    k["pinned_msg"] = build_state_fast(split(pinned_diff, NUMEL))
    k["pinned_mean"] = coracle.fedavg(MEAN, np.stack([k["diffs"][0], pinned_diff, k["diffs"][2]]), k["ckpt"])
    # shares: two clients of 1-byte varints, then one of 10-byte varints (negative values)
    sh = rng.integers(0, 100, (3, 2, P), dtype=np.int64)
    sh[2] = rng.integers(-2**63, -2**62, (2, P), dtype=np.int64)
    k["share_msgs"] = [[build_state_i64_fast(split(sh[c, s], NUMEL)) for s in range(2)] for c in range(3)]
    assert min(len(m) for m in k["share_msgs"][2]) >= 1.5 * max(len(m) for c in (0, 1) for m in k["share_msgs"][c])
    k["sum"] = O.secagg_sum(sh)
    k["dec"] = O.fix_prec_decode(k["sum"])
    idx = np.arange(P_STREAM, dtype=np.uint64)
    synth = np.stack([O.synth_diff(SEED, c, idx) for c in range(max(STREAM_N))])
    k["stream_ckpt"] = rng.standard_normal(P_STREAM).astype(F)
    k["stream"] = [coracle.fedavg(ITERATIVE, synth[:n], k["stream_ckpt"]) for n in STREAM_N]
    rc = (rng.standard_normal(P_REPORT) * 0.05).astype(F)
    rd = (rng.standard_normal((3, P_REPORT)) * 1e-2).astype(F)
    k["report_ckpt_msg"] = build_state_fast([rc])
    k["report_msgs"] = [build_state_fast([d]) for d in rd]
    k["report"] = coracle.fedavg(MEAN, rd, rc)
    return k


def one_life(k):
    from pygrid_amd import Engine, PinnedBuffer
    from pygrid_amd.state_schema import parse_state

    with Engine(0, pinned_bytes=16 << 20) as eng:
        eng.set_layout(NUMEL)
        eng.reserve(3)
        for c, d in enumerate(k["diffs"]):
            eng.ingest(c, d)
        assert np.array_equal(u32(eng.fedavg(MEAN, k["ckpt"])), u32(k["mean"]))
        eng.set_clip_norm(BOUND)  # the clip buffers and their event
        assert np.array_equal(u32(eng.fedavg(CLIPPED, k["ckpt"])), u32(k["clipped"]))
        assert eng.clip_stats()["clipped"] == 2
        msg = PinnedBuffer((len(k["pinned_msg"]),), np.uint8)  # d_vbytes, the gather tables, their events
        try:
            msg.array[:] = np.frombuffer(k["pinned_msg"], np.uint8)
            eng.ingest_state(1, msg.array)
            assert np.array_equal(u32(eng.fedavg(MEAN, k["ckpt"])), u32(k["pinned_mean"]))
        finally:
            msg.free()
        eng.reserve(3, I64, 2)  # frees the slab with the clip buffers live
        for c in range(3):      # the dec stream, both varint buffers, h_vtab; client 2 regrows them
            eng.ingest_state_shares(c, k["share_msgs"][c])
        s, dec = eng.secagg(10, 3)
        assert np.array_equal(s, k["sum"]) and np.array_equal(u32(dec), u32(k["dec"]))
        eng.set_layout([P_STREAM])
        eng.reserve(128)
        for n, want in zip(STREAM_N, k["stream"]):  # a superseded reciprocal table is kept until destroy
            eng.stream_begin(ITERATIVE, 64)
            for c0 in range(0, n, 64):
                eng.synth_ingest(SEED, c0, min(64, n - c0))
            assert np.array_equal(u32(eng.stream_finish(k["stream_ckpt"])), u32(want))
        eng.set_layout([P_REPORT])
        eng.reserve(3)
        eng.ckpt_upload_state(k["report_ckpt_msg"])
        for c, m in enumerate(k["report_msgs"]):
            eng.ingest_state(c, m)
        eng.fold_slots_finish_resident(MEAN, [0, 1, 2])  # final marks, the D2H cells and their events
        patched = parse_state(eng.ckpt_patch_state(k["report_ckpt_msg"]))
        assert np.array_equal(u32(np.asarray(patched[0]).reshape(-1)), u32(k["report"]))
        assert np.array_equal(u32(eng.ckpt_download()), u32(k["report"]))


def test_twenty_contexts_made_used_and_destroyed_return_their_memory(case):
    import torch

    hip = C.CDLL("libamdhip64.so.7")

    def dev_free():
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    from pygrid_amd import Engine

    torch.cuda.synchronize()
    # In a process whose first context is a full life, the HIP runtime takes 136 MiB more, once, in the
    # second full life (measured: 292 MiB below the start after the first, 428 MiB after the second and
    # after every later one; the same with the library as it was before the owners).  After bare
    # contexts the first life takes all of it (156 MiB, then 292 MiB for good), so three of them come
    # before the one warm-up life and the before-value holds every one-time allocation.
    for _ in range(3):
        with Engine(0, pinned_bytes=16 << 20):
            pass
    one_life(case)  # warm: the runtime's one-time allocations
    free0 = dev_free()
    below = []
    for _ in range(20):
        one_life(case)
        below.append((free0 - dev_free()) >> 10)
    free1 = dev_free()
    print("free device memory below the start after each context, KiB:", below)
    assert free0 - free1 < (8 << 20), f"device memory fell by {(free0 - free1) >> 20} MiB over 20 contexts"
