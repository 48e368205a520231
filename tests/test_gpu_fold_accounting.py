"""GPU: what pgh_stats accounts for every fold launch -- kernel_launches, kernel_bytes_last,
kernel_bytes_total and n_folded -- on both native fold drivers (RESIDENT / range / STREAM folds and
report-time slot folds), for every fp32 rule and the share sum.  The expected values are closed forms
of the row count, the param count, the trim count and the party count; benchlib's achieved-bandwidth
figures are these bytes over the kernel time."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import launch_shapes as LS  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MEAN, ITERATIVE, WEIGHTED, CLIPPED, TRIMMED, MEDIAN, STREAM_SECAGG = 0, 1, 2, 3, 4, 5, 16
I64 = 1
P = 259  # one 256-column tile and three params
CLIP_BOUND = 40.0  # row k's norm is about 16.1 (k + 1): rows 0 and 1 stay, the others are scaled


def fold_bytes(rows, ln, first, final):
    """One fp32 fold launch: the rows, the running state in (not FIRST), the state out or ckpt in + out."""
    return 4 * rows * ln + (0 if first else 4 * ln) + (8 * ln if final else 4 * ln)


def trim_state_bytes(b, ln, first, final):
    """K8's 2b state planes: read unless FIRST, written unless FINAL."""
    return (0 if first else 2 * b * 4 * ln) + (0 if final else 2 * b * 4 * ln)


def secagg_bytes(rows, ln, first, final, want_sum=True, want_dec=True):
    out = ((8 * ln if want_sum else 0) + (4 * ln if want_dec else 0)) if final else 8 * ln
    return 8 * rows * ln + (0 if first else 8 * ln) + out


def k7_bytes(rows, p):
    """One K7 launch: the rows once, a double per 4096-param tile and row."""
    return rows * (4 * p + 8 * -(-p // 4096))


def launch_bytes(mode, b, rows, ln, first, final):
    if mode == MEDIAN:  # K9: the rows once, ckpt in, out
        return 4 * rows * ln + 8 * ln
    return fold_bytes(rows, ln, first, final) + (trim_state_bytes(b, ln, first, final) if mode == TRIMMED else 0)


def measured(eng, fn, *a):
    """(result, stats) of one call."""
    eng.reset_stats()
    r = fn(*a)
    return r, eng.stats()


def check(st, launches, n_folded, what=None):
    """st holds exactly these launches' bytes, in this order."""
    print(what, "launches", st["kernel_launches"], "last", st["kernel_bytes_last"], "total", st["kernel_bytes_total"],
          "n_folded", st["n_folded"], "want", launches, n_folded)
    assert st["kernel_launches"] == len(launches), what
    assert st["kernel_bytes_total"] == sum(launches), what
    assert st["kernel_bytes_last"] == (launches[-1] if launches else 0), what
    assert st["n_folded"] == n_folded, what


def rows_of(n, p, seed=0):
    """Row k has entries near +-(k + 1): an L2 norm of about (k + 1) sqrt(p)."""
    rng = np.random.default_rng(1000 * p + n + seed)
    sign = rng.choice(np.array([-1, 1], F), size=(n, p))
    return (sign * (np.arange(1, n + 1, dtype=F)[:, None] + rng.random((n, p), dtype=F) * F(0.01))).astype(F)


def ckpt_of(p):
    return np.random.default_rng(p).standard_normal(p).astype(F)


def load(eng, diffs, clip=0.0, trim=0, weights=True):
    """A fresh slab holding diffs (reserve zeroes n_folded and the clip totals).  The clip bound is set
    before the ingests, so every row's K7 launch happens at ingest time."""
    eng.set_layout([diffs.shape[1]])
    eng.reserve(len(diffs))
    eng.set_clip_norm(clip)
    eng.set_trim(trim)
    for k, d in enumerate(diffs):
        eng.ingest(k, d)
    if weights:
        eng.set_weights(np.arange(1, len(diffs) + 1, dtype=F))


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_clip_norm(0.0)
    engine.set_trim(0)
    engine.set_layout([8])


def check_clip_stats(eng, diffs):
    norms = np.sqrt((diffs.astype(np.float64) ** 2).sum(1))
    cs = eng.clip_stats()
    assert cs["rows"] == len(diffs) and cs["clipped"] == int((norms > CLIP_BOUND).sum()) and 0 < cs["clipped"] < len(diffs)
    assert cs["max_norm"] == pytest.approx(norms.max(), rel=1e-12)


RULES = [(MEAN, 0), (ITERATIVE, 0), (WEIGHTED, 0), (TRIMMED, 1), (CLIPPED, 0), (MEDIAN, 0)]
RULE_IDS = ["mean", "iterative", "weighted", "trimmed", "clipped", "median"]


@pytest.mark.parametrize("mode,b", RULES, ids=RULE_IDS)
def test_resident_whole_shard(eng, mode, b):
    """One launch over the five rows; a FIRST | FINAL trimmed fold moves no state planes."""
    n = 5
    diffs, ckpt = rows_of(n, P), ckpt_of(P)
    eng.set_layout([P])
    eng.reserve(n)
    eng.set_clip_norm(CLIP_BOUND if mode == CLIPPED else 0.0)
    eng.set_trim(b)
    eng.reset_stats()
    for k, d in enumerate(diffs):
        eng.ingest(k, d)
    eng.set_weights(np.arange(1, n + 1, dtype=F))
    # the ingest-time K7 launches: one per row with a bound set, all of them before the fold
    check(eng.stats(), [k7_bytes(1, P)] * (n if mode == CLIPPED else 0), 0, "ingest")
    _, st = measured(eng, eng.fedavg, mode, ckpt)
    check(st, [launch_bytes(mode, b, n, P, True, True)], 0, "fold")
    if mode == CLIPPED:
        check_clip_stats(eng, diffs)
        _, st = measured(eng, eng.fedavg, mode, ckpt)  # the scales are kept: no K7, no second count
        check(st, [fold_bytes(n, P, True, True)], 0, "second fold")
        check_clip_stats(eng, diffs)


def test_resident_clipped_with_the_bound_set_after_the_ingests(eng):
    """The fold finds no sums: one K7 launch over the five contiguous rows, then the weighted fold."""
    n = 5
    diffs, ckpt = rows_of(n, P), ckpt_of(P)
    load(eng, diffs)
    eng.set_clip_norm(CLIP_BOUND)
    _, st = measured(eng, eng.fedavg, CLIPPED, ckpt)
    check(st, [k7_bytes(n, P), fold_bytes(n, P, True, True)], 0)
    check_clip_stats(eng, diffs)


@pytest.mark.parametrize("mode,b", RULES, ids=RULE_IDS)
def test_resident_two_device_ranges(eng, mode, b):
    import torch

    n, cut = 5, 128
    diffs, ckpt = rows_of(n, P), ckpt_of(P)
    load(eng, diffs, clip=CLIP_BOUND if mode == CLIPPED else 0.0, trim=b)
    ck = torch.from_numpy(ckpt).cuda()
    whole, parts = torch.zeros_like(ck), torch.zeros_like(ck)
    _, st = measured(eng, eng.fedavg_device, mode, ck.data_ptr(), whole.data_ptr())
    check(st, [launch_bytes(mode, b, n, P, True, True)], 0, "whole")
    for off, ln in ((0, cut), (cut, P - cut)):
        _, st = measured(eng, eng.fedavg_device_range, mode, off, ln, ck.data_ptr(), parts.data_ptr())
        check(st, [launch_bytes(mode, b, n, ln, True, True)], 0, (off, ln))
    torch.cuda.synchronize()
    assert np.array_equal(parts.cpu().numpy().view(np.uint32), whole.cpu().numpy().view(np.uint32))


def shares_of(n, parties, p):
    return np.random.default_rng(p + n).integers(-2**62, 2**62, size=(n, parties, p), dtype=np.int64)


def test_resident_secagg_two_device_ranges(eng):
    import torch

    n, parties, cut = 5, 3, 128
    shares = shares_of(n, parties, P)
    eng.set_layout([P])
    eng.reserve(n, I64, parties)
    for k in range(n):
        eng.ingest(k, shares[k])
    sums = [torch.zeros(P, dtype=torch.int64, device="cuda") for _ in range(2)]
    decs = [torch.zeros(P, dtype=torch.float32, device="cuda") for _ in range(2)]
    _, st = measured(eng, eng.secagg_device, sums[0].data_ptr(), decs[0].data_ptr())
    check(st, [secagg_bytes(n * parties, P, True, True)], 0, "whole")
    for off, ln in ((0, cut), (cut, P - cut)):
        _, st = measured(eng, eng.secagg_device_range, off, ln, sums[1].data_ptr(), decs[1].data_ptr())
        check(st, [secagg_bytes(n * parties, ln, True, True)], 0, (off, ln))
    _, st = measured(eng, eng.secagg_device, sums[0].data_ptr(), 0)  # the sum alone
    check(st, [secagg_bytes(n * parties, P, True, True, want_dec=False)], 0, "sum only")
    torch.cuda.synchronize()
    assert torch.equal(sums[0], sums[1]) and torch.equal(decs[0].view(torch.int32), decs[1].view(torch.int32))
    assert np.array_equal(sums[0].cpu().numpy(), shares.sum(axis=(0, 1), dtype=np.int64))


STREAM_N, STREAM_R, STREAM_BATCH = 7, 4, 2
IN_ORDER = tuple(range(STREAM_N))
# clients 0 .. 2 fold as one run of three, so the run of clients 3 and 4 starts in the ring's last slot
# and wraps (two launches); clients 5 and 6 fold as they come and the finish finds an empty run
WRAPPING = (0, 2, 1, 3, 4, 5, 6)
WRAPPING_LAUNCHES = [LS.Launch(3, True, False), LS.Launch(1, False, False), LS.Launch(1, False, False),
                     LS.Launch(2, False, False), LS.Launch(0, False, True)]


def stream_calls(eng, kind, rows, order, finish):
    """Per call (every ingest, then the finish): its stats."""
    eng.stream_begin(kind, STREAM_BATCH)
    if kind == WEIGHTED:
        eng.set_weights(np.arange(1, STREAM_N + 1, dtype=F))
    calls = [measured(eng, eng.ingest, k, rows[k])[1] for k in order]
    return calls + [measured(eng, finish)[1]]


def check_stream(calls, want, bytes_of, rows_per_client=1):
    """The calls' launches, in order, are `want`; n_folded counts the clients folded so far."""
    left, folded = list(want), 0
    for i, st in enumerate(calls):
        mine, left = left[:st["kernel_launches"]], left[st["kernel_launches"]:]
        folded += sum(l.n_rows for l in mine) // rows_per_client
        check(st, [bytes_of(l) for l in mine], folded, i)
    assert not left
    assert folded == STREAM_N


@pytest.mark.parametrize("order,want", [(IN_ORDER, None), (WRAPPING, WRAPPING_LAUNCHES)], ids=["in-order", "wrapping"])
@pytest.mark.parametrize("mode", [MEAN, ITERATIVE, WEIGHTED], ids=RULE_IDS[:3])
def test_stream_ring(eng, mode, order, want):
    rows, ckpt = rows_of(STREAM_N, P), ckpt_of(P)
    eng.set_layout([P])
    eng.reserve(STREAM_R)
    calls = stream_calls(eng, mode, rows, order, lambda: eng.stream_finish(ckpt))
    want = want or LS.stream_launches(STREAM_N, STREAM_R, STREAM_BATCH)
    check_stream(calls, want, lambda l: fold_bytes(l.n_rows, P, l.first, l.final))


@pytest.mark.parametrize("order,want", [(IN_ORDER, None), (WRAPPING, WRAPPING_LAUNCHES)], ids=["in-order", "wrapping"])
def test_stream_ring_secagg(eng, order, want):
    parties = 3
    shares = shares_of(STREAM_N, parties, P)
    eng.set_layout([P])
    eng.reserve(STREAM_R, I64, parties)
    calls = stream_calls(eng, STREAM_SECAGG, shares, order, eng.stream_finish_secagg)
    want = want and [LS.Launch(l.n_rows * parties, l.first, l.final) for l in want]
    want = want or LS.stream_launches(STREAM_N, STREAM_R, STREAM_BATCH, rows_per_client=parties)
    check_stream(calls, want, lambda l: secagg_bytes(l.n_rows, P, l.first, l.final), parties)


def test_the_wrapping_order_is_what_it_says():
    """WRAPPING_LAUNCHES by the ring arithmetic of launch_shapes.stream_launches."""
    R, slot_client, folded, out = STREAM_R, {}, 0, []
    for k in WRAPPING:
        slot_client[k % R] = k
        run = 0
        while run < R and slot_client.get((folded + run) % R) == folded + run:
            run += 1
        if run >= STREAM_BATCH:
            done = 0
            while done < run:
                seg = min(run - done, R - (folded + done) % R)
                out.append(LS.Launch(seg, folded + done == 0, False))
                done += seg
            folded += run
    assert folded == STREAM_N and out + [LS.Launch(0, False, True)] == WRAPPING_LAUNCHES


@pytest.mark.parametrize("mode,b", [(MEAN, 0), (ITERATIVE, 0), (WEIGHTED, 0), (CLIPPED, 0), (TRIMMED, 2)],
                         ids=["mean", "iterative", "weighted", "clipped", "trimmed"])
def test_slot_folds_in_two_calls(eng, mode, b):
    """fold_slots writes the running state (and K8's planes), the finish reads it."""
    n = 6
    diffs, ckpt = rows_of(n, P), ckpt_of(P)
    load(eng, diffs, clip=CLIP_BOUND if mode == CLIPPED else 0.0, trim=b, weights=False)
    if mode == WEIGHTED:
        eng.set_weights(np.arange(1, n + 1, dtype=F))
    eng.ckpt_upload(ckpt)
    _, st = measured(eng, eng.fold_slots, mode, [3, 1])
    check(st, [launch_bytes(mode, b, 2, P, True, False)], 2, "early")
    _, st = measured(eng, eng.fold_slots_finish_resident, mode, [4, 0, 5, 2])
    check(st, [launch_bytes(mode, b, 4, P, False, True)], 6, "finish")
    if mode == CLIPPED:
        check_clip_stats(eng, diffs)


def test_slot_fold_of_more_rows_than_a_row_table(eng):
    n, p = LS.ROWTAB_MAX + 1, 67
    diffs, ckpt = rows_of(n, p), ckpt_of(p)
    load(eng, diffs, weights=False)
    eng.ckpt_upload(ckpt)
    _, st = measured(eng, eng.fold_slots_finish_resident, MEAN, list(range(n)))
    check(st, [fold_bytes(LS.ROWTAB_MAX, p, True, False), fold_bytes(1, p, False, True)], n, "mean")
    for k, d in enumerate(diffs):  # (a finish frees its slots)
        eng.ingest(k, d)
    _, st = measured(eng, eng.fold_slots_finish_resident, MEDIAN, list(range(n)))
    check(st, [launch_bytes(MEDIAN, 0, n, p, True, True)], n, "median")  # K9 over the device row table


@pytest.mark.parametrize("mode,b", [(MEAN, 0), (TRIMMED, 1)], ids=["mean", "trimmed"])
def test_ranged_final_pass(eng, mode, b):
    """A FINAL pass over more than 2^20 params runs as ranges of 2^20: their bytes sum to the one-launch
    formula, and each range of a trimmed FIRST | FINAL fold moves no state."""
    n, p, rf = 3, (1 << 20) + 259, 1 << 20
    diffs, ckpt = rows_of(n, p), ckpt_of(p)
    load(eng, diffs, trim=b, weights=False)
    eng.ckpt_upload(ckpt)
    _, st = measured(eng, eng.fold_slots_finish_resident, mode, [2, 0, 1])
    assert -(-p // rf) == 2
    check(st, [launch_bytes(mode, b, n, rf, True, True), launch_bytes(mode, b, n, p - rf, True, True)], n)
    assert st["kernel_bytes_total"] == fold_bytes(n, p, True, True)
