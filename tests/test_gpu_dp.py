"""GPU: Gaussian noise on the clipped close (pgh_set_dp_noise, kernel K11), bit-exact against
tests/clip_oracle.py composed with the noise of tests/dp_oracle.py (u32 compares, NaNs by bits): the
sampler alone, the noised close through every entry point and range split, repetition, the key and the
round, z = 0, a server optimizer behind it, the refusals and the Python layer.  The definition is in
include/pgh_api.h and DESIGN.md section 5."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import clip_oracle as CO  # noqa: E402
import dp_oracle as DO  # noqa: E402
import serveropt_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MEAN, CLIPPED, TRIMMED, MEDIAN = 0, 3, 4, 5
ARG, STATE, UNSUPPORTED = -1, -3, -6
KEY, ROUND, Z, N = 0xDEADBEEF0BADF00D, 0xFFFFFFFE, 1.1, 3
CLOSE_P = (1, 2, 7, 1025, 4099, 70001)  # one column, a ragged tail of every length, more than one workgroup


def device():
    return int(os.environ.get("PGH_DEVICE", "0"))


@pytest.fixture(scope="module")
def eng():
    from pygrid_amd import Engine

    with Engine(device()) as e:
        yield e


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = u32(a).reshape(-1), u32(b).reshape(-1)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def bound(p):
    return float(F(1e-2 * np.sqrt(p)))  # the first two rows' norm is about this; the third row is 30 x larger


@functools.lru_cache(maxsize=None)
def case(p, n=N):
    """n diffs (the last one clipped for certain), a checkpoint, the clipped average g, the un-noised close
    and the noised one -- computed once per shape and shared."""
    rng = np.random.default_rng(7000 + p)
    d = (rng.standard_normal((n, p)) * 1e-2).astype(F)
    d[n - 1] *= F(30.0)
    ckpt = (rng.standard_normal(p) * 0.1).astype(F)
    rows = [d[k] for k in range(n)]
    c = bound(p)
    assert CO.scales(rows, c)[n - 1] < 1
    g = SO.avg_from(lambda ck: CO.fedavg_clipped(ck, rows, c), p)
    for a in (d, ckpt, g):
        a.setflags(write=False)
    return d, ckpt, g, CO.fedavg_clipped(ckpt, rows, c), DO.close(ckpt, g, KEY, ROUND, Z, c, n)


def prepare(e, p, n=N, z=Z, key=KEY, rnd=ROUND):
    e.set_layout([p])
    e.reserve(n)
    e.set_clip_norm(bound(p))
    e.set_dp_noise(z, key, rnd)


def ingest(e, rows):
    e.reset()
    for k, d in enumerate(rows):
        e.ingest(k, d)


def status_of(fn, *a):
    from pygrid_amd import AggregationError

    with pytest.raises(AggregationError) as ei:
        fn(*a)
    return ei.value.status


# ---- the sampler alone -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("i0", [0, 12345, (1 << 33) + 1], ids=["zero", "odd", "above-2^33"])
def test_dp_normals_are_the_oracle(eng, i0):
    want = DO.normals(KEY, ROUND, i0, 70001)
    for n in (1, 2, 7, 4099, 70001):
        got = eng.dp_normals(KEY, ROUND, i0, n)
        assert np.array_equal(DO.bits64(got), DO.bits64(want[:n])), (i0, n)
    assert eng.dp_normals(KEY, ROUND, i0, 0).size == 0
    assert np.array_equal(DO.bits64(eng.dp_normals(KEY, ROUND, i0, 4099)), DO.bits64(eng.dp_normals_host(KEY, ROUND, i0, 4099)))


# ---- the noised close --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", CLOSE_P)
def test_noised_close_over_pgh_fedavg(eng, p):
    d, ckpt, g, plain, want = case(p)
    prepare(eng, p)
    ingest(eng, d)
    got = eng.fedavg(CLIPPED, ckpt)
    assert same(got, want), p
    assert not same(got, plain)
    st = eng.dp_stats()
    assert st["multiplier"] == F(Z) and st["n"] == N and st["sigma"] == DO.sigma_of(Z, bound(p), N)
    # the same FINAL again: the same noise, bit for bit -- never a second draw
    assert same(eng.fedavg(CLIPPED, ckpt), want), p
    eng.set_dp_noise(0.0)


def test_round_and_key_reach_the_noise(eng):
    p = 4099
    d, ckpt, g, plain, want = case(p)
    c = bound(p)
    for key, rnd in ((KEY, ROUND + 1), (KEY ^ (1 << 40), ROUND), (KEY ^ 1, ROUND)):
        prepare(eng, p, key=key, rnd=rnd)
        ingest(eng, d)
        got = eng.fedavg(CLIPPED, ckpt)
        assert same(got, DO.close(ckpt, g, key, rnd, Z, c, N)), (key, rnd)
        assert not same(got, want), (key, rnd)
    eng.set_dp_noise(0.0)


def test_z_zero_is_todays_clipped_close(eng):
    for p in (7, 4099):
        d, ckpt, g, plain, want = case(p)
        prepare(eng, p, z=0.0)
        ingest(eng, d)
        assert same(eng.fedavg(CLIPPED, ckpt), plain), p
        eng.set_dp_noise(Z, KEY, ROUND)  # on, and off again before the close
        eng.set_dp_noise(0.0)
        assert same(eng.fedavg(CLIPPED, ckpt), plain), p
        assert eng.dp_stats()["multiplier"] == 0.0


def test_device_range_splits_equal_the_one_launch_result(eng):
    import torch

    p = 4099
    d, ckpt, g, plain, want = case(p)
    prepare(eng, p)
    ingest(eng, d)
    ck = torch.from_numpy(np.array(ckpt)).cuda()
    out = torch.full((p,), 77.0, dtype=torch.float32, device="cuda")
    eng.fedavg_device(CLIPPED, ck.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert same(out.cpu().numpy(), want)
    # starts are multiples of 4; lengths odd, even and no multiple of 4, and the shard's ragged end
    for ranges in (((0, 1025), (1028, 1030), (2060, p - 2060)), ((0, 1), (4, 2), (8, 3), (12, 7), (2048, 2051)),
                   ((4, p - 4),)):
        out.fill_(77.0)
        sel = np.zeros(p, bool)
        for off, ln in ranges:
            eng.fedavg_device_range(CLIPPED, off, ln, ck.data_ptr(), out.data_ptr())
            sel[off:off + ln] = True
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert same(got[sel], want[sel]), ranges
        assert np.all(got[~sel] == F(77.0)), ranges  # nothing outside the ranges is written
    eng.set_dp_noise(0.0)


@pytest.mark.parametrize("p", [7, 70001])
def test_resident_and_slot_closes(eng, p):
    d, ckpt, g, plain, want = case(p)
    prepare(eng, p)
    ingest(eng, d)
    eng.ckpt_upload(ckpt)
    eng.fedavg_resident(CLIPPED)
    assert same(eng.ckpt_download(), want), p
    # early slot folds run un-noised; K11 follows the finish's FINAL pass alone
    ingest(eng, d)
    eng.ckpt_upload(ckpt)
    eng.fold_slots(CLIPPED, [0])
    eng.fold_slots(CLIPPED, [1])
    eng.fold_slots_finish_resident(CLIPPED, [2])
    assert same(eng.ckpt_download(), want), p
    # every row folded early: the finish is a FINAL over no rows
    ingest(eng, d)
    eng.ckpt_upload(ckpt)
    eng.fold_slots(CLIPPED, [0, 1, 2])
    eng.fold_slots_finish_resident(CLIPPED, [])
    assert same(eng.ckpt_download(), want), p
    assert eng.dp_stats()["n"] == N
    eng.set_dp_noise(0.0)


def test_large_model_slot_close_in_final_ranges(eng):
    """2^20 + 7 params: pgh_fold_slots_finish_resident runs its FINAL pass in 4 MiB ranges, K11 behind each."""
    p = (1 << 20) + 7
    d, ckpt, g, plain, want = case(p)
    prepare(eng, p)
    ingest(eng, d)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(CLIPPED, [0, 1, 2])
    assert same(eng.ckpt_download(), want)
    eng.set_dp_noise(0.0)


# ---- a server optimizer behind the noise -------------------------------------------------------------------------

@pytest.mark.parametrize("p", [7, 4099])
def test_fedadam_takes_the_noised_average(eng, p):
    hp = {"lr": 0.3, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
    d, ckpt, g, plain, want = case(p)
    gn = DO.noised_avg(g, KEY, ROUND, Z, bound(p), N)
    m0, v0 = SO.init_state(p, hp["tau"])
    wout, wm, wv = SO.step(SO.ADAM, ckpt, gn, m0, v0, **hp)
    prepare(eng, p)
    eng.set_server_opt(SO.ADAM, hp["lr"], hp["beta1"], hp["beta2"], hp["tau"])
    ingest(eng, d)
    assert same(eng.fedavg(CLIPPED, ckpt), wout), p
    assert same(eng.fedavg(CLIPPED, ckpt), wout), p  # a repeated FINAL: the same noise into the same step
    eng.server_opt_commit()
    gm, gv = eng.server_opt_state()
    assert same(gm, wm) and same(gv, wv), p
    # the next cycle steps from the committed moments, with another round's noise
    eng.set_dp_noise(Z, KEY, 5)
    gn2 = DO.noised_avg(g, KEY, 5, Z, bound(p), N)
    wout2, wm2, wv2 = SO.step(SO.ADAM, wout, gn2, wm, wv, **hp)
    assert same(eng.fedavg(CLIPPED, wout), wout2), p
    eng.server_opt_commit()
    gm, gv = eng.server_opt_state()
    assert same(gm, wm2) and same(gv, wv2), p
    eng.set_server_opt(SO.NONE)
    eng.set_dp_noise(0.0)


# ---- refusals and lifetime -----------------------------------------------------------------------------------------

def test_other_modes_are_refused_while_noise_is_on(eng):
    import torch

    p = 1025
    d, ckpt, g, plain, want = case(p)
    prepare(eng, p)
    eng.set_trim(1)
    ingest(eng, d)
    eng.ckpt_upload(ckpt)
    launches = eng.stats()["kernel_launches"]
    ck = torch.from_numpy(np.array(ckpt)).cuda()
    out = torch.full((p,), 77.0, dtype=torch.float32, device="cuda")
    for mode in (MEAN, TRIMMED, MEDIAN):
        assert status_of(eng.fedavg, mode, ckpt) == STATE, mode
        assert status_of(eng.fedavg_resident, mode) == STATE, mode
        assert status_of(eng.fold_slots_finish_resident, mode, [0, 1, 2]) == STATE, mode
        assert status_of(eng.fedavg_device_range, mode, 0, p, ck.data_ptr(), out.data_ptr()) == STATE, mode
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == F(77.0))
    assert eng.stats()["kernel_launches"] == launches  # nothing was launched
    assert same(eng.ckpt_download(), ckpt)             # and the resident checkpoint is as it was
    assert same(eng.fedavg(CLIPPED, ckpt), want)        # the context stays usable
    eng.set_dp_noise(0.0)
    from oracle import oracle as O

    assert same(eng.fedavg(MEAN, ckpt), O.fedavg_mean([np.array(ckpt)], [[r] for r in d])[0])  # works again after z = 0
    eng.set_trim(0)


def test_setter_arguments_and_lifetime(eng):
    p = 64
    prepare(eng, p, z=0.0)
    for bad in (-1.0, float("nan"), float("inf")):
        assert status_of(eng.set_dp_noise, bad, KEY, ROUND) == ARG, bad
    eng.set_dp_noise(Z, KEY, ROUND)
    eng.reset()
    assert eng.dp_stats()["multiplier"] == F(Z)   # pgh_reset keeps it
    eng.reserve(5)
    assert eng.dp_stats()["multiplier"] == F(Z)   # pgh_reserve keeps it
    eng.set_shard(0, p)
    assert eng.dp_stats()["multiplier"] == 0.0    # pgh_set_shard clears it
    eng.set_dp_noise(Z, KEY, ROUND)
    eng.set_layout([p])
    assert eng.dp_stats()["multiplier"] == 0.0    # pgh_set_layout clears it
    # a shard narrower than the layout refuses z > 0 like pgh_set_clip_norm, and takes z = 0
    eng.set_shard(0, p // 2)
    assert status_of(eng.set_dp_noise, Z, KEY, ROUND) == UNSUPPORTED
    eng.set_dp_noise(0.0)
    eng.set_layout([p])
    # an int64 slab
    eng.reserve(2, 1, 2)
    assert status_of(eng.set_dp_noise, Z, KEY, ROUND) == UNSUPPORTED
    eng.set_dp_noise(0.0)
    eng.set_layout([p])


def test_a_group_refuses_the_noise():
    from pygrid_amd import Engine

    with Engine(devices=[device()]) as grp:
        grp.set_layout([64])
        grp.reserve(2)
        assert status_of(grp.set_dp_noise, Z, KEY, ROUND) == UNSUPPORTED
        grp.set_dp_noise(0.0)


# ---- the Python layer at MNIST size ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def mnist_case():
    from oracle.gen_golden import MNIST_SHAPES, mnist_inputs, split

    diffs, ckpt = mnist_inputs(4321, 4)
    diffs = [np.asarray(x, F) for x in diffs]
    diffs[2] = (diffs[2] * F(50.0)).astype(F)
    c = float(F(0.5 * np.sqrt(CO.row_sumsq(diffs[0]))))  # below every row's norm: all four are clipped
    g = SO.avg_from(lambda ck: CO.fedavg_clipped(ck, diffs, c), ckpt.size)
    return MNIST_SHAPES, split, diffs, np.asarray(ckpt, F), c, g


def test_drop_in_close_at_mnist_size(eng):
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.state_schema import build_state_fast, parse_state

    shapes, split, diffs, ckpt, c, g = mnist_case()
    cfg = {"diff_clip_norm": c, "dp_noise": {"multiplier": Z, "key": KEY}}
    agg = CycleAggregator(eng)
    new = agg.average_plan_diffs(cfg, build_state_fast(split(ckpt, shapes)), [build_state_fast(split(x, shapes)) for x in diffs],
                                 dp_round=(1 << 32) + 9)
    got = np.concatenate([np.asarray(t, F).reshape(-1) for t in parse_state(new)])
    assert same(got, DO.close(ckpt, g, KEY, 9, Z, c, len(diffs)))
    eng.set_dp_noise(0.0)


def test_incremental_close_at_mnist_size(eng):
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.state_schema import build_state_fast, parse_state

    shapes, split, diffs, ckpt, c, g = mnist_case()
    ck_pb = build_state_fast(split(ckpt, shapes))
    inc = IncrementalCycle(eng, [int(np.prod(s)) for s in shapes], slots=6, fold_batch=1, checkpoint=ck_pb, clip_norm=c,
                           dp_noise={"multiplier": Z, "key": KEY}, dp_round=31)
    for w in range(5):
        inc.assigned(w)
    for w in (1, 0, 3, 2):  # worker 4 never reports
        inc.reported(w, build_state_fast(split(diffs[w], shapes)))
    new = inc.close(ck_pb)
    got = np.concatenate([np.asarray(t, F).reshape(-1) for t in parse_state(new)])
    assert same(got, DO.close(ckpt, g, KEY, 31, Z, c, 4))
    assert inc.last_close["early"] > 0 and inc.last_close["clipped"] == 4
    assert inc.last_close["noise_multiplier"] == float(F(Z)) and inc.last_close["noise_std"] == DO.sigma_of(Z, c, 4)
    eng.set_dp_noise(0.0)
    eng.set_clip_norm(0.0)
