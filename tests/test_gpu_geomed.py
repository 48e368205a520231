"""GPU: geometric-median FedAvg (PGH_GEOMETRIC_MEDIAN, kernel K12), bit-exact against tests/geomed_oracle.py
and the golden file tests/golden/geomed_cases.npz -- K12's sums as u64, every close as u32 (NaNs by
position).  The definition is in include/pgh_api.h and DESIGN.md section 5."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import geomed_oracle as GO  # noqa: E402
import gen_geomed_golden as GG  # noqa: E402
import serveropt_oracle as SO  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
GEOMED, MEAN = 6, 0
UNSUPPORTED, STATE, ARG = -6, -3, -1
RC = 32  # DISTSQ_RC: the rows a K12 workgroup streams past its tile of the point
SHAPE_P = (1, 4095, 4096, 4097, 2 * 4096 + 2048 + 3)  # K7's tile edges and a ragged last tile
SHAPE_N = (1, 3, 4, 5, RC - 1, RC, RC + 1, 2 * RC + 3)  # row-group and row-chunk remainders
NU = 1e-6


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GG.GOLDEN)


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_geomed(0)
    engine.set_server_opt(SO.NONE)


def make_engine(**env):
    """A context of its own: PGH_BLOCK_BYTES and PGH_FINAL_RANGES are read when a context is made."""
    from pygrid_amd import Engine

    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return Engine(int(os.environ.get("PGH_DEVICE", "0")))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def load(eng, diffs, slots=None, cap=None):
    eng.set_layout([diffs.shape[1]])
    eng.reserve(cap or len(diffs))
    for k, d in enumerate(diffs):
        eng.ingest(k if slots is None else int(slots[k]), d)


@functools.lru_cache(maxsize=None)
def shape_rows(p, n=SHAPE_N[-1]):
    """n rows of p floats around a common centre, of mixed spread, and a checkpoint: every N takes a prefix."""
    rng = np.random.default_rng(12000 + p)
    centre = rng.standard_normal(p)
    rows = np.stack([(centre + rng.standard_normal(p) * 10.0 ** rng.integers(-2, 2)).astype(F) for _ in range(n)])
    return rows, rng.standard_normal(p).astype(F)


@functools.lru_cache(maxsize=None)
def shape_want(p, n, iters):
    rows, ckpt = shape_rows(p)
    return GO.fedavg_geomed(ckpt, rows[:n], iters, NU)


# ---- K12 alone ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", SHAPE_P)
def test_row_distsq_shapes(eng, p):
    rows, ckpt = shape_rows(p)
    load(eng, rows)
    points = {"random": ckpt, "zero": np.zeros(p, F), "row": rows[2].copy()}
    want = {k: u64([GO.row_distsq(r, pt) for r in rows]) for k, pt in points.items()}
    assert want["row"][2] == 0  # +0.0: the point is the row
    sumsq = eng.row_sumsq(list(range(len(rows))))
    assert np.array_equal(u64(sumsq), want["zero"])  # K12 against the zero point is K7, bit for bit
    for n in SHAPE_N:
        for k, pt in points.items():
            got = eng.row_distsq(list(range(n)), pt)
            assert np.array_equal(u64(got), want[k][:n]), (p, n, k)
    # a row table (scattered, repeated and out of order) gives each row the same bits
    slots = [5, 2, 66, 2, 40, 0, 33]
    assert np.array_equal(u64(eng.row_distsq(slots, ckpt)), want["random"][slots])
    assert np.array_equal(u64(eng.row_sumsq(list(range(len(rows))))), u64(sumsq))  # K7's cache is untouched


def test_row_distsq_golden_and_narrow_blocks(G):
    """PGH_BLOCK_BYTES=4096: blocks of 1,024 columns, so every tile straddles four of them."""
    diffs = G["fold_diffs"]
    p = 70001
    rng = np.random.default_rng(p)
    rows = (rng.standard_normal((5, p)) * 0.3 + rng.standard_normal(p)).astype(F)
    point, ckpt = rng.standard_normal(p).astype(F), rng.standard_normal(p).astype(F)
    with make_engine(PGH_BLOCK_BYTES="4096") as e:
        load(e, rows, [5, 2, 7, 0, 3], cap=8)
        assert e.slab()[1] == 1024 and e.slab()[2] > 0
        assert np.array_equal(u64(e.row_distsq([5, 2, 7, 0, 3], point)), u64([GO.row_distsq(r, point) for r in rows]))
        e.set_geomed(3, NU)
        e.ckpt_upload(ckpt)
        e.fold_slots_finish_resident(GEOMED, [5, 2, 7, 0, 3])
        assert np.array_equal(u32(e.ckpt_download()), u32(GO.fedavg_geomed(ckpt, rows, 3, NU)))
        # the golden case in the same context (a shard of one narrow block column set)
        load(e, diffs, [5, 2, 7, 0, 3], cap=8)
        assert np.array_equal(u64(e.row_distsq([5, 2, 7, 0, 3], diffs[1])), G["distsq_bits"])
        e.set_geomed(3, NU)
        e.ckpt_upload(G["fold_ckpt"])
        e.fold_slots_finish_resident(GEOMED, [5, 2, 7, 0, 3])
        assert np.array_equal(u32(e.ckpt_download()), G["fold_out_bits_3"])


def test_row_distsq_more_rows_than_a_row_table(eng):
    """513 scattered rows over 4,097 params: two RowTab launches; then the close over the same slots."""
    p, n = 4097, 513
    rng = np.random.default_rng(513)
    rows = (rng.standard_normal((n, p)) * 0.1 + rng.standard_normal(p)).astype(F)
    point, ckpt = rng.standard_normal(p).astype(F), rng.standard_normal(p).astype(F)
    slot_of = rng.permutation(n + 3)[:n]
    load(eng, rows, slot_of, cap=n + 3)
    got = eng.row_distsq(slot_of, point)
    assert np.array_equal(u64(got), u64([GO.row_distsq(r, point) for r in rows]))
    eng.set_geomed(2, NU)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(GEOMED, slot_of)
    assert GO.same_bits(eng.ckpt_download(), GO.fedavg_geomed(ckpt, rows, 2, NU))


# ---- the close ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", SHAPE_P)
def test_close_shapes(eng, p):
    rows, ckpt = shape_rows(p)
    for n in SHAPE_N:
        load(eng, rows[:n])
        for iters in (1, 2, 3):
            eng.set_geomed(iters, NU)
            got = eng.fedavg(GEOMED, ckpt)
            assert np.array_equal(u32(got), u32(shape_want(p, n, iters))), (p, n, iters)
            if n == 1:
                assert np.array_equal(u32(got), u32(ckpt - rows[0]))


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_every_entry_point_gives_the_same_bits(eng, iters):
    import torch

    p, n = SHAPE_P[-1], RC + 1
    rows, ckpt = shape_rows(p)
    want = shape_want(p, n, iters)
    load(eng, rows[:n])
    eng.set_geomed(iters, NU)
    assert eng.effective_variant(GEOMED) == eng.effective_variant(2)  # what the weighted fold would run
    assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want))
    assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want))  # idempotent: the close again, the same bits
    st = eng.geomed_stats()
    g = GO.geomed(rows[:n], iters, NU)
    assert st["iterations"] == iters and st["rows"] == n and st["excluded"] == 0
    assert u64([st["objective"]])[0] == u64([g["objective"]])[0] and u32([st["max_weight"]])[0] == u32([g["max_weight"]])[0]
    eng.ckpt_upload(ckpt)
    eng.fedavg_resident(GEOMED)
    assert np.array_equal(u32(eng.ckpt_download()), u32(want))
    eng.fedavg_resident(GEOMED)  # the new checkpoint is the next cycle's input
    assert np.array_equal(u32(eng.ckpt_download()), u32(GO.fedavg_geomed(want, rows[:n], iters, NU)))
    ck = torch.from_numpy(ckpt).cuda()
    out = torch.zeros_like(ck)
    cuts = (0, 4100, 8200, p)  # multiples of 4, not of a block or a tile
    for a, b in zip(cuts, cuts[1:]):
        eng.fedavg_device_range(GEOMED, a, b - a, ck.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(u32(out.cpu().numpy()), u32(want))
    # a permuted slot list: the rows where they landed, folded in the order given
    rng = np.random.default_rng(iters)
    slot_of = rng.permutation(n + 5)[:n]
    order = rng.permutation(n)
    load(eng, rows[:n], slot_of, cap=n + 5)
    eng.set_geomed(iters, NU)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(GEOMED, slot_of[order])
    assert np.array_equal(u32(eng.ckpt_download()), u32(GO.fedavg_geomed(ckpt, rows[:n][order], iters, NU)))
    eng.ckpt_upload(ckpt)  # the finish freed its slots
    for k in range(n):
        eng.ingest(int(slot_of[k]), rows[k])
    eng.fold_slots_finish_resident(GEOMED, slot_of[:n])
    assert np.array_equal(u32(eng.ckpt_download()), u32(want))


def test_final_ranges_and_a_large_shard():
    """PGH_FINAL_RANGES=4 (shards of >= 1 M params): the FINAL fold as four ranges on two streams; the slot
    finish of such a shard runs its FINAL in 4 MiB ranges too."""
    p, n, iters = (1 << 20) + 4099, 3, 2
    rng = np.random.default_rng(20)
    rows = (rng.standard_normal((n, p)) * 0.1 + 1).astype(F)
    ckpt = rng.standard_normal(p).astype(F)
    want = GO.fedavg_geomed(ckpt, rows, iters, NU)
    with make_engine(PGH_FINAL_RANGES="4") as e:
        load(e, rows)
        e.set_geomed(iters, NU)
        e.ckpt_upload(ckpt)
        e.fedavg_resident(GEOMED)
        assert np.array_equal(u32(e.ckpt_download()), u32(want))
        assert np.array_equal(u32(e.fedavg(GEOMED, ckpt)), u32(want))
        e.ckpt_upload(ckpt)
        e.fold_slots_finish_resident(GEOMED, [0, 1, 2])
        assert np.array_equal(u32(e.ckpt_download()), u32(want))


def test_server_optimizer_takes_the_geometric_median(eng):
    p, n, iters = 4097, 5, 3
    rows, ckpt = shape_rows(p)
    hp = {"lr": 0.3, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
    g = GO.geomed(rows[:n], iters, NU)["v"]
    m0, v0 = SO.init_state(p, hp["tau"])
    want, _, _ = SO.step(SO.ADAM, ckpt, g, m0, v0, **hp)
    load(eng, rows[:n])
    eng.set_geomed(iters, NU)
    eng.set_server_opt(SO.ADAM, hp["lr"], hp["beta1"], hp["beta2"], hp["tau"])
    assert SO.same_bits(eng.fedavg(GEOMED, ckpt), want)
    assert SO.same_bits(eng.fedavg(GEOMED, ckpt), want)  # nothing committed: the same step again


def test_hostile_rows(eng, G):
    ckpt, diffs = G["hostile_ckpt"], G["hostile_diffs"]
    load(eng, diffs)
    eng.set_geomed(3, NU)
    got = eng.fedavg(GEOMED, ckpt)
    assert np.isfinite(got).all() and np.array_equal(u32(got), G["hostile_out_bits"])
    st = eng.geomed_stats()
    assert st["rows"] == 10 and st["excluded"] == 2
    assert not np.isfinite(eng.fedavg(MEAN, ckpt)).all()  # the plain mean of the same slab is lost
    # a clean diff into an excluded slot brings the row back
    clean = diffs[0][::-1].copy()
    eng.ingest(6, clean)
    rows = diffs.copy()
    rows[6] = clean
    got = eng.fedavg(GEOMED, ckpt)
    assert np.array_equal(u32(got), u32(GO.fedavg_geomed(ckpt, rows, 3, NU)))
    assert eng.geomed_stats()["excluded"] == 1


def test_refusals_leave_the_context_usable(eng, G):
    from pygrid_amd import Engine
    from pygrid_amd.exceptions import AggregationError

    ckpt, diffs = G["fold_ckpt"], G["fold_diffs"]
    p, n = diffs.shape[1], len(diffs)

    def refused(status, fn, *a):
        with pytest.raises(AggregationError) as e:
            fn(*a)
        assert e.value.status == status, e.value

    def still_right():
        load(eng, diffs)
        eng.set_geomed(3, NU)
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), G["fold_out_bits_3"])
        assert np.array_equal(u32(eng.fedavg(MEAN, ckpt)), u32(O.fedavg_mean([ckpt], [[d] for d in diffs])[0]))

    load(eng, diffs)
    refused(STATE, eng.fedavg, GEOMED, ckpt)  # the mode without the setting
    for bad in ((-1, NU), (17, NU), (3, 0.0), (3, -1.0), (3, float("nan")), (3, float("inf"))):
        refused(ARG, eng.set_geomed, *bad)
    still_right()
    eng.ckpt_upload(ckpt)
    refused(UNSUPPORTED, eng.fold_slots, GEOMED, [0, 1])  # nothing can be folded early
    eng.fold_slots_finish_resident(GEOMED, list(range(n)))  # ... and nothing was
    assert np.array_equal(u32(eng.ckpt_download()), G["fold_out_bits_3"])
    still_right()
    refused(UNSUPPORTED, eng.stream_begin, GEOMED)
    still_right()
    load(eng, diffs)
    eng.set_geomed(3, NU)
    eng.ckpt_upload(ckpt)
    eng.fold_slots(MEAN, [0, 1])  # a running fold state: the cycle cannot close with every row any more
    refused(STATE, eng.fold_slots_finish_resident, GEOMED, list(range(2, n)))
    eng.fold_slots_finish_resident(MEAN, list(range(2, n)))
    still_right()
    # the setting beside DP noise: no un-noised average leaves the context
    load(eng, diffs)
    eng.set_geomed(3, NU)
    eng.set_clip_norm(1.0)
    eng.set_dp_noise(1.0, 7, 1)
    try:
        refused(STATE, eng.fedavg, GEOMED, ckpt)
    finally:
        eng.set_dp_noise(0.0)
        eng.set_clip_norm(0.0)
    still_right()
    # every row non-finite: nothing to take a median of
    bad = diffs.copy()
    bad[:, 3] = np.nan
    load(eng, bad)
    eng.set_geomed(3, NU)
    refused(STATE, eng.fedavg, GEOMED, ckpt)
    eng.ckpt_upload(ckpt)
    refused(STATE, eng.fold_slots_finish_resident, GEOMED, list(range(n)))
    still_right()
    # a sub-range shard and a group: the distances need whole rows
    try:
        eng.set_layout([p])
        eng.set_shard(1000, p)
        eng.reserve(n)
        refused(UNSUPPORTED, eng.set_geomed, 3, NU)
        refused(UNSUPPORTED, eng.fedavg, GEOMED, ckpt[1000:])
    finally:
        eng.set_layout([p])
    still_right()
    assert eng.geomed_stats()["iterations"] == 3
    eng.set_layout([p])  # a new layout clears the setting; reset and reserve keep it
    assert eng.geomed_stats()["iterations"] == 0
    eng.set_geomed(2, NU)
    eng.reserve(n)
    eng.reset()
    assert eng.geomed_stats()["iterations"] == 2
    with Engine(devices=[0, 0]) as grp:
        grp.set_layout([p])
        grp.reserve(n)
        refused(UNSUPPORTED, grp.set_geomed, 3, NU)
        for k, d in enumerate(diffs):
            grp.ingest(k, d)
        refused(UNSUPPORTED, grp.fedavg, GEOMED, ckpt)
        assert np.array_equal(u32(grp.fedavg(MEAN, ckpt)), u32(O.fedavg_mean([ckpt], [[d] for d in diffs])[0]))


# ---- through the host layer -----------------------------------------------------------------------------------------

SHAPES = [(40, 100), (100,), (7, 3), (1,)]


def model_case(n, hostile=(1, 4)):
    rng = np.random.default_rng(4122)
    ckpt = [rng.standard_normal(s).astype(F) for s in SHAPES]
    diffs = [[(rng.standard_normal(s) * 1e-2 + 0.5).astype(F) for s in SHAPES] for _ in range(n)]
    diffs[hostile[0]][0][0, :3] = (np.nan, np.inf, -np.inf)  # excluded
    diffs[hostile[1]][1][:] = F(1e30)                        # kept, with next to no weight
    return ckpt, diffs


def flat(ts):
    return np.concatenate([np.asarray(t, F).reshape(-1) for t in ts])


def test_cycle_aggregator_and_incremental_cycle(eng):
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.exceptions import GeometricMedianUnavailableError
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.settings import settings_of
    from pygrid_amd.state_schema import build_state_fast, parse_state

    ckpt, diffs = model_case(7)
    cfg = {"diff_geometric_median": {"iterations": 2}}
    g = GO.geomed([flat(d) for d in diffs], 2, NU)
    want = (flat(ckpt) - g["v"]).astype(F)
    assert np.isfinite(want).all() and g["excluded"] == 1
    agg = CycleAggregator(eng)
    pbs = [build_state_fast(d) for d in diffs]
    ck_pb = build_state_fast(ckpt)
    new = agg.average_plan_diffs(cfg, ck_pb, pbs)
    assert np.array_equal(u32(flat(parse_state(new))), u32(want))
    assert np.array_equal(u32(flat(agg.average_params(cfg, ckpt, diffs))), u32(want))
    with pytest.raises(GeometricMedianUnavailableError):
        agg.average_plan_diffs(dict(cfg, diff_trim_count=1), ck_pb, pbs)
    new2 = agg.average_plan_diffs({}, new, pbs[2:4])  # the next cycle without the key: the plain mean
    for got, w in zip(parse_state(new2), O.fedavg_mean(parse_state(new), diffs[2:4])):
        assert np.array_equal(u32(got), u32(w))
    assert eng.geomed_stats()["iterations"] == 0
    # report time: out of order, one worker never reports; everything at the close, in assignment order
    inc = IncrementalCycle(eng, [int(np.prod(s)) for s in SHAPES], slots=8, fold_batch=2, checkpoint=ck_pb,
                           settings=settings_of(cfg))
    for w in range(8):
        inc.assigned(w)
    for w in (3, 0, 6, 1, 5, 4, 2):  # worker 7 never reports
        inc.reported(w, pbs[w])
    new3 = inc.close(ck_pb)
    assert np.array_equal(u32(flat(parse_state(new3))), u32(want))
    lc, st = inc.last_close, eng.geomed_stats()
    assert lc["n"] == 7 and lc["early"] == 0
    assert lc["geometric_median"] == {"iterations": 2, "excluded": 1, "objective": st["objective"],
                                      "max_weight": st["max_weight"]}
    assert u64([st["objective"]])[0] == u64([g["objective"]])[0]
    # an engine that cannot apply the rule -- a group -- fails closed instead of falling back
    from pygrid_amd import Engine

    with Engine(devices=[0]) as grp:
        with pytest.raises(GeometricMedianUnavailableError):
            CycleAggregator(grp).average_plan_diffs(cfg, ck_pb, pbs)
