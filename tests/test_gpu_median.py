"""GPU: coordinate-wise median (PGH_MEDIAN, kernels K9 and K9p), bit-exact against
tests/median_oracle.py and the golden file tests/golden/median_cases.npz (NaNs by position), on the
auto path (K9 up to PGH_MEDIAN_NCHIP rows) and with PGH_MEDIAN_PATH=passes (K9p), a context each.
The definition is in DESIGN.md section 5 and include/pgh_api.h."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_median_golden as GG  # noqa: E402
import median_oracle as MO  # noqa: E402
import trim_oracle as TO  # noqa: E402
from gen_trim_golden import special_rows  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MEAN, TRIMMED, MEDIAN = 0, 4, 5
STATE, UNSUPPORTED = -3, -6
N_CHIP = 1024
PATHS = ("auto", "passes")
SHAPE_P = (1, 3, 5, 4097, 2 * 65536 + 5)  # below a tile, ragged last tiles, thousands of workgroups
SHAPE_N = (1, 2, 3, 4, 5, 8, 9, 37)
# K9's tiers end at 8, 16, 32 and 64 rows (one lane holds the column) and at 128, 256, 512 and 1,024
# (2, 4, 8 and 16 waves share it): each tier's last row count, the ones beside it, N_chip
TIER_N = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
TIER_P = 257  # four tiles and one column


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GG.GOLDEN)


def make_engine(path, **env):
    """A context of its own: PGH_MEDIAN_PATH (and PGH_BLOCK_BYTES) are read when a context is made."""
    from pygrid_amd import Engine

    env = dict(env, PGH_MEDIAN_PATH="passes" if path == "passes" else None)
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        return Engine(int(os.environ.get("PGH_DEVICE", "0")))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.fixture(scope="module")
def engines():
    made = {path: make_engine(path) for path in PATHS}
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(params=PATHS)
def eng(request, engines):
    e = engines[request.param]
    e.path = request.param
    return e


def variant_for(eng, n):
    return 51 if eng.path == "passes" or n > N_CHIP else 50


@functools.lru_cache(maxsize=None)
def shape_rows(p):
    """37 rows of p floats (specials in the first three) and a checkpoint: every N takes a prefix."""
    return special_rows(37, p, 5000 + p), np.random.default_rng(p).standard_normal(p).astype(F)


@functools.lru_cache(maxsize=None)
def shape_want(p, n):
    rows, ckpt = shape_rows(p)
    return MO.fedavg_median(ckpt, rows[:n])


@functools.lru_cache(maxsize=None)
def tall_rows(p, n=N_CHIP + 1):
    """n rows of p floats, a special value in every fifth place of every row."""
    return special_rows(n, p, 6000 + p, every=5, rows=n), np.random.default_rng(p).standard_normal(p).astype(F)


@functools.lru_cache(maxsize=None)
def tall_want(p, n):
    rows, ckpt = tall_rows(p)
    return MO.fedavg_median(ckpt, rows[:n])


def load(eng, diffs, slots=None, cap=None):
    eng.set_layout([diffs.shape[1]])
    eng.reserve(cap or len(diffs))
    for k, d in enumerate(diffs):
        eng.ingest(k if slots is None else int(slots[k]), d)


def test_shapes(eng):
    for p in SHAPE_P:
        rows, ckpt = shape_rows(p)
        eng.set_layout([p])
        eng.reserve(37)
        have = 0
        for n in SHAPE_N:
            for k in range(have, n):
                eng.ingest(k, rows[k])
            have = n
            assert eng.effective_variant(MEDIAN) == variant_for(eng, n)
            got = eng.fedavg(MEDIAN, ckpt)
            assert MO.same_bits(got, shape_want(p, n)), (p, n)


def test_tier_boundaries_and_the_path_table(eng):
    rows, ckpt = tall_rows(TIER_P)
    eng.set_layout([TIER_P])
    eng.reserve(N_CHIP)
    have = 0
    for n in TIER_N:
        for k in range(have, n):
            eng.ingest(k, rows[k])
        have = n
        got = eng.fedavg(MEDIAN, ckpt)
        assert MO.same_bits(got, tall_want(TIER_P, n)), n
    assert eng.effective_variant(MEDIAN) == variant_for(eng, N_CHIP)
    eng.set_variant(13)  # the table of pgh_set_variant does not reach median folds
    assert eng.effective_variant(MEDIAN) == variant_for(eng, N_CHIP)
    assert MO.same_bits(eng.fedavg(MEDIAN, ckpt), tall_want(TIER_P, N_CHIP))
    eng.set_variant(-1)


def test_path_switch_past_n_chip(eng):
    """N_chip + 1 rows x 67 params: the auto path takes K9p by itself."""
    p, n = 67, N_CHIP + 1
    rows, ckpt = tall_rows(p)
    load(eng, rows[:N_CHIP], cap=n)
    assert eng.effective_variant(MEDIAN) == variant_for(eng, N_CHIP)
    eng.ingest(N_CHIP, rows[N_CHIP])
    assert eng.effective_variant(MEDIAN) == 51
    assert MO.same_bits(eng.fedavg(MEDIAN, ckpt), tall_want(p, n))


@pytest.mark.parametrize("n", [9, 12])
def test_accounted_bytes(eng, n):
    """K9 reads the slab once: 4 N P + 8 P.  K9p: a pass per bit (and one for an even N), each the
    rows plus the prefix plane read (not by the first) and written (the last: ckpt in, out)."""
    p = 4097
    rows, ckpt = shape_rows(p)
    load(eng, rows[:n])
    eng.reset_stats()
    assert MO.same_bits(eng.fedavg(MEDIAN, ckpt), shape_want(p, n))
    st = eng.stats()
    if variant_for(eng, n) == 50:
        assert st["kernel_launches"] == 1 and st["kernel_bytes_last"] == st["kernel_bytes_total"] == 4 * n * p + 8 * p
    else:
        passes = 32 + (n % 2 == 0)
        assert st["kernel_launches"] == passes
        assert st["kernel_bytes_total"] == passes * 4 * n * p + 2 * (passes - 1) * 4 * p + 8 * p
        assert st["kernel_bytes_last"] == 4 * n * p + 4 * p + 8 * p


def test_specials_match_the_golden_file(eng, G):
    """+-0 and subnormal middles, ties, 3e38 twice, -inf and +inf, NaN minorities and majorities."""
    for n in GG.CASES:
        ckpt, diffs = G[f"ckpt_{n}"], G[f"diffs_{n}"]
        want = MO.fedavg_median(ckpt, diffs)
        assert MO.same_bits(want, G[f"out_{n}"])
        load(eng, diffs)
        got = eng.fedavg(MEDIAN, ckpt)
        assert MO.same_bits(got, want), n
        assert np.isfinite(got[8:10]).all() and np.isfinite(got[12:15]).all() and np.isnan(got[15:17]).all()
        assert got[5] == ckpt[5] - F(0.25)  # the all-equal column


@pytest.mark.parametrize("path", PATHS)
def test_narrow_blocks(path):
    """PGH_BLOCK_BYTES=4096: blocks of 1,024 columns, in a context of its own."""
    p, n = SHAPE_P[-1], 37
    rows, ckpt = shape_rows(p)
    with make_engine(path, PGH_BLOCK_BYTES="4096") as e:
        load(e, rows[:n])
        assert e.slab()[1] == 1024 and e.slab()[2] > 0
        assert e.effective_variant(MEDIAN) == (51 if path == "passes" else 50)
        assert MO.same_bits(e.fedavg(MEDIAN, ckpt), shape_want(p, n))


def test_ranges_and_chained_resident_cycles(eng):
    import torch

    p, n = 8197, 12
    diffs = special_rows(n, p, 8197)
    ckpt = np.random.default_rng(8197).standard_normal(p).astype(F)
    want = MO.fedavg_median(ckpt, diffs)
    load(eng, diffs)
    ck = torch.from_numpy(ckpt).cuda()
    out = torch.zeros_like(ck)
    cut = 4100  # a multiple of 4, not of a block
    eng.fedavg_device_range(MEDIAN, 0, cut, ck.data_ptr(), out.data_ptr())
    eng.fedavg_device_range(MEDIAN, cut, p - cut, ck.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert MO.same_bits(out.cpu().numpy(), want)
    eng.ckpt_upload(ckpt)
    eng.fedavg_resident(MEDIAN)
    assert MO.same_bits(eng.ckpt_download(), want)
    eng.fedavg_resident(MEDIAN)  # the new checkpoint is the next cycle's input
    assert MO.same_bits(eng.ckpt_download(), MO.fedavg_median(want, diffs))


def test_group_and_shard_match_one_context(engine):
    from pygrid_amd import Engine

    p, n = 70001, 9
    diffs = special_rows(n, p, 70001)
    ckpt = np.random.default_rng(7).standard_normal(p).astype(F)
    want = MO.fedavg_median(ckpt, diffs)
    try:
        load(engine, diffs)
        one = engine.fedavg(MEDIAN, ckpt)
        assert MO.same_bits(one, want)
        lo, hi = 35000, p  # a shard: nothing in the median looks along a row
        engine.set_layout([p])
        engine.set_shard(lo, hi)
        engine.reserve(n)
        for k, d in enumerate(diffs):
            engine.ingest(k, d[lo:hi])
        assert np.array_equal(u32(engine.fedavg(MEDIAN, ckpt[lo:hi])), u32(one[lo:hi]))
    finally:
        engine.set_layout([p])
    with Engine(devices=[0, 0]) as grp:
        grp.set_layout([p])
        grp.reserve(n + 2)
        for k, d in enumerate(diffs):
            grp.ingest(k, d)
        assert grp.effective_variant(MEDIAN) == 50
        assert np.array_equal(u32(grp.fedavg(MEDIAN, ckpt)), u32(one))
        grp.ckpt_upload(ckpt)
        grp.fedavg_resident(MEDIAN)
        assert np.array_equal(u32(grp.ckpt_download()), u32(one))
        grp.ckpt_upload(ckpt)
        grp.fold_slots_finish_resident(MEDIAN, list(range(n)))
        assert np.array_equal(u32(grp.ckpt_download()), u32(one))


def test_scattered_slots_in_any_order(eng):
    """Reports where they landed, non-reporters' slots between them (one holds a stale diff that is
    not listed); a permuted list of the same rows gives the same bits."""
    p, n = 1000, 10
    rng = np.random.default_rng(1000)
    diffs = special_rows(n, p, 1010)
    ckpt = rng.standard_normal(p).astype(F)
    slot_of = rng.permutation(n + 6)[:n + 1]
    want = MO.fedavg_median(ckpt, diffs)
    for order in (np.arange(n), rng.permutation(n)):
        load(eng, np.concatenate([diffs, np.full((1, p), np.nan, F)]), slot_of, cap=n + 6)
        eng.ckpt_upload(ckpt)
        eng.fold_slots_finish_resident(MEDIAN, slot_of[order])
        assert MO.same_bits(eng.ckpt_download(), want)


def test_more_rows_than_a_row_table(eng):
    """513 rows over 1,000 params in one finish: the rows reach the kernels as a device table."""
    p, n = 1000, 513
    rows, ckpt = tall_rows(p, 513)
    rng = np.random.default_rng(513)
    slot_of = rng.permutation(n + 3)[:n]
    want = MO.fedavg_median(ckpt, rows)
    load(eng, rows, slot_of, cap=n + 3)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(MEDIAN, slot_of)
    assert MO.same_bits(eng.ckpt_download(), want)
    for k in range(n):  # (a finish frees its slots) the same rows, listed in another order
        eng.ingest(int(slot_of[k]), rows[k])
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(MEDIAN, slot_of[rng.permutation(n)])
    assert MO.same_bits(eng.ckpt_download(), want)


def test_robust_where_the_mean_and_the_trimmed_mean_are_not(eng):
    """5 hostile rows of 11: the median stays inside the honest rows' range in every column; the
    plain mean and the trimmed mean at b = 2 of the same slab do not stay finite."""
    n, bad, p = 11, 5, 1001
    rng = np.random.default_rng(11)
    diffs = rng.standard_normal((n, p)).astype(F)
    hostile = rng.permutation(n)[:bad]
    diffs[hostile] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F), size=(bad, p))
    good = np.delete(diffs, hostile, axis=0)
    ckpt = rng.standard_normal(p).astype(F)
    load(eng, diffs)
    got = eng.fedavg(MEDIAN, ckpt)
    assert MO.same_bits(got, MO.fedavg_median(ckpt, diffs)) and np.isfinite(got).all()
    m = MO.median_of_rows(diffs)
    assert np.all(m >= good.min(0)) and np.all(m <= good.max(0)) and np.array_equal(u32(got), u32(ckpt - m))
    assert not np.isfinite(eng.fedavg(MEAN, ckpt)).all()
    try:
        eng.set_trim(2)
        trimmed = eng.fedavg(TRIMMED, ckpt)
        assert TO.same_bits(trimmed, TO.fedavg_trimmed(ckpt, diffs, 2)) and not np.isfinite(trimmed).all()
    finally:
        eng.set_trim(0)


def test_refusals_leave_the_context_usable(eng, G):
    from pygrid_amd.exceptions import AggregationError

    n = 9
    ckpt, diffs, want = G[f"ckpt_{n}"], G[f"diffs_{n}"], G[f"out_{n}"]

    def refused(status, fn, *a):
        with pytest.raises(AggregationError) as e:
            fn(*a)
        assert e.value.status == status, e.value

    def still_right():
        load(eng, diffs)
        assert MO.same_bits(eng.fedavg(MEDIAN, ckpt), want)
        assert MO.same_bits(eng.fedavg(MEAN, ckpt), O.fedavg_mean([ckpt], [[d] for d in diffs])[0])

    load(eng, diffs)
    eng.ckpt_upload(ckpt)
    refused(UNSUPPORTED, eng.fold_slots, MEDIAN, [0, 1])  # nothing can be folded early
    eng.fold_slots_finish_resident(MEDIAN, list(range(n)))  # ... and nothing was
    assert MO.same_bits(eng.ckpt_download(), want)
    still_right()
    refused(UNSUPPORTED, eng.stream_begin, MEDIAN)
    still_right()
    load(eng, diffs)
    eng.ckpt_upload(ckpt)
    eng.fold_slots(MEAN, [0, 1])  # the cycle has a running fold state of another mode
    refused(STATE, eng.fold_slots_finish_resident, MEDIAN, list(range(2, n)))
    eng.fold_slots_finish_resident(MEAN, list(range(2, n)))
    assert MO.same_bits(eng.ckpt_download(), O.fedavg_mean([ckpt], [[d] for d in diffs])[0])
    still_right()
    load(eng, diffs)
    eng.ckpt_upload(ckpt)
    refused(STATE, eng.fold_slots_finish_resident, MEDIAN, [])  # a closing fold of 0 diffs, as for the other modes
    refused(STATE, eng.fold_slots_finish_resident, MEAN, [])
    still_right()
    eng.set_layout([diffs.shape[1]])
    eng.reserve(2, 1, 2)  # an int64 slab
    refused(STATE, eng.fedavg, MEDIAN, ckpt)
    refused(STATE, eng.fold_slots_finish_resident, MEDIAN, [0])
    still_right()


MNIST_SHAPES = [(392, 784), (392,), (10, 392), (10,)]


def mnist_case(n, hostile=(0, 3, 5)):
    assert sum(int(np.prod(s)) for s in MNIST_SHAPES) == 311_650
    rng = np.random.default_rng(311)
    ckpt = [rng.standard_normal(s).astype(F) for s in MNIST_SHAPES]
    diffs = [[(rng.standard_normal(s) * 1e-2).astype(F) for s in MNIST_SHAPES] for _ in range(n)]
    for w in hostile:  # a NaN, infinities and 1e30 from a minority of the workers
        diffs[w][0][0, :5] = (np.nan, np.inf, -np.inf, 1e30, -1e30)
        diffs[w][3][:] = np.nan
    return ckpt, diffs


def test_cycle_aggregator_from_state_bytes(eng):
    """MNIST size, seven clients, three hostile, server_config["diff_median"] = True; then a chained
    cycle WITHOUT the key is the plain mean."""
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.exceptions import MedianUnavailableError
    from pygrid_amd.state_schema import build_state_fast, parse_state

    ckpt, diffs = mnist_case(7)
    agg = CycleAggregator(eng)
    pbs = [build_state_fast(d) for d in diffs]
    new = agg.average_plan_diffs({"diff_median": True}, build_state_fast(ckpt), pbs)
    want = MO.fedavg_median_tensors(ckpt, diffs)
    for g, w in zip(parse_state(new), want):
        assert np.array_equal(u32(g), u32(w)) and np.isfinite(g).all()
    got = agg.average_params({"diff_median": True}, ckpt, diffs)
    for g, w in zip(got, want):
        assert np.array_equal(u32(g), u32(w))
    with pytest.raises(MedianUnavailableError):
        agg.average_plan_diffs({"diff_median": True, "diff_trim_count": 1}, new, pbs)
    new2 = agg.average_plan_diffs({}, new, pbs[1:3])
    for g, w in zip(parse_state(new2), O.fedavg_mean(want, diffs[1:3])):
        assert np.array_equal(u32(g), u32(w))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
def test_ranged_report_time_close(pinned, path):
    """IncrementalCycle(median=True) on a 1.11 M-param model (just over 2^20: the FINAL pass runs as
    4 MiB ranges behind the ranged ingest of the last report); worker 6 never reports, worker 2
    re-reports; a second cycle chained on the resident checkpoint."""
    import base64

    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.report import PinnedPool, b64decode
    from pygrid_amd.state_schema import build_state_fast, parse_state

    shapes = [(1100, 1000), (1000,), (10, 1000), (10,)]
    numel = [int(np.prod(s)) for s in shapes]
    assert sum(numel) > 1 << 20
    rng = np.random.default_rng(1111)
    ckpt = [rng.standard_normal(s).astype(F) for s in shapes]
    diffs = [[(rng.standard_normal(s) * 1e-2).astype(F) for s in shapes] for _ in range(6)]
    diffs[5][0][::7] = np.inf  # the last reporter is a hostile one
    diffs[1][0][::5] = np.nan
    first_of_2 = [(rng.standard_normal(s) * 1e3).astype(F) for s in shapes]  # replaced by its re-report
    pbs = [build_state_fast(d) for d in diffs]
    pool = PinnedPool(max_blocks=8) if pinned else None

    def as_report(pb):
        return b64decode(base64.b64encode(pb).decode(), into=pool) if pinned else pb

    with make_engine(path) as eng:
        ck_pb = build_state_fast(ckpt)
        want = ckpt
        for cycle in range(2):
            inc = IncrementalCycle(eng, numel, slots=8, fold_batch=2, checkpoint=ck_pb, median=True)
            assert os.environ.get("PGH_INGEST_RANGES", "1") != "0"
            for w in range(7):
                inc.assigned(w)
            inc.reported(2, as_report(build_state_fast(first_of_2)))
            for w in (0, 1, 3, 2, 4, 5):  # worker 6 never reports
                inc.reported(w, as_report(pbs[w]))
            ck_pb = inc.close(ck_pb)
            want = MO.fedavg_median_tensors(want, diffs)
            for g, w in zip(parse_state(ck_pb), want):
                assert np.array_equal(u32(g), u32(w)), cycle
                assert np.isfinite(g).all()
            assert inc.last_close["n"] == 6 and inc.last_close["median"] is True and inc.last_close["early"] == 0
            assert inc.last_close["from_hbm"] == 6
    if pool is not None:
        pool.close()


def test_installed_node_close(engine):
    """One close of the installed node on the MNIST-sized model, diff_median in the FL process's
    server_config, reports copied into HBM as they arrive."""
    from fake_node import assign, host_process, make_node
    from pygrid_amd import node as pnode
    from pygrid_amd import state
    from pygrid_amd.state_schema import build_state_fast

    ckpt, diffs = mnist_case(5, hostile=(1, 4))
    mod = make_node()
    node = pnode.install(mod, engine=engine, framing="template", fold_batch=1)
    try:
        cfg = {"min_diffs": 5, "max_diffs": 5, "num_cycles": 0, "cycle_length": None, "diff_median": True}
        ck_pb = build_state_fast(ckpt)
        proc, model, _ = host_process(mod, cfg, ck_pb)
        keys = {w: assign(mod, w, proc) for w in range(6)}
        for w in (0, 1, 2, 4, 3):
            mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diffs[w]))
        assert mod.cycle_manager.task_errors == []
        want = MO.flat(MO.fedavg_median_tensors(ckpt, diffs))
        assert np.isfinite(want).all()
        assert mod.model_manager.load(model_id=model.id).value == state.serialize_model_params(ck_pb, want)
        assert node.stats["closes_report_time"] == 1
    finally:
        node.uninstall()
