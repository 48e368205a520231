"""GPU: coordinate-wise trimmed mean (PGH_TRIMMED_MEAN, kernel K8), bit-exact against
tests/trim_oracle.py and the golden file tests/golden/trim_cases.npz (NaNs by position).  The
streaming definition is in DESIGN.md section 5 and include/pgh_api.h."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_trim_golden as GG  # noqa: E402
import trim_oracle as TO  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
TRIMMED = 4
ARG, STATE, UNSUPPORTED = -1, -3, -6
VECS = (4, 1)
SHAPE_P = (1, 3, 5, 4097, 2 * 65536 + 5)  # the last one spans several workgroups of either form


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GG.GOLDEN)


@pytest.fixture(scope="module")
def engines():
    """One context per column width: PGH_TRIM_VEC is read when a context is made."""
    from pygrid_amd import Engine

    made = {}
    old = os.environ.get("PGH_TRIM_VEC")
    try:
        for vec in VECS:
            os.environ["PGH_TRIM_VEC"] = str(vec)
            made[vec] = Engine(int(os.environ.get("PGH_DEVICE", "0")))
    finally:
        if old is None:
            os.environ.pop("PGH_TRIM_VEC", None)
        else:
            os.environ["PGH_TRIM_VEC"] = old
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(params=VECS, ids=lambda v: f"vec{v}")
def eng(request, engines):
    e = engines[request.param]
    e.forced_vec = request.param
    yield e
    e.set_trim(0)


@functools.lru_cache(maxsize=None)
def shape_rows(p):
    """37 rows of p floats (specials in the first three) and a checkpoint: every N takes a prefix."""
    return GG.special_rows(37, p, 4000 + p), np.random.default_rng(p).standard_normal(p).astype(F)


@functools.lru_cache(maxsize=None)
def shape_want(p, n, b):
    rows, ckpt = shape_rows(p)
    return TO.fedavg_trimmed(ckpt, rows[:n], b)


def load(eng, diffs, slots=None, cap=None):
    eng.set_layout([diffs.shape[1]])
    eng.reserve(cap or len(diffs))
    for k, d in enumerate(diffs):
        eng.ingest(k if slots is None else int(slots[k]), d)


@pytest.mark.parametrize("b", range(1, 9))
def test_shapes(eng, b):
    """N at the smallest legal count, one past it, past a row batch, and 37; P below a column, ragged
    last columns, and several workgroups."""
    eng.set_trim(b)
    for p in SHAPE_P:
        rows, ckpt = shape_rows(p)
        eng.set_layout([p])
        eng.reserve(37)
        assert eng.effective_variant(TRIMMED) == (40 if eng.forced_vec == 4 else 41)
        eng.set_variant(13)  # the table of pgh_set_variant does not reach trimmed folds
        assert eng.effective_variant(TRIMMED) == (40 if eng.forced_vec == 4 else 41)
        eng.set_variant(-1)
        for n in sorted({2 * b + 1, 2 * b + 2, 2 * b + 9, 37}):
            eng.reset()
            for k in range(n):
                eng.ingest(k, rows[k])
            got = eng.fedavg(TRIMMED, ckpt)
            assert TO.same_bits(got, shape_want(p, n, b)), (p, n, b)


def test_narrow_blocks(monkeypatch):
    """PGH_BLOCK_BYTES=4096: blocks of 1,024 columns, in a context of its own."""
    from pygrid_amd import Engine

    monkeypatch.setenv("PGH_BLOCK_BYTES", "4096")
    p, n, b = SHAPE_P[-1], 37, 3
    rows, ckpt = shape_rows(p)
    with Engine(0) as e:
        load(e, rows[:n])
        assert e.slab()[1] == 1024 and e.slab()[2] > 0
        e.set_trim(b)
        assert TO.same_bits(e.fedavg(TRIMMED, ckpt), shape_want(p, n, b))


def test_specials_match_the_golden_file(eng, G):
    """+-0, subnormals, +-inf, NaNs of both signs, an all-equal column, ties at the trim boundary."""
    for n, b in GG.CASES:
        ckpt, diffs = G[f"ckpt_{n}_{b}"], G[f"diffs_{n}_{b}"]
        want = TO.fedavg_trimmed(ckpt, diffs, b)
        assert TO.same_bits(want, G[f"out_{n}_{b}"])
        load(eng, diffs)
        eng.set_trim(b)
        got = eng.fedavg(TRIMMED, ckpt)
        assert TO.same_bits(got, want), (n, b)
        assert got[11] == ckpt[11] - F(0.25)  # the all-equal column


def test_more_nans_than_b(eng):
    """A column with more than b NaNs of one sign keeps a NaN: NaN out, where the oracle's is."""
    n, b, p = 9, 2, 67
    rng = np.random.default_rng(92)
    diffs = rng.standard_normal((n, p)).astype(F)
    diffs[[0, 4, 8], 3] = np.nan    # three +NaN: one survives the trim
    diffs[[1, 2, 3], 9] = -np.nan   # three -NaN
    diffs[[0, 1], 20] = np.nan      # two: trimmed away
    ckpt = rng.standard_normal(p).astype(F)
    want = TO.fedavg_trimmed(ckpt, diffs, b)
    assert np.isnan(want[[3, 9]]).all() and np.isfinite(np.delete(want, [3, 9])).all()
    load(eng, diffs)
    eng.set_trim(b)
    assert TO.same_bits(eng.fedavg(TRIMMED, ckpt), want)


def test_robust_where_the_mean_is_not(eng):
    """b hostile rows per side: the trimmed result stays inside the honest rows' range; the plain
    mean of the same slab does not stay finite."""
    n, b, p = 11, 2, 1001
    rng = np.random.default_rng(11)
    diffs = rng.standard_normal((n, p)).astype(F)
    diffs[0], diffs[1] = np.nan, np.inf
    diffs[2], diffs[3] = -np.inf, F(-3e38)
    ckpt = rng.standard_normal(p).astype(F)
    load(eng, diffs)
    eng.set_trim(b)
    got = eng.fedavg(TRIMMED, ckpt)
    assert TO.same_bits(got, TO.fedavg_trimmed(ckpt, diffs, b))
    assert np.isfinite(got).all()
    assert not np.isfinite(eng.fedavg(0, ckpt)).any()


@pytest.mark.parametrize("b", (1, 3, 8))
def test_state_carry_through_slot_folds(eng, b):
    """fold_slots batches that split inside the fill phase (1, b, 2b - 1 rows, then the rest), in
    scattered slots with non-reporters between them; then a restart and a re-fold in other batches."""
    p, n = 1000, 2 * b + 9
    rng = np.random.default_rng(100 + b)
    diffs = GG.special_rows(n, p, 500 + b)
    ckpt = rng.standard_normal(p).astype(F)
    slot_of = rng.permutation(n + 5)[:n]
    want = TO.fedavg_trimmed(ckpt, diffs, b)
    eng.set_trim(b)
    load(eng, diffs, slot_of, cap=n + 5)
    eng.ckpt_upload(ckpt)
    cuts = np.cumsum([0, 1, b, 2 * b - 1])
    for a, z in zip(cuts[:-1], cuts[1:]):
        eng.fold_slots(TRIMMED, slot_of[a:z])
    eng.fold_slots_finish_resident(TRIMMED, slot_of[cuts[-1]:])
    assert TO.same_bits(eng.ckpt_download(), want)
    # a re-report: the folds so far are dropped, the rows go in again (row 0 changed) and are
    # folded in other batches, the finish with no rows of its own
    for k in range(n):
        eng.ingest(int(slot_of[k]), diffs[k])
    eng.ckpt_upload(ckpt)
    eng.fold_slots(TRIMMED, slot_of[:b + 1])
    eng.fold_restart()
    diffs2 = diffs.copy()
    diffs2[0] = diffs[0][::-1]
    for k in range(b + 1):
        eng.ingest(int(slot_of[k]), diffs2[k])
    eng.fold_slots(TRIMMED, slot_of[:2 * b + 1])
    eng.fold_slots(TRIMMED, slot_of[2 * b + 1:])
    eng.fold_slots_finish_resident(TRIMMED, [])
    assert TO.same_bits(eng.ckpt_download(), TO.fedavg_trimmed(ckpt, diffs2, b))


def test_more_rows_than_a_row_table(eng):
    """513 rows over 1,000 params in one finish: two row-table launches, the state in HBM between."""
    p, n, b = 1000, 513, 2
    rng = np.random.default_rng(513)
    diffs = rng.standard_normal((n, p)).astype(F)
    diffs[::50, ::3] = np.inf
    ckpt = rng.standard_normal(p).astype(F)
    slot_of = rng.permutation(n)
    load(eng, diffs, slot_of)
    eng.set_trim(b)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(TRIMMED, slot_of)
    assert TO.same_bits(eng.ckpt_download(), TO.fedavg_trimmed(ckpt, diffs, b))


def test_ranges_and_chained_resident_cycles(eng):
    import torch

    p, n, b = 8197, 12, 3
    rng = np.random.default_rng(8197)
    diffs = GG.special_rows(n, p, 8197)
    ckpt = rng.standard_normal(p).astype(F)
    want = TO.fedavg_trimmed(ckpt, diffs, b)
    load(eng, diffs)
    eng.set_trim(b)
    ck = torch.from_numpy(ckpt).cuda()
    out = torch.zeros_like(ck)
    cut = 4100  # a multiple of 4, not of a block
    eng.fedavg_device_range(TRIMMED, 0, cut, ck.data_ptr(), out.data_ptr())
    eng.fedavg_device_range(TRIMMED, cut, p - cut, ck.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert TO.same_bits(out.cpu().numpy(), want)
    eng.ckpt_upload(ckpt)
    eng.fedavg_resident(TRIMMED)
    assert TO.same_bits(eng.ckpt_download(), want)
    eng.fedavg_resident(TRIMMED)  # the new checkpoint is the next cycle's input
    assert TO.same_bits(eng.ckpt_download(), TO.fedavg_trimmed(want, diffs, b))


def test_group_and_shard_match_one_context(engine):
    from pygrid_amd import Engine

    p, n, b = 70001, 9, 2
    diffs = GG.special_rows(n, p, 70001)
    ckpt = np.random.default_rng(7).standard_normal(p).astype(F)
    want = TO.fedavg_trimmed(ckpt, diffs, b)
    try:
        engine.set_trim(b)
        load(engine, diffs)
        one = engine.fedavg(TRIMMED, ckpt)
        assert TO.same_bits(one, want)
        lo, hi = 35000, p  # a shard: nothing in the fold looks along a row
        engine.set_layout([p])
        engine.set_shard(lo, hi)
        engine.reserve(n)
        for k, d in enumerate(diffs):
            engine.ingest(k, d[lo:hi])
        assert np.array_equal(u32(engine.fedavg(TRIMMED, ckpt[lo:hi])), u32(one[lo:hi]))
    finally:
        engine.set_trim(0)
        engine.set_layout([p])
    with Engine(devices=[0, 0]) as grp:
        grp.set_layout([p])
        grp.reserve(n + 2)
        grp.set_trim(b)
        for k, d in enumerate(diffs):
            grp.ingest(k, d)
        assert np.array_equal(u32(grp.fedavg(TRIMMED, ckpt)), u32(one))
        grp.ckpt_upload(ckpt)
        grp.fold_slots(TRIMMED, [0, 1, 2])
        grp.fold_slots_finish_resident(TRIMMED, list(range(3, n)))
        assert np.array_equal(u32(grp.ckpt_download()), u32(one))


def test_refusals_leave_the_context_usable(engine, G):
    from pygrid_amd.exceptions import AggregationError

    n, b = 5, 2
    ckpt, diffs = G[f"ckpt_{n}_{b}"], G[f"diffs_{n}_{b}"]
    want = G[f"out_{n}_{b}"]

    def refused(status, fn, *a):
        with pytest.raises(AggregationError) as e:
            fn(*a)
        assert e.value.status == status, e.value

    def trimmed_ok():
        load(engine, diffs)
        engine.set_trim(b)
        assert TO.same_bits(engine.fedavg(TRIMMED, ckpt), want)

    try:
        engine.set_trim(0)
        load(engine, diffs)
        refused(STATE, engine.fedavg, TRIMMED, ckpt)  # the mode without set_trim
        engine.ckpt_upload(ckpt)
        refused(STATE, engine.fedavg_resident, TRIMMED)
        refused(STATE, engine.fold_slots, TRIMMED, [0, 1])
        trimmed_ok()
        refused(ARG, engine.set_trim, 9)
        refused(ARG, engine.set_trim, -1)
        trimmed_ok()
        load(engine, diffs[:4])  # N = 2b
        refused(STATE, engine.fedavg, TRIMMED, ckpt)
        engine.ckpt_upload(ckpt)
        refused(STATE, engine.fedavg_resident, TRIMMED)
        refused(STATE, engine.fold_slots_finish_resident, TRIMMED, [0, 1, 2, 3])
        assert TO.same_bits(engine.fedavg(0, ckpt), O.fedavg_mean([ckpt], [[d] for d in diffs[:4]])[0])
        trimmed_ok()
        load(engine, diffs)  # changing b with slot folds of the cycle under way
        engine.ckpt_upload(ckpt)
        engine.fold_slots(TRIMMED, [0, 1])
        refused(STATE, engine.set_trim, 1)
        engine.set_trim(b)  # the same value is no change
        engine.fold_slots_finish_resident(TRIMMED, [2, 3, 4])
        assert TO.same_bits(engine.ckpt_download(), want)
        engine.set_trim(1)  # between cycles it may change
        trimmed_ok()
        refused(UNSUPPORTED, engine.stream_begin, TRIMMED)
        trimmed_ok()
        engine.set_layout([diffs.shape[1]])
        engine.reserve(2, 1, 2)  # an int64 slab
        refused(STATE, engine.fedavg, TRIMMED, ckpt)
        trimmed_ok()
    finally:
        engine.set_trim(0)


MNIST_SHAPES = [(392, 784), (392,), (10, 392), (10,)]


def mnist_case(n, hostile=(0, 3)):
    assert sum(int(np.prod(s)) for s in MNIST_SHAPES) == 311_650
    rng = np.random.default_rng(311)
    ckpt = [rng.standard_normal(s).astype(F) for s in MNIST_SHAPES]
    diffs = [[(rng.standard_normal(s) * 1e-2).astype(F) for s in MNIST_SHAPES] for _ in range(n)]
    for w in hostile:  # a NaN, an infinity and 1e30 from two workers
        diffs[w][0][0, :5] = (np.nan, np.inf, -np.inf, 1e30, -1e30)
        diffs[w][3][:] = np.nan
    return ckpt, diffs


def test_cycle_aggregator_from_state_bytes(engine):
    """MNIST size, seven clients, two hostile, server_config["diff_trim_count"] = 2; then a chained
    cycle WITHOUT the key is the plain mean: the count does not leak into the next process's cycle."""
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.exceptions import TrimUnavailableError
    from pygrid_amd.state_schema import build_state_fast, parse_state

    ckpt, diffs = mnist_case(7)
    agg = CycleAggregator(engine)
    pbs = [build_state_fast(d) for d in diffs]
    try:
        new = agg.average_plan_diffs({"diff_trim_count": 2}, build_state_fast(ckpt), pbs)
        want = TO.fedavg_trimmed_tensors(ckpt, diffs, 2)
        for g, w in zip(parse_state(new), want):
            assert np.array_equal(u32(g), u32(w)) and np.isfinite(g).all()
        got = agg.average_params({"diff_trim_count": 2}, ckpt, diffs)
        for g, w in zip(got, want):
            assert np.array_equal(u32(g), u32(w))
        with pytest.raises(TrimUnavailableError):
            agg.average_plan_diffs({"diff_trim_count": 2}, new, pbs[:4])
        new2 = agg.average_plan_diffs({}, new, pbs[1:3])
        for g, w in zip(parse_state(new2), O.fedavg_mean(want, diffs[1:3])):
            assert np.array_equal(u32(g), u32(w))
    finally:
        engine.set_trim(0)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
def test_ranged_report_time_close(pinned):
    """IncrementalCycle(trim_count=) on a 1.11 M-param model (just over 2^20: the FINAL pass runs as
    4 MiB ranges behind the ranged ingest of the last report), early folds on; a second cycle chained
    on the resident checkpoint."""
    import base64

    from pygrid_amd import Engine
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.report import PinnedPool, b64decode
    from pygrid_amd.state_schema import build_state_fast, parse_state

    shapes = [(1100, 1000), (1000,), (10, 1000), (10,)]
    numel = [int(np.prod(s)) for s in shapes]
    assert sum(numel) > 1 << 20
    rng = np.random.default_rng(1111)
    ckpt = [rng.standard_normal(s).astype(F) for s in shapes]
    diffs = [[(rng.standard_normal(s) * 1e-2).astype(F) for s in shapes] for _ in range(6)]
    diffs[5][0][::7] = np.inf  # the last reporter is the hostile one
    pbs = [build_state_fast(d) for d in diffs]
    pool = PinnedPool(max_blocks=8) if pinned else None

    def as_report(pb):
        return b64decode(base64.b64encode(pb).decode(), into=pool)

    with Engine(0) as eng:
        ck_pb = build_state_fast(ckpt)
        want = ckpt
        for cycle in range(2):
            inc = IncrementalCycle(eng, numel, slots=8, fold_batch=2, checkpoint=ck_pb, trim_count=1)
            assert os.environ.get("PGH_INGEST_RANGES", "1") != "0"
            for w in range(7):
                inc.assigned(w)
            for w in (0, 1, 3, 2, 4, 5):  # worker 6 never reports
                inc.reported(w, as_report(pbs[w]) if pinned else pbs[w])
            ck_pb = inc.close(ck_pb)
            want = TO.fedavg_trimmed_tensors(want, diffs, 1)
            for g, w in zip(parse_state(ck_pb), want):
                assert np.array_equal(u32(g), u32(w)), cycle
                assert np.isfinite(g).all()
            assert inc.last_close["n"] == 6 and inc.last_close["trim"] == 1 and inc.last_close["early"] >= 2
    if pool is not None:
        pool.close()


def test_installed_node_close(engine):
    """One close of the installed node on the MNIST-sized model, diff_trim_count in the FL process's
    server_config, reports folded as they arrive."""
    from fake_node import assign, host_process, make_node
    from pygrid_amd import node as pnode
    from pygrid_amd import state
    from pygrid_amd.state_schema import build_state_fast

    ckpt, diffs = mnist_case(5, hostile=(1,))
    mod = make_node()
    node = pnode.install(mod, engine=engine, framing="template", fold_batch=1)
    try:
        cfg = {"min_diffs": 5, "max_diffs": 5, "num_cycles": 0, "cycle_length": None, "diff_trim_count": 1}
        ck_pb = build_state_fast(ckpt)
        proc, model, _ = host_process(mod, cfg, ck_pb)
        keys = {w: assign(mod, w, proc) for w in range(6)}
        for w in (0, 1, 2, 4, 3):
            mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diffs[w]))
        assert mod.cycle_manager.task_errors == []
        want = TO.flat(TO.fedavg_trimmed_tensors(ckpt, diffs, 1))
        assert np.isfinite(want).all()
        assert mod.model_manager.load(model_id=model.id).value == state.serialize_model_params(ck_pb, want)
        assert node.stats["closes_report_time"] == 1
    finally:
        node.uninstall()
        engine.set_trim(0)
