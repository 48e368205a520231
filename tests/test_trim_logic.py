"""CPU: the coordinate-wise trimmed mean -- the oracle's pins (tests/trim_oracle.py against a sort
and the golden file), the robustness property, the library's argument check (no GPU), and the host
logic that drives the engine: ``trim_count_of``, ``select_mode``, fail-closed closes,
``IncrementalCycle`` and the installed node over a numpy engine that trims with the oracle."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_trim_golden as GG  # noqa: E402
import trim_oracle as TO  # noqa: E402
from fake_engine import NumpyEngine  # noqa: E402
from fake_node import assign, host_process, make_node  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pygrid_amd import state  # noqa: E402
from pygrid_amd.cycle import TRIM_KEY, CycleAggregator, make_average_plan_diffs, select_mode, trim_count_of  # noqa: E402
from pygrid_amd.engine import ITERATIVE_MEAN, MEAN, MODE_NAMES, TRIMMED_MEAN, WEIGHTED_MEAN  # noqa: E402
from pygrid_amd.exceptions import AggregationError, PlanNotAcceleratedError, TrimUnavailableError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402

F = np.float32


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GG.GOLDEN)


# ---- the oracle ----------------------------------------------------------------------------------

def test_key_is_a_total_order_and_its_own_inverse():
    vals = np.array([-np.nan, -np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf, np.nan], F)
    k = TO.key(vals)
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert np.array_equal(u32(TO.unkey(k)), u32(vals))
    bits = np.random.default_rng(0).integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(u32(TO.unkey(TO.key(bits.view(F)))), bits)


def test_oracle_matches_the_golden_file(G):
    assert [tuple(c) for c in G["cases"]] == list(GG.CASES)
    for n, b in GG.CASES:
        ckpt, diffs = GG.case_inputs(n, b)
        assert np.array_equal(u32(diffs), u32(G[f"diffs_{n}_{b}"])) and np.array_equal(u32(ckpt), u32(G[f"ckpt_{n}_{b}"]))
        st = TO.TrimState(GG.CASE_P, b)
        for row in G[f"diffs_{n}_{b}"]:
            st.step(row)
        assert np.array_equal(st.lo, G[f"lo_{n}_{b}"]) and np.array_equal(st.hi, G[f"hi_{n}_{b}"])
        assert TO.same_bits(st.close(ckpt), G[f"out_{n}_{b}"])
        assert np.array_equal(u32(G[f"out_{n}_{b}"][11]), u32(ckpt[11] - F(0.25)))  # the all-equal column


@pytest.mark.parametrize("n,b", list(GG.CASES) + [(19, 8), (64, 5), (7, 3)])
def test_kept_values_are_the_middle_of_the_sort(n, b):
    """Independent of the network: the evicted multiset is sort(keys)[b : N - b], lo and hi end as
    the two ends, on random and special inputs, whatever the row order."""
    p = 311
    for seed, every in ((n, 7), (100 + n, 2), (200 + n, 10 ** 9)):
        d = GG.special_rows(n, p, seed, every=every, rows=n)
        st = TO.TrimState(p, b)
        for row in d:
            st.step(row)
        K = np.sort(TO.key(d), axis=0)
        kept = np.sort(TO.key(np.stack(st.kept)), axis=0)
        assert np.array_equal(kept, K[b:n - b])
        assert np.array_equal(np.sort(st.lo, axis=0), K[:b]) and np.array_equal(np.sort(st.hi, axis=0), K[n - b:])
        # finite columns: the f32 left fold of the kept values in eviction order, nothing else
        acc = st.kept[0].copy()
        with np.errstate(all="ignore"):
            for v in st.kept[1:]:
                acc = (acc + v).astype(F)
        assert TO.same_bits(acc, st.acc)


def test_fewer_than_2b_plus_1_rows_is_an_error():
    with pytest.raises(ValueError):
        TO.fedavg_trimmed(np.zeros(3, F), np.zeros((4, 3), F), 2)
    with pytest.raises(ValueError):
        TO.TrimState(3, 9)
    assert np.array_equal(TO.fedavg_trimmed(np.ones(3, F), [np.full(3, x, F) for x in (5, -7, 2)], 1), np.full(3, -1, F))


def test_minus_zero_survives():
    out = TO.fedavg_trimmed(np.zeros(1, F), [np.array([x], F) for x in (-1.0, -0.0, 1.0)], 1)
    assert u32(out)[0] == u32(F(0.0) - F(-0.0) / F(1))[0]
    st = TO.TrimState(1, 1)
    for x in (-1.0, -0.0, 1.0):
        st.step(np.array([x], F))
    assert u32(st.acc)[0] == 0x80000000  # the sum starts at the first kept value, not at +0


@pytest.mark.parametrize("b", [1, 2, 4, 8])
def test_b_hostile_rows_per_side_cannot_move_a_coordinate(b):
    p, honest = 500, 9
    rng = np.random.default_rng(b)
    good = rng.standard_normal((honest, p)).astype(F)
    hostile = np.array([np.nan, -np.nan, np.inf, -np.inf, 3e38, -3e38], F)
    high = rng.choice(hostile[[0, 2, 4]], size=(b, p))   # land above every honest value
    high[0] = rng.choice(hostile[[0, 2]], size=p)        # (a NaN or an infinity in every column)
    low = rng.choice(hostile[[1, 3, 5]], size=(b, p))    # below
    rows = np.concatenate([good, high, low])[rng.permutation(honest + 2 * b)]
    ckpt = rng.standard_normal(p).astype(F)
    out = TO.fedavg_trimmed(ckpt, rows, b)
    assert np.isfinite(out).all()
    avg = (ckpt.astype(np.float64) - out.astype(np.float64))
    # |values| < 6: the 8 f32 additions round by at most 2^-19 each (sums below 64), 1.7e-6 after the
    # division by 9; the division and ckpt - avg add at most 2^-22 + 2^-21; the f64 difference nothing
    tol = 1e-5
    assert np.all(avg >= good.min(0) - tol) and np.all(avg <= good.max(0) + tol)
    mean = O.fedavg_mean([ckpt], [[r] for r in rows])[0]
    assert not np.isfinite(mean).any()


# ---- the ABI -----------------------------------------------------------------------------------------

def test_abi_names_and_null_context():
    from pygrid_amd import _lib

    assert MODE_NAMES[TRIMMED_MEAN] == "trimmed_mean" and TRIMMED_MEAN == 4
    lib = _lib.load()
    assert "pgh_set_trim" in _lib.SIGNATURES
    assert lib.pgh_set_trim(C.c_void_p(None), 1) == -1  # PGH_E_ARG
    assert lib.pgh_abi_version() == 10
    header = (Path(__file__).resolve().parent.parent / "include" / "pgh_api.h").read_text()
    assert "PGH_TRIMMED_MEAN = 4" in header and "int pgh_set_trim(pgh_ctx* ctx, int b);" in header


# ---- server_config["diff_trim_count"] ------------------------------------------------------------------

def test_trim_count_of():
    assert TRIM_KEY == "diff_trim_count"
    assert trim_count_of({}) is None and trim_count_of({TRIM_KEY: None}) is None
    assert trim_count_of({TRIM_KEY: 1}) == 1 and trim_count_of({TRIM_KEY: 8}) == 8
    assert trim_count_of({TRIM_KEY: 3.0}) == 3 and trim_count_of({TRIM_KEY: np.int64(2)}) == 2
    assert type(trim_count_of({TRIM_KEY: np.int64(2)})) is int
    for bad in (True, False, 2.5, 0, -1, 9, 100, "2", [2], float("nan"), float("inf")):
        with pytest.raises(AggregationError):
            trim_count_of({TRIM_KEY: bad})


def canonical(avg, item, num):
    return [(a * num + i) / (num + 1) for a, i in zip(avg, item)]


def mean_plan(diffs):
    import torch as th
    from functools import reduce

    return [th.div(reduce(th.add, [d[j] for d in diffs]), len(diffs)) for j in range(len(diffs[0]))]


def other_plan(diffs):
    return [sum(d[j] for d in diffs) * 0.5 for j in range(len(diffs[0]))]


def test_select_mode():
    assert select_mode({}, trim_count=2) == TRIMMED_MEAN
    assert select_mode({}, mean_plan, mean_plans="probe", trim_count=2) == TRIMMED_MEAN
    with pytest.raises(TrimUnavailableError):
        select_mode({"iterative_plan": True}, canonical, trim_count=2)
    with pytest.raises(TrimUnavailableError):
        select_mode({}, weights=[1.0, 2.0], trim_count=2)
    with pytest.raises(TrimUnavailableError):
        select_mode({}, mean_plan, trim_count=2)  # declined: non-iterative plans are user code by default
    with pytest.raises(TrimUnavailableError):
        select_mode({}, other_plan, mean_plans="probe", trim_count=2)
    with pytest.raises(TrimUnavailableError):
        select_mode({}, clip_norm=1.0, trim_count=2)
    assert not issubclass(TrimUnavailableError, PlanNotAcceleratedError)
    assert issubclass(TrimUnavailableError, AggregationError)
    # without a trim count every verdict is what it was
    assert select_mode({}) == MEAN
    assert select_mode({"iterative_plan": True}, canonical) == ITERATIVE_MEAN
    assert select_mode({}, weights=[1.0]) == WEIGHTED_MEAN


# ---- a numpy engine that trims with the oracle -------------------------------------------------------------

class TrimEngine(NumpyEngine):
    def __init__(self):
        super().__init__()
        self.trim = 0
        self.clip = None

    def set_trim(self, b):
        if not 0 <= int(b) <= 8:
            raise AggregationError("trim count outside [0,8]", status=-1)
        if int(b) != self.trim and self.folded:
            raise AggregationError("trim count changed mid-cycle", status=-3)
        self.trim = int(b)
        self.calls.append(("trim", int(b)))

    def set_clip_norm(self, c):
        self.clip = float(c) or None

    def _finish(self, mode, diffs):
        if mode != TRIMMED_MEAN:
            return super()._finish(mode, diffs)
        if not self.trim:
            raise AggregationError("PGH_TRIMMED_MEAN with trimming off", status=-3)
        if self.ckpt is None:
            raise AggregationError("no resident checkpoint")
        if len(diffs) < 2 * self.trim + 1:
            raise AggregationError("too few diffs", status=-3)
        self.ckpt = TO.fedavg_trimmed(self.ckpt, diffs, self.trim)


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]
B = 2


def ckpt_tensors(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


def diff_tensors(w, version=0):
    rng = np.random.default_rng([version, w])
    t = [rng.standard_normal(s).astype(F) for s in SHAPES]
    if w in (0, 5):
        t[0][0, 0], t[2][3] = np.nan, F(1e30)  # the two hostile workers
    return t


def check_close(new_pb, ckpt, order, latest, inc):
    want = TO.fedavg_trimmed_tensors(ckpt, [latest[w] for w in order], B)
    for g, w in zip(parse_state(new_pb), want):
        assert TO.same_bits(g, w)
        assert np.isfinite(g).all()
    assert inc.last_close["n"] == len(order) and inc.last_close["trim"] == B


def drive(n, arrivals, slots, fold_batch=2, db_order=None):
    eng = TrimEngine()
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    inc = IncrementalCycle(eng, NUMEL, slots=slots, fold_batch=fold_batch, checkpoint=ck_pb, trim_count=B)
    assert ("trim", B) in eng.calls and not any(c[0] == "ingest" for c in eng.calls)
    for w in range(n):
        inc.assigned(w, key=w)
    latest, db = {}, {}
    for w, version in arrivals:
        latest[w] = diff_tensors(w, version)
        db[w] = build_state_fast(latest[w])
        inc.reported(w, db[w])
    order = [w for w in (db_order if db_order is not None else range(n)) if w in latest]
    new = inc.close(ck_pb, framing="template", order=order, fetch=db.__getitem__)
    check_close(new, ckpt, order, latest, inc)
    return inc, eng


def test_incremental_shuffled_reports_with_dropouts():
    rng = np.random.default_rng(20)
    reporters = [w for w in range(1, 30) if rng.random() >= 0.2]
    rng.shuffle(reporters)
    inc, _ = drive(30, [(w, 0) for w in reporters], slots=32)
    assert inc.last_close["early"] == 0 and not inc.last_close["refold"]


def test_incremental_early_folds_stay_as_they_are():
    order = list(np.random.default_rng(21).permutation(12))
    inc, eng = drive(12, [(int(w), 0) for w in order], slots=3, fold_batch=1)
    assert inc.last_close["early"] > 0 and any(c[0] == "fold" for c in eng.calls)


def test_incremental_re_report_restarts():
    inc, eng = drive(8, [(0, 0), (1, 0), (0, 1), (3, 0), (2, 0), (4, 0), (5, 0)], slots=8, fold_batch=1)
    assert inc.last_close["refold"] and ("restart",) in eng.calls
    inc, eng = drive(8, [(w, 0) for w in (0, 1, 2, 3, 5, 4, 7)], slots=8, fold_batch=2, db_order=[2, 0, 1, 3, 7, 5, 4, 6])
    assert inc.last_close["refold"]


def test_incremental_close_with_too_few_diffs_fails_closed():
    eng = TrimEngine()
    ck_pb = build_state_fast(ckpt_tensors())
    inc = IncrementalCycle(eng, NUMEL, slots=8, checkpoint=ck_pb, trim_count=B)
    for w in range(6):
        inc.assigned(w)
    for w in range(4):  # N = 2b
        inc.reported(w, build_state_fast(diff_tensors(w)))
    with pytest.raises(TrimUnavailableError):
        inc.close(ck_pb, framing="template")
    assert not any(c[0] == "finish" for c in eng.calls)


def test_incremental_constructor_refusals_and_clearing():
    with pytest.raises(TrimUnavailableError):
        IncrementalCycle(NumpyEngine(), NUMEL, slots=4, trim_count=1)  # an engine that cannot trim
    with pytest.raises(TrimUnavailableError):
        IncrementalCycle(TrimEngine(), NUMEL, slots=4, trim_count=1, mode=ITERATIVE_MEAN)
    with pytest.raises(TrimUnavailableError):
        IncrementalCycle(TrimEngine(), NUMEL, slots=4, trim_count=1, clip_norm=1.0)
    with pytest.raises(TrimUnavailableError):
        IncrementalCycle(TrimEngine(), NUMEL, slots=4, trim_count=1, weights_by_worker={0: 1.0})
    with pytest.raises(AggregationError):
        IncrementalCycle(TrimEngine(), NUMEL, slots=4, trim_count=9)
    shared = TrimEngine()
    IncrementalCycle(shared, NUMEL, slots=4, trim_count=3).abandon()
    assert shared.trim == 3
    IncrementalCycle(shared, NUMEL, slots=4)  # the next FL process has no trim count: cleared
    assert shared.trim == 0
    # without the key an engine that has no set_trim is never asked
    eng = NumpyEngine()
    inc = IncrementalCycle(eng, NUMEL, slots=4, checkpoint=build_state_fast(ckpt_tensors()))
    for w in range(3):
        inc.assigned(w)
        inc.reported(w, build_state_fast(diff_tensors(w + 1)))
    new = inc.close(build_state_fast(ckpt_tensors()), framing="template")
    want = O.fedavg_mean(ckpt_tensors(), [diff_tensors(w + 1) for w in range(3)])
    assert all(np.array_equal(u32(g), u32(w)) for g, w in zip(parse_state(new), want))
    assert inc.last_close["trim"] is None


# ---- the close-time aggregator --------------------------------------------------------------------------

def test_close_time_aggregator_trims_and_clears_the_count():
    eng = TrimEngine()
    agg = CycleAggregator(eng)
    ckpt = ckpt_tensors()
    diffs = [diff_tensors(w) for w in range(7)]
    pbs = [build_state_fast(d) for d in diffs]
    ck_pb = build_state_fast(ckpt)
    new = agg.average_plan_diffs({TRIM_KEY: B}, ck_pb, pbs, framing="template")
    want = TO.fedavg_trimmed_tensors(ckpt, diffs, B)
    assert all(TO.same_bits(g, w) for g, w in zip(parse_state(new), want))
    assert eng.calls.index(("trim", B)) < next(i for i, c in enumerate(eng.calls) if c[0] == "fedavg_resident")
    new2 = agg.average_plan_diffs({}, new, pbs[1:4], framing="template")  # the next process does not trim
    assert eng.trim == 0
    assert all(np.array_equal(u32(g), u32(w)) for g, w in zip(parse_state(new2), O.fedavg_mean(want, diffs[1:4])))
    for cfg, kw in (({TRIM_KEY: B}, {"weights": [1.0] * 7}), ({TRIM_KEY: B, "diff_clip_norm": 1.0}, {}),
                    ({TRIM_KEY: B, "iterative_plan": True}, {"avg_plan": canonical}), ({TRIM_KEY: B}, {"avg_plan": mean_plan})):
        with pytest.raises(TrimUnavailableError):
            agg.average_plan_diffs(cfg, ck_pb, pbs, framing="template", **kw)
    with pytest.raises(TrimUnavailableError):  # N = 2b
        agg.average_plan_diffs({TRIM_KEY: B}, ck_pb, pbs[:4], framing="template")
    with pytest.raises(TrimUnavailableError):
        agg.average_params({TRIM_KEY: B}, ckpt, diffs[:4])
    with pytest.raises(AggregationError):
        agg.average_plan_diffs({TRIM_KEY: 2.5}, ck_pb, pbs, framing="template")
    with pytest.raises(TrimUnavailableError):  # an engine without the method
        CycleAggregator(NumpyEngine()).average_plan_diffs({TRIM_KEY: B}, ck_pb, pbs, framing="template")


def f64_state(tensors):
    from pygrid_amd.state_schema import classes

    st = classes()["State"]()
    st.ParseFromString(build_state_fast(tensors))
    td = st.tensors[0].torch_tensor.contents_data
    n = len(td.contents_float32)
    td.ClearField("contents_float32")
    td.dtype = "float64"
    td.contents_float64.extend([1.0] * n)
    return st.SerializeToString()


def test_drop_in_fails_closed_on_a_non_float32_model():
    mod = make_node()
    called = []

    def original(cm, server_config, cycle):
        called.append(cycle.id)

    drop_in = make_average_plan_diffs(CycleAggregator(TrimEngine()), mod.model_manager, mod.process_manager,
                                      mod.PlanManager, original=original, framing="template")
    for cfg, exc in (({TRIM_KEY: 1}, TrimUnavailableError), ({TRIM_KEY: 0}, AggregationError)):
        proc, _, cyc = host_process(mod, cfg, f64_state(ckpt_tensors()))
        for w in "abc":
            key = assign(mod, w + str(cfg[TRIM_KEY]), proc)
            wc = mod.cycle_manager._worker_cycles.first(request_key=key)
            wc.is_completed, wc.diff = True, build_state_fast(diff_tensors(1))
        with pytest.raises(exc):
            drop_in(mod.cycle_manager, cfg, cyc)
        assert called == []  # never the node's own, untrimmed averaging


# ---- the installed node ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("report_time", [True, False], ids=["report-time", "close-time"])
def test_installed_node_saves_the_trimmed_checkpoint(report_time):
    from pygrid_amd import node as pnode

    mod = make_node()
    node = pnode.install(mod, engine=TrimEngine(), framing="template", fold_batch=1, report_time=report_time)
    cfg = {"min_diffs": 5, "max_diffs": 5, "num_cycles": 0, "cycle_length": None, TRIM_KEY: B}
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    proc, model, _ = host_process(mod, cfg, ck_pb)
    want = ckpt
    for cycle in range(2):
        keys = {w: assign(mod, w, proc) for w in range(7)}
        for w in (3, 0, 1, 6, 5):
            mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w, cycle)))
        assert mod.cycle_manager.task_errors == []
        want = TO.fedavg_trimmed_tensors(want, [diff_tensors(w, cycle) for w in (0, 1, 3, 5, 6)], B)
        saved = mod.model_manager.load(model_id=model.id).value
        assert saved == state.serialize_model_params(ck_pb, TO.flat(want))
        assert np.isfinite(TO.flat(want)).all()  # workers 0 and 5 sent a NaN and 1e30
    assert node.stats["closes_report_time" if report_time else "closes_close_time"] == 2
    assert node.stats["closes_declined"] == 0
    node.uninstall()


@pytest.mark.parametrize("cfg_extra,plan", [({"iterative_plan": True}, b"ITERATIVE_AVG_PLAN"), ({"min_diffs": 4, "max_diffs": 4}, None)],
                         ids=["iterative-plan", "too-few-diffs"])
def test_installed_node_fails_closed(cfg_extra, plan):
    from pygrid_amd import node as pnode

    mod = make_node()
    pnode.install(mod, engine=TrimEngine(), framing="template", fold_batch=1)
    cfg = {"min_diffs": 5, "max_diffs": 5, "num_cycles": 0, "cycle_length": None, TRIM_KEY: B, **cfg_extra}
    ck_pb = build_state_fast(ckpt_tensors())
    proc, model, _ = host_process(mod, cfg, ck_pb, *([plan] if plan else []))
    keys = {w: assign(mod, w, proc) for w in range(6)}
    for w in range(cfg["max_diffs"]):
        mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w)))
    errs = mod.cycle_manager.task_errors
    assert errs and all(isinstance(e, TrimUnavailableError) for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == ck_pb  # no untrimmed checkpoint was saved
