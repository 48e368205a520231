"""CPU: the coordinate-wise median -- the oracle's pins (tests/median_oracle.py against a plain sort,
``np.median`` and the golden file), the robustness property, and the host logic that drives the
engine: ``median_of``, ``select_mode``, fail-closed closes, ``IncrementalCycle(median=True)`` and
the installed node over a numpy engine that takes the median with the oracle."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_median_golden as GG  # noqa: E402
import median_oracle as MO  # noqa: E402
from fake_engine import NumpyEngine  # noqa: E402
from fake_node import assign, host_process, make_node  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pygrid_amd import state  # noqa: E402
from pygrid_amd.cycle import MEDIAN_KEY, CycleAggregator, make_average_plan_diffs, median_of, select_mode  # noqa: E402
from pygrid_amd.engine import ITERATIVE_MEAN, MEAN, MEDIAN, MODE_NAMES, WEIGHTED_MEAN  # noqa: E402
from pygrid_amd.exceptions import AggregationError, MedianUnavailableError, PlanNotAcceleratedError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402

F = np.float32


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GG.GOLDEN)


def sort_median(col):
    """One column by a plain Python sort of (sign-aware) integer keys."""
    bits = [int(b) for b in u32(col)]
    keys = sorted((b ^ 0xFFFFFFFF) if b >> 31 else (b | 0x80000000) for b in bits)  # unsigned order
    back = [np.array([(k ^ 0xFFFFFFFF) if not k >> 31 else (k & 0x7FFFFFFF)], np.uint32).view(F)[0] for k in keys]
    n = len(back)
    if n & 1:
        return back[(n - 1) // 2]
    with np.errstate(all="ignore"):
        return F(F(0.5) * back[n // 2 - 1]) + F(F(0.5) * back[n // 2])


# ---- the oracle ----------------------------------------------------------------------------------

def test_oracle_matches_the_golden_file(G):
    assert list(G["cases"]) == list(GG.CASES)
    for n in GG.CASES:
        ckpt, d = GG.case_inputs(n)
        assert np.array_equal(u32(d), u32(G[f"diffs_{n}"])) and np.array_equal(u32(ckpt), u32(G[f"ckpt_{n}"]))
        assert MO.same_bits(MO.median_of_rows(d), G[f"median_{n}"])
        assert MO.same_bits(MO.fedavg_median(ckpt, d), G[f"out_{n}"])


def test_golden_specials(G):
    for n in GG.CASES:
        m, d = G[f"median_{n}"], G[f"diffs_{n}"]
        even = n % 2 == 0
        assert u32(m)[0] == (0x00000000 if even else 0x80000000)  # -0, +0 -> +0; a single middle -0 stays
        assert u32(m)[1] == 0
        assert u32(m)[2] == 1  # 0.5 * 1 ulp -> 0 (ties to even), 0.5 * 2 ulp = 1 ulp
        assert u32(m)[3] == (4 if even else 3)  # 0.5 * 3 ulp -> 2 ulp each (ties to even)
        assert u32(m)[4] == (0x80000002 if even else 0x80000001)
        assert u32(m)[5] == u32(F(0.25))[0]
        assert m[6] in (F(1.5), F(-2.0), F(-0.25)) and m[7] in (F(1.5), F(-0.25))
        assert m[8] == F(3e38) and m[9] == F(-3e38)  # not (a + b) / 2, which overflows
        assert np.isnan(m[10]) if even else m[10] == -np.inf
        assert m[11] == np.inf
        assert np.isfinite(m[12:15]).all() and np.abs(m[12:15]).max() < 10
        assert np.isnan(m[15]) and np.isnan(m[16])
        assert np.isfinite(m[17:]).all() if n > 2 else True
        for c in range(GG.CASE_P):
            assert MO.same_bits(m[c:c + 1], np.array([sort_median(d[:, c])], F)), (n, c)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 37, 64])
def test_oracle_against_a_plain_sort_and_numpy(n):
    p = 97
    rng = np.random.default_rng(n)
    d = rng.standard_normal((n, p)).astype(F)
    d[rng.integers(0, n, 40), rng.integers(0, p, 40)] = rng.choice(
        np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 3e38, -3e38, 1e-45, -1e-45], F), 40)
    m = MO.median_of_rows(d)
    assert MO.same_bits(m, np.array([sort_median(d[:, c]) for c in range(p)], F))
    assert MO.same_bits(MO.median_of_rows(d[rng.permutation(n)]), m)  # the row order does not matter
    if n & 1:
        fin = np.isfinite(d).all(axis=0)
        assert np.array_equal(m[fin], np.median(d[:, fin], axis=0))  # (np.median does not tell -0 from +0)
    ckpt = rng.standard_normal(p).astype(F)
    with np.errstate(all="ignore"):
        assert MO.same_bits(MO.fedavg_median(ckpt, d), ckpt - m)
    t = MO.fedavg_median_tensors([ckpt[:50].reshape(5, 10), ckpt[50:]], [[r[:50].reshape(5, 10), r[50:]] for r in d])
    assert t[0].shape == (5, 10) and MO.same_bits(np.concatenate([x.reshape(-1) for x in t]), MO.fedavg_median(ckpt, d))


def test_a_minority_of_hostile_rows_cannot_move_a_coordinate():
    p, honest, bad = 1001, 6, 5
    rng = np.random.default_rng(3)
    good = rng.standard_normal((honest, p)).astype(F)
    hostile = rng.choice(np.array([np.nan, -np.nan, np.inf, -np.inf, 3e38, -3e38], F), size=(bad, p))
    rows = np.concatenate([good, hostile])[rng.permutation(honest + bad)]
    ckpt = rng.standard_normal(p).astype(F)
    m = MO.median_of_rows(rows)
    assert np.isfinite(m).all() and np.all(m >= good.min(0)) and np.all(m <= good.max(0))  # a selection: no tolerance
    assert np.isfinite(MO.fedavg_median(ckpt, rows)).all()
    assert not np.isfinite(O.fedavg_mean([ckpt], [[r] for r in rows])[0]).all()


# ---- the ABI -----------------------------------------------------------------------------------------

def test_abi_and_mode_constant():
    from pygrid_amd import _lib

    assert MODE_NAMES[MEDIAN] == "median" and MEDIAN == 5
    assert _lib.load().pgh_abi_version() == 10
    header = (Path(__file__).resolve().parent.parent / "include" / "pgh_api.h").read_text()
    assert "PGH_MEDIAN = 5" in header and "#define PGH_ABI_VERSION 10" in header
    assert "#define PGH_MEDIAN_NCHIP 1024" in header


# ---- server_config["diff_median"] ----------------------------------------------------------------------

def test_median_of():
    assert MEDIAN_KEY == "diff_median"
    assert median_of({}) is False and median_of({MEDIAN_KEY: None}) is False and median_of({MEDIAN_KEY: False}) is False
    assert median_of({MEDIAN_KEY: True}) is True and median_of({MEDIAN_KEY: np.bool_(True)}) is True
    assert median_of({MEDIAN_KEY: np.bool_(False)}) is False
    for bad in (1, 0, "true", "True", 1.0, [True], np.int64(1)):
        with pytest.raises(AggregationError):
            median_of({MEDIAN_KEY: bad})


def canonical(avg, item, num):
    return [(a * num + i) / (num + 1) for a, i in zip(avg, item)]


def mean_plan(diffs):
    import torch as th
    from functools import reduce

    return [th.div(reduce(th.add, [d[j] for d in diffs]), len(diffs)) for j in range(len(diffs[0]))]


def other_plan(diffs):
    return [sum(d[j] for d in diffs) * 0.5 for j in range(len(diffs[0]))]


def test_select_mode():
    assert select_mode({}, median=True) == MEDIAN
    assert select_mode({}, mean_plan, mean_plans="probe", median=True) == MEDIAN
    refusals = (
        lambda: select_mode({"iterative_plan": True}, canonical, median=True),
        lambda: select_mode({}, weights=[1.0, 2.0], median=True),
        lambda: select_mode({}, mean_plan, median=True),  # declined: non-iterative plans are user code by default
        lambda: select_mode({}, other_plan, mean_plans="probe", median=True),
        lambda: select_mode({}, clip_norm=1.0, median=True),
        lambda: select_mode({}, trim_count=2, median=True),
    )
    for call in refusals:
        with pytest.raises(MedianUnavailableError) as e:
            call()
        assert not isinstance(e.value, PlanNotAcceleratedError)
    assert not issubclass(MedianUnavailableError, PlanNotAcceleratedError)
    assert issubclass(MedianUnavailableError, AggregationError)
    # without the switch every verdict is what it was
    assert select_mode({}) == MEAN and select_mode({}, median=False) == MEAN
    assert select_mode({"iterative_plan": True}, canonical) == ITERATIVE_MEAN
    assert select_mode({}, weights=[1.0]) == WEIGHTED_MEAN


# ---- a numpy engine that takes the median with the oracle ---------------------------------------------------

class MedianEngine(NumpyEngine):
    def __init__(self):
        super().__init__()
        self.trim = 0

    def set_trim(self, b):
        self.trim = int(b)

    def fold_slots(self, mode, slots):
        if mode == MEDIAN:
            raise AggregationError("a median needs every row at once", status=-6)
        super().fold_slots(mode, slots)

    def _finish(self, mode, diffs):
        if mode != MEDIAN:
            return super()._finish(mode, diffs)
        if self.ckpt is None:
            raise AggregationError("no resident checkpoint")
        if not diffs:
            raise AggregationError("no diffs folded")
        self.ckpt = MO.fedavg_median(self.ckpt, diffs)


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]


def ckpt_tensors(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


def diff_tensors(w, version=0):
    rng = np.random.default_rng([version, w])
    t = [rng.standard_normal(s).astype(F) for s in SHAPES]
    if w in (0, 5):
        t[0][0, 0], t[2][3] = np.nan, F(1e30)  # the two hostile workers
    return t


def drive(n, arrivals, slots, db_order=None, early_fold=True):
    eng = MedianEngine()
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    inc = IncrementalCycle(eng, NUMEL, slots=slots, fold_batch=1, checkpoint=ck_pb, median=True, early_fold=early_fold)
    for w in range(n):
        inc.assigned(w, key=w)
    latest, db = {}, {}
    for w, version in arrivals:
        latest[w] = diff_tensors(w, version)
        db[w] = build_state_fast(latest[w])
        inc.reported(w, db[w])
    order = [w for w in (db_order if db_order is not None else range(n)) if w in latest]
    return inc, eng, ckpt, ck_pb, order, latest, db


def check_close(new_pb, ckpt, order, latest, inc, eng):
    want = MO.fedavg_median_tensors(ckpt, [latest[w] for w in order])
    for g, w in zip(parse_state(new_pb), want):
        assert MO.same_bits(g, w) and np.isfinite(g).all()
    assert inc.last_close["n"] == len(order) and inc.last_close["median"] is True
    assert inc.last_close["early"] == 0 and not inc.last_close["refold"]
    assert not any(c[0] == "fold" for c in eng.calls)  # never an early fold
    assert [c for c in eng.calls if c[0] == "finish"] == [("finish", len(order))]  # one finish with every slot


@pytest.mark.parametrize("early_fold", [True, False])
def test_incremental_one_finish_with_all_slots(early_fold):
    rng = np.random.default_rng(20)
    reporters = [w for w in range(30) if rng.random() >= 0.2]
    rng.shuffle(reporters)
    inc, eng, ckpt, ck_pb, order, latest, db = drive(30, [(w, 0) for w in reporters], slots=32, early_fold=early_fold)
    assert not inc.early_fold and inc.n_parked == 0
    check_close(inc.close(ck_pb, framing="template", order=order, fetch=db.__getitem__), ckpt, order, latest, inc, eng)
    assert inc.last_close["from_hbm"] == len(order) and inc.last_close["from_db"] == 0


def test_incremental_re_report_replaces_the_slots_diff():
    arrivals = [(0, 0), (1, 0), (0, 1), (3, 0), (2, 0), (4, 0), (5, 0), (3, 2)]
    inc, eng, ckpt, ck_pb, order, latest, db = drive(8, arrivals, slots=8, db_order=[2, 0, 1, 3, 7, 5, 4, 6])
    assert inc.stale is None  # no order can be stale: the result does not depend on it
    assert len([c for c in eng.calls if c[0] == "ingest"]) == len(arrivals) and len(inc._slot_of) == 6
    assert inc.seal(order) is False  # every diff is in HBM: nothing is read through fetch
    assert inc.fetch_plan() == []
    check_close(inc.finish(ck_pb, framing="template"), ckpt, order, latest, inc, eng)


def test_incremental_every_slot_is_used_and_parked_diffs_go_to_free_slots():
    """Exactly as many reporters as slots: none parks (there is no fold front to keep a slot for).  A
    report this object never saw is read through fetch into the slot a non-reporter's diff freed."""
    inc, eng, ckpt, ck_pb, order, latest, db = drive(6, [(w, 0) for w in (4, 2, 0, 1, 3)], slots=5)
    assert inc.n_parked == 0 and len(inc._slot_of) == 5
    check_close(inc.close(ck_pb, framing="template", order=order, fetch=db.__getitem__), ckpt, order, latest, inc, eng)
    # one held diff is not in the DB's order (its row was not completed), one of the order was never seen here
    inc, eng, ckpt, ck_pb, order, latest, db = drive(6, [(w, 0) for w in (4, 2, 0, 1)], slots=4)
    latest[6] = diff_tensors(6)
    db[6] = build_state_fast(latest[6])
    order = [0, 1, 2, 6]
    assert inc.seal(order) is True and inc.fetch_plan() == [6]
    check_close(inc.finish(ck_pb, framing="template", fetch=db.__getitem__), ckpt, order, latest, inc, eng)
    assert inc.last_close["from_db"] == 1


def test_incremental_more_reporters_than_slots_fails_closed():
    inc, eng, ckpt, ck_pb, order, latest, db = drive(7, [(w, 0) for w in range(6)], slots=4)
    assert inc.n_parked == 2 and len(inc._slot_of) == 4
    held = dict(inc._slot_of)
    with pytest.raises(MedianUnavailableError):
        inc.close(ck_pb, framing="template", order=order, fetch=db.__getitem__)
    assert not any(c[0] in ("fold", "finish") for c in eng.calls)  # nothing folded ...
    assert inc._slot_of == held                                      # ... and no slot given up


def test_incremental_constructor_refusals():
    for kw in ({"mode": ITERATIVE_MEAN}, {"clip_norm": 1.0}, {"trim_count": 1}, {"weights_by_worker": {0: 1.0}},
               {"mode": WEIGHTED_MEAN, "weights_by_worker": {0: 1.0}}):
        with pytest.raises(MedianUnavailableError):
            IncrementalCycle(MedianEngine(), NUMEL, slots=4, median=True, **kw)
    # without the switch nothing changes: early folds as before, last_close says so
    eng = NumpyEngine()
    inc = IncrementalCycle(eng, NUMEL, slots=4, fold_batch=1, checkpoint=build_state_fast(ckpt_tensors()))
    for w in range(3):
        inc.assigned(w)
        inc.reported(w, build_state_fast(diff_tensors(w + 1)))
    new = inc.close(build_state_fast(ckpt_tensors()), framing="template")
    want = O.fedavg_mean(ckpt_tensors(), [diff_tensors(w + 1) for w in range(3)])
    assert all(np.array_equal(u32(g), u32(w)) for g, w in zip(parse_state(new), want))
    assert inc.last_close["median"] is False and any(c[0] == "fold" for c in eng.calls)


# ---- the close-time aggregator --------------------------------------------------------------------------

def test_close_time_aggregator():
    eng = MedianEngine()
    agg = CycleAggregator(eng)
    ckpt = ckpt_tensors()
    diffs = [diff_tensors(w) for w in range(7)]
    pbs = [build_state_fast(d) for d in diffs]
    ck_pb = build_state_fast(ckpt)
    new = agg.average_plan_diffs({MEDIAN_KEY: True}, ck_pb, pbs, framing="template")
    want = MO.fedavg_median_tensors(ckpt, diffs)
    assert all(MO.same_bits(g, w) and np.isfinite(g).all() for g, w in zip(parse_state(new), want))
    new2 = agg.average_plan_diffs({MEDIAN_KEY: False}, new, pbs[1:4], framing="template")  # the next process: the mean
    assert all(np.array_equal(u32(g), u32(w)) for g, w in zip(parse_state(new2), O.fedavg_mean(want, diffs[1:4])))
    for cfg, kw in (({MEDIAN_KEY: True}, {"weights": [1.0] * 7}), ({MEDIAN_KEY: True, "diff_clip_norm": 1.0}, {}),
                    ({MEDIAN_KEY: True, "diff_trim_count": 1}, {}),
                    ({MEDIAN_KEY: True, "iterative_plan": True}, {"avg_plan": canonical}),
                    ({MEDIAN_KEY: True}, {"avg_plan": mean_plan})):
        with pytest.raises(MedianUnavailableError):
            agg.average_plan_diffs(cfg, ck_pb, pbs, framing="template", **kw)
        with pytest.raises(MedianUnavailableError):
            agg.average_params(cfg, ckpt, diffs, **kw)
    with pytest.raises(AggregationError):
        agg.average_plan_diffs({MEDIAN_KEY: 1}, ck_pb, pbs, framing="template")


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

    drop_in = make_average_plan_diffs(CycleAggregator(MedianEngine()), mod.model_manager, mod.process_manager,
                                      mod.PlanManager, original=original, framing="template")
    for tag, cfg, exc in (("t", {MEDIAN_KEY: True}, MedianUnavailableError), ("s", {MEDIAN_KEY: "yes"}, AggregationError)):
        proc, _, cyc = host_process(mod, cfg, f64_state(ckpt_tensors()))
        for w in "abc":
            key = assign(mod, w + tag, proc)
            wc = mod.cycle_manager._worker_cycles.first(request_key=key)
            wc.is_completed, wc.diff = True, build_state_fast(diff_tensors(1))
        with pytest.raises(exc):
            drop_in(mod.cycle_manager, cfg, cyc)
        assert called == []  # never the node's own averaging, which takes no median


# ---- the installed node ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("report_time", [True, False], ids=["report-time", "close-time"])
def test_installed_node_saves_the_median_checkpoint(report_time):
    from pygrid_amd import node as pnode

    mod = make_node()
    eng = MedianEngine()
    node = pnode.install(mod, engine=eng, framing="template", fold_batch=1, report_time=report_time)
    cfg = {"min_diffs": 5, "max_diffs": 5, "num_cycles": 0, "cycle_length": None, MEDIAN_KEY: True}
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    proc, model, _ = host_process(mod, cfg, ck_pb)
    want = ckpt
    for cycle in range(2):
        keys = {w: assign(mod, w, proc) for w in range(7)}
        for w in (3, 0, 1, 6, 5):
            mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w, cycle)))
        assert mod.cycle_manager.task_errors == []
        want = MO.fedavg_median_tensors(want, [diff_tensors(w, cycle) for w in (0, 1, 3, 5, 6)])
        saved = mod.model_manager.load(model_id=model.id).value
        assert saved == state.serialize_model_params(ck_pb, MO.flat(want))
        assert np.isfinite(MO.flat(want)).all()  # workers 0 and 5 sent a NaN and 1e30
    assert node.stats["closes_report_time" if report_time else "closes_close_time"] == 2
    assert node.stats["closes_declined"] == 0
    assert not any(c[0] == "fold" for c in eng.calls)
    node.uninstall()


def test_installed_node_fails_closed_on_the_iterative_plan():
    from pygrid_amd import node as pnode

    mod = make_node()
    pnode.install(mod, engine=MedianEngine(), framing="template", fold_batch=1)
    cfg = {"min_diffs": 5, "max_diffs": 5, "num_cycles": 0, "cycle_length": None, MEDIAN_KEY: True, "iterative_plan": True}
    ck_pb = build_state_fast(ckpt_tensors())
    proc, model, _ = host_process(mod, cfg, ck_pb, b"ITERATIVE_AVG_PLAN")
    keys = {w: assign(mod, w, proc) for w in range(6)}
    for w in range(5):
        mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w)))
    errs = mod.cycle_manager.task_errors
    assert errs and all(isinstance(e, MedianUnavailableError) for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == ck_pb  # no checkpoint of another average was saved
