"""CPU: per-client L2 clipping -- the oracle's pins (tests/clip_oracle.py against exact arithmetic
and the golden file), the host half of the library (``pgh_clip_scale``, no GPU), and the host logic
that drives the engine: ``clip_norm_of``, ``select_mode``, fail-closed closes, ``IncrementalCycle``
and the installed node over a numpy engine that clips with the oracle."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import gen_clip_golden as GG  # noqa: E402
from fake_engine import NumpyEngine  # noqa: E402
from fake_node import assign, host_process, make_node  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pygrid_amd import state  # noqa: E402
from pygrid_amd.cycle import CycleAggregator, clip_norm_of, make_average_plan_diffs, select_mode  # noqa: E402
from pygrid_amd.engine import CLIPPED_MEAN, ITERATIVE_MEAN, MEAN, MODE_NAMES, WEIGHTED_MEAN  # noqa: E402
from pygrid_amd.exceptions import AggregationError, ClipUnavailableError, PlanNotAcceleratedError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402

F = np.float32


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GG.GOLDEN)


# ---- the oracle ----------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1, 3, 63, 64, 65, 1023, 4095, 4096, 4097, 8193, 70001, 311650])
def test_oracle_sumsq_is_the_exact_sum_to_1e_13(p):
    rng = np.random.default_rng(p)
    d = (rng.standard_normal(p) * 10.0 ** rng.integers(-4, 5, p)).astype(F)
    exact = math.fsum(float(x) * float(x) for x in d)  # each square is exact in f64
    assert abs(float(CO.row_sumsq(d)) - exact) <= 1e-13 * exact


def test_oracle_matches_the_golden_file(G):
    for p in G["sumsq_p"]:
        rows = G[f"rows_{p}"] if p <= GG.STORED_P_MAX else GG.mixed_rows(int(p))
        got = np.array([CO.row_sumsq(r) for r in rows]).view(np.uint64)
        assert np.array_equal(got, G[f"sumsq_bits_{p}"]), p
    s = CO.scales(G["fold_diffs"], float(G["fold_c"]))
    assert np.array_equal(u32(s), u32(G["fold_scales"]))
    assert np.array_equal(u32(CO.fold(G["fold_diffs"], s, G["fold_ckpt"])), u32(G["fold_out"]))
    assert (s == 1).sum() == 4 and (s < 1).sum() == 3
    for k, c in enumerate(G["bnd_c"]):
        assert np.array_equal(u32(CO.fedavg_clipped(G["bnd_ckpt"], G["bnd_diffs"], c)), u32(G["bnd_out"][k]))
    assert CO.same_bits(CO.fedavg_clipped(G["nf_ckpt"], G["nf_diffs"], float(G["nf_c"])), G["nf_out"])


def test_oracle_order_is_not_a_plain_sum():
    """The tree is part of the definition: on long rows it differs from a left fold in the last bit
    often enough that a kernel summing in another order cannot pass by accident."""
    rng = np.random.default_rng(3)
    differ = 0
    for _ in range(20):
        d = rng.standard_normal(70001).astype(F)
        sq = d.astype(np.float64) ** 2
        differ += CO.row_sumsq(d) != np.cumsum(sq)[-1]
    assert differ >= 5


def test_huge_bound_is_the_plain_mean(G):
    ckpt, diffs = G["fold_ckpt"], G["fold_diffs"]
    assert np.all(CO.scales(diffs, 1e30) == 1)
    want = O.fedavg_mean([ckpt], [[d] for d in diffs])[0]
    assert np.array_equal(u32(CO.fedavg_clipped(ckpt, diffs, 1e30)), u32(want))


def test_exact_boundary():
    d = np.array([3, 4], F)
    assert CO.row_sumsq(d) == 25.0
    assert CO.scale(25.0, 5.0) == 1 and u32(CO.scale(25.0, 5.0)) == u32(F(1))
    below = np.nextafter(F(5), F(0))
    s = CO.scale(25.0, below)
    assert s < 1 and u32(s) == u32(F(np.float64(below) / 5.0))


def test_inf_and_nan_rows():
    d = np.array([1, np.inf, 2], F)
    assert np.isinf(CO.row_sumsq(d)) and CO.scale(CO.row_sumsq(d), 3.0) == 0
    n = np.array([1, np.nan, 2], F)
    assert np.isnan(CO.row_sumsq(n)) and np.isnan(CO.scale(CO.row_sumsq(n), 3.0))
    out = CO.fedavg_clipped(np.zeros(3, F), [d, np.ones(3, F)], 3.0)
    assert np.isnan(out[1]) and not np.isnan(out[[0, 2]]).any()  # inf * 0 at the inf only
    assert np.isnan(CO.fedavg_clipped(np.zeros(3, F), [n, np.ones(3, F)], 3.0)).all()


# ---- pgh_clip_scale: the library's host half, no GPU ----------------------------------------------

def test_library_clip_scale_is_the_oracle():
    from pygrid_amd import Engine

    below = float(np.nextafter(F(5), F(0)))
    cases = [(25.0, 5.0), (25.0, below), (np.nextafter(25.0, 26.0), 5.0), (0.0, 1.0), (np.inf, 2.0),
             (1e300, 1e-30), (4e-320, 1e-30), (1e-300, 3e38)]
    rng = np.random.default_rng(10_000)
    ss = 10.0 ** rng.uniform(-30, 30, 10_000)
    cs = (10.0 ** rng.uniform(-12, 12, 10_000)).astype(F)
    cases += list(zip(ss, cs))
    for sumsq, c in cases:
        got, want = Engine.clip_scale(sumsq, c), CO.scale(sumsq, c)
        assert u32(got) == u32(want), (sumsq, c, got, want)
    assert np.isnan(Engine.clip_scale(float("nan"), 1.0))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(AggregationError):
            Engine.clip_scale(1.0, bad)


# ---- server_config["diff_clip_norm"] -----------------------------------------------------------------

def test_clip_norm_of():
    assert clip_norm_of({}) is None and clip_norm_of({"diff_clip_norm": None}) is None
    assert clip_norm_of({"diff_clip_norm": 2}) == 2.0 and clip_norm_of({"diff_clip_norm": F(0.5)}) == 0.5
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "1.0", True, [1.0], 1e39, 1e-60):
        with pytest.raises(AggregationError):
            clip_norm_of({"diff_clip_norm": bad})


def canonical(avg, item, num):
    return [(a * num + i) / (num + 1) for a, i in zip(avg, item)]


def mean_plan(diffs):
    import torch as th
    from functools import reduce

    return [th.div(reduce(th.add, [d[j] for d in diffs]), len(diffs)) for j in range(len(diffs[0]))]


def other_plan(diffs):
    return [sum(d[j] for d in diffs) * 0.5 for j in range(len(diffs[0]))]


def test_select_mode():
    assert MODE_NAMES[CLIPPED_MEAN] == "clipped_mean"
    assert select_mode({}, clip_norm=1.0) == CLIPPED_MEAN
    assert select_mode({}, mean_plan, mean_plans="probe", clip_norm=1.0) == CLIPPED_MEAN
    with pytest.raises(ClipUnavailableError):
        select_mode({"iterative_plan": True}, canonical, clip_norm=1.0)
    with pytest.raises(ClipUnavailableError):
        select_mode({}, weights=[1.0, 2.0], clip_norm=1.0)
    with pytest.raises(ClipUnavailableError):
        select_mode({}, mean_plan, clip_norm=1.0)  # declined: non-iterative plans are user code by default
    with pytest.raises(ClipUnavailableError):
        select_mode({}, other_plan, mean_plans="probe", clip_norm=1.0)
    assert not issubclass(ClipUnavailableError, PlanNotAcceleratedError)
    # without a bound every verdict is what it was
    assert select_mode({}) == MEAN
    assert select_mode({}, mean_plan, mean_plans="probe") == MEAN
    assert select_mode({"iterative_plan": True}, canonical) == ITERATIVE_MEAN
    assert select_mode({}, weights=[1.0]) == WEIGHTED_MEAN
    for plan, policy in ((mean_plan, None), (other_plan, "probe")):
        with pytest.raises(PlanNotAcceleratedError):
            select_mode({}, plan, mean_plans=policy)


# ---- a numpy engine that clips with the oracle ----------------------------------------------------------

class ClipEngine(NumpyEngine):
    def __init__(self):
        super().__init__()
        self.clip = None
        self._zero()

    def _zero(self):
        self.rows, self.clipped, self.max_norm = 0, 0, 0.0

    def reserve(self, n, dtype=0, parties=1):
        super().reserve(n, dtype, parties)
        self._zero()

    def reset(self):
        super().reset()
        self._zero()

    def set_clip_norm(self, c):
        self.clip = float(c) or None
        self.calls.append(("clip", float(c)))

    def row_sumsq(self, slots, wait=True):
        self.calls.append(("sumsq", tuple(int(s) for s in slots), wait))
        got = np.array([CO.row_sumsq(self.slot[int(s)]) for s in slots])  # KeyError: an empty slot
        return got if wait else None

    clip_scale = staticmethod(CO.scale)

    def clip_stats(self):
        return {"rows": self.rows, "clipped": self.clipped, "max_norm": self.max_norm}

    def _finish(self, mode, diffs):
        if mode != CLIPPED_MEAN:
            return super()._finish(mode, diffs)
        if self.clip is None:
            raise AggregationError("PGH_CLIPPED_MEAN with clipping off", status=-3)
        if self.ckpt is None or not diffs:
            raise AggregationError("nothing to fold")
        s = CO.scales(diffs, self.clip)
        self.rows += len(diffs)
        self.clipped += int((s != 1).sum())
        self.max_norm = max([self.max_norm] + [float(np.sqrt(CO.row_sumsq(d))) for d in diffs])
        self.ckpt = CO.fold(diffs, s, self.ckpt)


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]
C = 1.0


def ckpt_tensors(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


def diff_tensors(w, version=0):
    rng = np.random.default_rng([version, w])
    return [(rng.standard_normal(s) * 10.0 ** (w % 4 - 2)).astype(F) for s in SHAPES]  # norms 0.05 .. 50


def check_close(new_pb, ckpt, order, latest, inc):
    diffs = [latest[w] for w in order]
    want = CO.fedavg_clipped_tensors(ckpt, diffs, C)
    for g, w in zip(parse_state(new_pb), want):
        assert np.array_equal(u32(g), u32(w))
    s = CO.scales([CO.flat(d) for d in diffs], C)
    assert inc.last_close["clipped"] == int((s < 1).sum()) > 0
    assert inc.last_close["max_norm"] == max(float(np.sqrt(CO.row_sumsq(CO.flat(d)))) for d in diffs)
    assert inc.last_close["n"] == len(order)
    return want


def drive(n, arrivals, slots, fold_batch=2, db_order=None, never=()):
    """Workers 0 .. n-1 assigned in order; ``arrivals``: (worker, version) reports in arrival order.
    The close folds the DB's order (default: assignment order) of the workers that reported."""
    eng = ClipEngine()
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    inc = IncrementalCycle(eng, NUMEL, slots=slots, fold_batch=fold_batch, checkpoint=ck_pb, clip_norm=C)
    assert ("clip", C) in eng.calls and eng.calls.index(("clip", C)) < len(eng.calls)
    for w in range(n):
        inc.assigned(w, key=w)
    latest, db = {}, {}
    for w, version in arrivals:
        assert w not in never
        latest[w] = diff_tensors(w, version)
        db[w] = build_state_fast(latest[w])
        inc.reported(w, db[w])
    order = [w for w in (db_order if db_order is not None else range(n)) if w in latest]
    new = inc.close(ck_pb, framing="template", order=order, fetch=db.__getitem__)
    check_close(new, ckpt, order, latest, inc)
    # every diff that went into a slot had its norm pass queued right behind it, none waited for
    ingests = [c[1] for c in eng.calls if c[0] == "ingest"]
    queued = [c[1][0] for c in eng.calls if c[0] == "sumsq"]
    assert queued == ingests and all(c[2] is False for c in eng.calls if c[0] == "sumsq")
    return inc, eng


def test_incremental_shuffled_reports_with_dropouts():
    rng = np.random.default_rng(20)
    n = 30
    reporters = [w for w in range(1, n) if rng.random() >= 0.2]  # ~20 % never report, worker 0 among them
    rng.shuffle(reporters)
    inc, eng = drive(n, [(w, 0) for w in reporters], slots=32, never=(0,))
    assert inc.last_close["early"] == 0 and not inc.last_close["refold"]  # nothing is certain behind worker 0


def test_incremental_early_folds_and_slot_pressure():
    rng = np.random.default_rng(21)
    order = list(rng.permutation(12))
    inc, eng = drive(12, [(int(w), 0) for w in order], slots=3, fold_batch=1)
    assert inc.last_close["early"] > 0 and any(c[0] == "fold" for c in eng.calls)
    assert inc.last_close["from_host"] + inc.last_close["from_db"] >= 0


def test_incremental_re_report_before_and_after_its_fold():
    # worker 3 re-reports while it waits behind worker 0: the new diff replaces the old one
    inc, eng = drive(6, [(3, 0), (3, 1), (1, 0), (0, 0), (2, 0), (4, 0)], slots=8, fold_batch=1)
    assert not inc.last_close["refold"]
    # worker 0 is folded at once (fold_batch 1), then re-reports: the close re-folds from the DB
    inc, eng = drive(6, [(0, 0), (1, 0), (0, 1), (3, 0), (2, 0)], slots=8, fold_batch=1)
    assert inc.last_close["refold"] and ("restart",) in eng.calls


def test_incremental_db_order_differs_from_assignment_order():
    inc, eng = drive(8, [(w, 0) for w in (0, 1, 2, 3, 5, 4, 7)], slots=8, fold_batch=2,
                     db_order=[2, 0, 1, 3, 7, 5, 4, 6])
    assert inc.last_close["refold"]


def test_incremental_without_a_bound_never_touches_the_clip_methods():
    eng = NumpyEngine()  # has no set_clip_norm / row_sumsq / clip_stats
    ckpt = ckpt_tensors()
    inc = IncrementalCycle(eng, NUMEL, slots=4, checkpoint=build_state_fast(ckpt))
    for w in range(3):
        inc.assigned(w)
        inc.reported(w, build_state_fast(diff_tensors(w)))
    new = inc.close(build_state_fast(ckpt), framing="template")
    want = O.fedavg_mean(ckpt, [diff_tensors(w) for w in range(3)])
    for g, w in zip(parse_state(new), want):
        assert np.array_equal(u32(g), u32(w))
    assert inc.last_close["clipped"] == 0 and inc.last_close["max_norm"] is None
    with pytest.raises(ClipUnavailableError):  # a bound on an engine that cannot clip
        IncrementalCycle(NumpyEngine(), NUMEL, slots=4, clip_norm=1.0)
    with pytest.raises(ClipUnavailableError):
        IncrementalCycle(ClipEngine(), NUMEL, slots=4, clip_norm=1.0, mode=ITERATIVE_MEAN)
    shared = ClipEngine()
    IncrementalCycle(shared, NUMEL, slots=4, clip_norm=2.0).abandon()
    IncrementalCycle(shared, NUMEL, slots=4)  # the next FL process has no bound: cleared
    assert shared.clip is None


# ---- fail closed ------------------------------------------------------------------------------------------

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

    drop_in = make_average_plan_diffs(CycleAggregator(ClipEngine()), mod.model_manager, mod.process_manager,
                                      mod.PlanManager, original=original, framing="template")
    for cfg, exc in (({"diff_clip_norm": 1.0}, ClipUnavailableError), ({"diff_clip_norm": -1.0}, AggregationError)):
        proc, _, cyc = host_process(mod, cfg, f64_state(ckpt_tensors()))
        key = assign(mod, "w", proc)
        wc = mod.cycle_manager._worker_cycles.first(request_key=key)
        wc.is_completed, wc.diff = True, build_state_fast(diff_tensors(1))
        with pytest.raises(exc):
            drop_in(mod.cycle_manager, cfg, cyc)
        assert called == []  # never the node's own, unclipped averaging
    # the same model without the key is handed to the node, as before
    proc, _, cyc = host_process(mod, {}, f64_state(ckpt_tensors()))
    key = assign(mod, "v", proc)
    wc = mod.cycle_manager._worker_cycles.first(request_key=key)
    wc.is_completed, wc.diff = True, build_state_fast(diff_tensors(1))
    drop_in(mod.cycle_manager, {}, cyc)
    assert called == [cyc.id]


def test_close_time_aggregator_clips_and_clears_the_bound():
    eng = ClipEngine()
    agg = CycleAggregator(eng)
    ckpt = ckpt_tensors()
    diffs = [diff_tensors(w) for w in range(5)]
    pbs = [build_state_fast(d) for d in diffs]
    new = agg.average_plan_diffs({"diff_clip_norm": C}, build_state_fast(ckpt), pbs, framing="template")
    want = CO.fedavg_clipped_tensors(ckpt, diffs, C)
    for g, w in zip(parse_state(new), want):
        assert np.array_equal(u32(g), u32(w))
    first_ingest = next(i for i, c in enumerate(eng.calls) if c[0] == "ingest")
    assert eng.calls.index(("clip", C)) < first_ingest
    new2 = agg.average_plan_diffs({}, new, pbs, framing="template")  # the next process has no bound
    assert eng.clip is None
    for g, w in zip(parse_state(new2), O.fedavg_mean(want, diffs)):
        assert np.array_equal(u32(g), u32(w))
    with pytest.raises(ClipUnavailableError):
        agg.average_plan_diffs({"diff_clip_norm": C}, new, pbs, weights=[1.0] * 5)


# ---- the installed node ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("report_time", [True, False], ids=["report-time", "close-time"])
def test_installed_node_saves_the_clipped_checkpoint(report_time):
    from pygrid_amd import node as pnode

    mod = make_node()
    eng = ClipEngine()
    node = pnode.install(mod, engine=eng, framing="template", fold_batch=1, report_time=report_time)
    cfg = {"min_diffs": 3, "max_diffs": 3, "num_cycles": 0, "cycle_length": None, "diff_clip_norm": C}
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    proc, model, _ = host_process(mod, cfg, ck_pb)
    want = ckpt
    for cycle in range(2):
        keys = {w: assign(mod, w, proc) for w in range(5)}
        for w in (3, 0, 1):
            mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w, cycle)))
        assert mod.cycle_manager.task_errors == []
        want = CO.fedavg_clipped_tensors(want, [diff_tensors(w, cycle) for w in (0, 1, 3)], C)
        saved = mod.model_manager.load(model_id=model.id).value
        assert saved == state.serialize_model_params(ck_pb, CO.flat(want))
    assert node.stats["closes_report_time" if report_time else "closes_close_time"] == 2
    assert node.stats["closes_declined"] == 0
    node.uninstall()


def test_installed_node_fails_closed_on_an_iterative_plan():
    from pygrid_amd import node as pnode

    mod = make_node()
    pnode.install(mod, engine=ClipEngine(), framing="template", fold_batch=1)
    cfg = {"min_diffs": 2, "max_diffs": 2, "num_cycles": 0, "cycle_length": None, "iterative_plan": True,
           "diff_clip_norm": C}
    ck_pb = build_state_fast(ckpt_tensors())
    proc, model, _ = host_process(mod, cfg, ck_pb, b"ITERATIVE_AVG_PLAN")
    keys = {w: assign(mod, w, proc) for w in range(3)}
    for w in (0, 1):
        mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w)))
    errs = mod.cycle_manager.task_errors
    assert errs and all(isinstance(e, ClipUnavailableError) for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == ck_pb  # no unclipped checkpoint was saved
