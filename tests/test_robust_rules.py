"""CPU: the three robust-aggregation rules of the host layer -- ``diff_clip_norm``, ``diff_trim_count``,
``diff_median`` -- fail closed the same way at every site.  Where the engine cannot apply a cycle's
rule the caller gets the rule's own error (never a ``PlanNotAcceleratedError``, on which it would fall
back to the node's undefended averaging), naming the config key, with the engine's verdict as its
``__cause__`` where there is one.  One parametrised table instead of three copies, so that a fourth
rule gets every cell by adding a row.

Covered elsewhere and not repeated here: the values each key accepts (``test_clip_norm_of``,
``test_trim_count_of``, ``test_median_of``), the arithmetic and the engine-call order of a close
that succeeds (``test_close_time_aggregator_*``, the ``test_incremental_*`` of each
``test_*_logic.py``), an engine without the rule's setter (``test_incremental_without_a_bound_...``,
``test_incremental_constructor_refusals_and_clearing``), too few diffs for a trim count and more
diffs than slots for a median (``test_trim_logic.py``, ``test_median_logic.py``), and the installed
node on an iterative plan (``test_installed_node_fails_closed*``)."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from fake_engine import NumpyEngine  # noqa: E402
from fake_node import PlanManager, assign, host_process, make_node  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pygrid_amd.cycle import CLIP_KEY, MEDIAN_KEY, TRIM_KEY, CycleAggregator, hosted_plan, make_average_plan_diffs, \
    select_mode  # noqa: E402
from pygrid_amd.engine import CLIPPED_MEAN, ITERATIVE_MEAN, MEAN, MEDIAN, TRIMMED_MEAN, WEIGHTED_MEAN  # noqa: E402
from pygrid_amd.exceptions import AggregationError, ClipUnavailableError, MedianUnavailableError, \
    ModelNotAcceleratedError, PlanNotAcceleratedError, TrimUnavailableError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402

F = np.float32
R = namedtuple("R", "key value arg error mode")
CLIP = R(CLIP_KEY, 1.0, "clip_norm", ClipUnavailableError, CLIPPED_MEAN)
TRIM = R(TRIM_KEY, 2, "trim_count", TrimUnavailableError, TRIMMED_MEAN)
MED = R(MEDIAN_KEY, True, "median", MedianUnavailableError, MEDIAN)
rules = pytest.mark.parametrize("r", [CLIP, TRIM, MED], ids=["clip", "trim", "median"])
BAD = {CLIP_KEY: -1.0, TRIM_KEY: 0, MEDIAN_KEY: "yes"}
# (the rules set together, the one whose error refuses the combination): median > trim > clip
COMBOS = [((MED, CLIP), MED), ((MED, TRIM), MED), ((TRIM, CLIP), TRIM), ((MED, TRIM, CLIP), MED)]
combos = pytest.mark.parametrize("together,winner", COMBOS, ids=["median+clip", "median+trim", "trim+clip", "all"])


def cfg_of(*rs, **extra):
    return {**{r.key: r.value for r in rs}, **extra}


def kw_of(*rs):
    return {r.arg: r.value for r in rs}


def refused(excinfo, r, cause=None):
    e = excinfo.value
    assert type(e) is r.error and not isinstance(e, PlanNotAcceleratedError)
    assert r.key in str(e)  # the message names the config key
    if cause is not None:
        assert type(e.__cause__) is cause
    return e


class AllEngine(NumpyEngine):
    """Takes every rule's setter and records it; folds as the plain NumpyEngine (these tests are
    about refusals, the arithmetic of each rule has its own file)."""

    def set_clip_norm(self, c):
        self.calls.append(("clip", float(c)))

    def set_trim(self, b):
        self.calls.append(("trim", int(b)))

    def row_sumsq(self, slots, wait=True):
        return None

    def clip_stats(self):
        return {"rows": 0, "clipped": 0, "max_norm": 0.0}

    def setters(self):
        return [c for c in self.calls if c[0] in ("clip", "trim")]


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]


def tensors(seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


def f64_state(ts):
    """Well-formed State bytes whose first tensor is float64: a model the engine does not implement."""
    from pygrid_amd.state_schema import classes

    st = classes()["State"]()
    st.ParseFromString(build_state_fast(ts))
    td = st.tensors[0].torch_tensor.contents_data
    n = len(td.contents_float32)
    td.ClearField("contents_float32")
    td.dtype = "float64"
    td.contents_float64.extend([1.0] * n)
    return st.SerializeToString()


CK = build_state_fast(tensors(0))
PBS = [build_state_fast(tensors(w + 1)) for w in range(5)]  # 5 = 2 b + 1 diffs: enough for TRIM


def canonical(avg, item, num):
    return [(a * num + i) / (num + 1) for a, i in zip(avg, item)]


def mean_plan(diffs):
    import torch as th
    from functools import reduce

    return [th.div(reduce(th.add, [d[j] for d in diffs]), len(diffs)) for j in range(len(diffs[0]))]


def other_plan(diffs):
    return [sum(d[j] for d in diffs) * 0.5 for j in range(len(diffs[0]))]


def never_called(*_a, **_k):
    raise AssertionError("a plan whose verdict is cached was run again")


# ---- select_mode ------------------------------------------------------------------------------------------

@rules
def test_select_mode_gives_the_rules_mode_or_the_rules_error(r):
    kw = kw_of(r)
    assert select_mode({}, **kw) == r.mode
    assert select_mode({}, mean_plan, mean_plans="probe", **kw) == r.mode
    with pytest.raises(AggregationError) as e:
        select_mode({}, weights=[1.0, 2.0], **kw)
    refused(e, r)
    with pytest.raises(AggregationError) as e:
        select_mode({"iterative_plan": True}, canonical, **kw)
    refused(e, r)
    with pytest.raises(AggregationError) as e:
        select_mode({}, mean_plan, **kw)  # declined: non-iterative plans are user code by default
    refused(e, r, cause=PlanNotAcceleratedError)
    with pytest.raises(AggregationError) as e:
        select_mode({}, other_plan, mean_plans="probe", **kw)
    refused(e, r, cause=PlanNotAcceleratedError)


@rules
def test_a_cached_declined_verdict_is_refused_again(r):
    key = b"robust-rules-user-plan-" + r.arg.encode()
    for plan in (other_plan, never_called):
        with pytest.raises(AggregationError) as e:
            select_mode({}, plan, plan_key=key, **kw_of(r))
        first = refused(e, r, cause=PlanNotAcceleratedError)
    assert str(first.__cause__) in str(first)  # the verdict is passed on
    # the node's lookup of such a plan raises the cached verdict itself (no rule involved) ...
    mod = make_node()
    called = []
    cfg = cfg_of(r)
    proc, model, cyc = host_process(mod, cfg, CK, key)
    with pytest.raises(PlanNotAcceleratedError):
        hosted_plan(cfg, cyc, mod.process_manager, mod.PlanManager)
    # ... and the drop-in close turns it into the rule's error: never the node's own averaging
    drop_in = make_average_plan_diffs(CycleAggregator(AllEngine()), mod.model_manager, mod.process_manager,
                                      mod.PlanManager, original=lambda *a: called.append(a), framing="template")
    assert key not in PlanManager.PLANS  # (deserializing it would raise KeyError: the verdict came from the cache)
    with pytest.raises(AggregationError) as e:
        drop_in(mod.cycle_manager, cfg, cyc)
    refused(e, r, cause=PlanNotAcceleratedError)
    assert called == [] and mod.model_manager.load(model_id=model.id).value == CK


# ---- the close-time aggregator ----------------------------------------------------------------------------

@rules
@pytest.mark.parametrize("how", ["config", "argument"])
def test_average_plan_diffs_refuses_a_non_float32_model(r, how):
    agg = CycleAggregator(AllEngine())
    cfg, kw = (cfg_of(r), {}) if how == "config" else ({}, kw_of(r))
    with pytest.raises(AggregationError) as e:
        agg.average_plan_diffs(cfg, f64_state(tensors(0)), PBS, framing="template", **kw)
    refused(e, r, cause=ModelNotAcceleratedError)
    with pytest.raises(AggregationError) as e:
        agg.average_plan_diffs(cfg, CK, PBS[:2] + [f64_state(tensors(3))] + PBS[3:], framing="template", **kw)
    refused(e, r, cause=ModelNotAcceleratedError)


@rules
def test_an_explicit_argument_overrides_the_config(r):
    """``None`` (``False`` for the median) turns a configured rule off; a value turns it on."""
    eng = AllEngine()
    agg = CycleAggregator(eng)
    new = agg.average_plan_diffs(cfg_of(r), CK, PBS, framing="template", **{r.arg: None})
    want = O.fedavg_mean(tensors(0), [tensors(w + 1) for w in range(5)])
    assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(parse_state(new), want))
    assert eng.setters() == [("clip", 0.0), ("trim", 0)]
    if r is MED:
        agg.average_plan_diffs(cfg_of(r), CK, PBS, framing="template", median=False)
        assert eng.setters() == [("clip", 0.0), ("trim", 0)] * 2
    with pytest.raises(AggregationError) as e:  # on: the rule's refusal of weights shows it
        agg.average_plan_diffs({}, CK, PBS, framing="template", weights=[1.0] * 5, **kw_of(r))
    refused(e, r)
    with pytest.raises(AggregationError) as e:  # a malformed explicit value is malformed
        agg.average_plan_diffs({}, CK, PBS, framing="template", **{r.arg: BAD[r.key]})
    assert type(e.value) is AggregationError


@pytest.mark.parametrize("r", [None, CLIP, TRIM, MED], ids=["none", "clip", "trim", "median"])
def test_the_engine_gets_the_rules_value_and_the_others_cleared(r):
    """Before the first ingest, bound first, then the trim count: a shared engine carries nothing over."""
    want = [("clip", r.value if r is CLIP else 0.0), ("trim", r.value if r is TRIM else 0)]
    eng = AllEngine()
    CycleAggregator(eng).average_plan_diffs(cfg_of(*([r] if r else [])), CK, PBS, framing="template")
    assert eng.setters() == want
    assert eng.calls.index(want[1]) < next(i for i, c in enumerate(eng.calls) if c[0] == "ingest")
    eng = AllEngine()
    IncrementalCycle(eng, NUMEL, slots=8, checkpoint=CK, **(kw_of(r) if r else {}))
    assert eng.setters() == want and not any(c[0] == "ingest" for c in eng.calls)


def test_a_bound_the_engine_reports_unsupported_is_the_rules_error():
    class Group(AllEngine):
        def set_clip_norm(self, c):
            if c:
                raise AggregationError("a group engine does not clip", status=-6)

    with pytest.raises(AggregationError) as e:
        CycleAggregator(Group()).average_plan_diffs(cfg_of(CLIP), CK, PBS, framing="template")
    refused(e, CLIP, cause=AggregationError)
    CycleAggregator(Group()).average_plan_diffs({}, CK, PBS, framing="template")  # clearing it is fine


# ---- IncrementalCycle ---------------------------------------------------------------------------------------

@rules
def test_incremental_cycle_declined_by_a_non_float32_report_fails_closed_at_the_seal(r):
    eng = AllEngine()
    inc = IncrementalCycle(eng, NUMEL, slots=8, checkpoint=CK, **kw_of(r))
    assert (inc.clip_norm, inc.trim_count, inc.median) == (CLIP.value if r is CLIP else None,
                                                           TRIM.value if r is TRIM else None, r is MED)
    for w in range(3):
        inc.assigned(w)
    inc.reported(0, PBS[0])
    inc.reported(1, f64_state(tensors(2)))  # accepted: the reference would average it
    inc.reported(2, PBS[2])
    assert inc.declined
    with pytest.raises(AggregationError) as e:
        inc.seal()
    refused(e, r)
    assert inc.declined in str(e.value)
    assert not any(c[0] in ("fold", "finish") for c in eng.calls)


@rules
def test_incremental_cycle_refuses_a_non_float32_checkpoint(r):
    with pytest.raises(AggregationError) as e:
        IncrementalCycle(AllEngine(), NUMEL, slots=8, checkpoint=f64_state(tensors(0)), **kw_of(r))
    refused(e, r, cause=ModelNotAcceleratedError)


@rules
@pytest.mark.parametrize("kw", [{"mode": ITERATIVE_MEAN}, {"weights_by_worker": {0: 1.0}},
                                {"mode": WEIGHTED_MEAN, "weights_by_worker": {0: 1.0}}],
                         ids=["iterative", "weights", "weighted-mode"])
def test_incremental_cycle_refuses_another_mode_or_weights(r, kw):
    with pytest.raises(AggregationError) as e:
        IncrementalCycle(AllEngine(), NUMEL, slots=8, **kw_of(r), **kw)
    refused(e, r)


# ---- combinations: median > trim > clip, refused with the winner's error --------------------------------------

@combos
def test_combinations_are_refused_with_the_winners_error(together, winner):
    with pytest.raises(AggregationError) as e:
        select_mode({}, **kw_of(*together))
    refused(e, winner)
    with pytest.raises(AggregationError) as e:
        IncrementalCycle(AllEngine(), NUMEL, slots=8, **kw_of(*together))
    refused(e, winner)
    agg = CycleAggregator(AllEngine())
    for cfg, kw in ((cfg_of(*together), {}), ({}, kw_of(*together)), (cfg_of(together[0]), kw_of(*together[1:]))):
        with pytest.raises(AggregationError) as e:
            agg.average_plan_diffs(cfg, CK, PBS, framing="template", **kw)
        refused(e, winner)
        with pytest.raises(AggregationError) as e:
            agg.average_params(cfg, tensors(0), [tensors(w + 1) for w in range(5)], **kw)
        refused(e, winner)


@pytest.mark.parametrize("good,bad", [(MED, TRIM), (MED, CLIP), (TRIM, CLIP)],
                         ids=["median+trim", "median+clip", "trim+clip"])
def test_a_malformed_value_beside_a_winning_rule_is_still_malformed(good, bad):
    cfg = cfg_of(good, **{bad.key: BAD[bad.key]})
    agg = CycleAggregator(AllEngine())
    with pytest.raises(AggregationError) as e:
        agg.average_plan_diffs(cfg, CK, PBS, framing="template")
    assert type(e.value) is AggregationError and bad.key in str(e.value)
    with pytest.raises(AggregationError) as e:
        agg.average_params(cfg, tensors(0), [tensors(w + 1) for w in range(5)])
    assert type(e.value) is AggregationError
    mod = make_node()
    called = []
    drop_in = make_average_plan_diffs(agg, mod.model_manager, mod.process_manager, mod.PlanManager,
                                      original=lambda *a: called.append(a), framing="template")
    proc, model, cyc = host_process(mod, cfg, CK)
    with pytest.raises(AggregationError) as e:
        drop_in(mod.cycle_manager, cfg, cyc)
    assert type(e.value) is AggregationError and called == []


# ---- without a rule nothing changes ----------------------------------------------------------------------------

def test_without_a_rule_every_verdict_and_decline_is_what_it_was():
    assert select_mode({}) == MEAN and select_mode({}, clip_norm=None, trim_count=None, median=False) == MEAN
    assert select_mode({}, mean_plan, mean_plans="probe") == MEAN
    assert select_mode({"iterative_plan": True}, canonical) == ITERATIVE_MEAN
    assert select_mode({}, weights=[1.0]) == WEIGHTED_MEAN
    key = b"robust-rules-user-plan-no-rule"
    for plan, policy, pk in ((mean_plan, None, None), (other_plan, "probe", None), (other_plan, None, key),
                             (never_called, None, key)):
        with pytest.raises(PlanNotAcceleratedError) as e:
            select_mode({}, plan, mean_plans=policy, plan_key=pk)
        assert type(e.value) is PlanNotAcceleratedError and e.value.__cause__ is None
    agg = CycleAggregator(AllEngine())
    for ck, pbs in ((f64_state(tensors(0)), PBS), (CK, PBS[:1] + [f64_state(tensors(2))])):
        with pytest.raises(PlanNotAcceleratedError) as e:
            agg.average_plan_diffs({}, ck, pbs, framing="template")
        assert type(e.value) is ModelNotAcceleratedError
    with pytest.raises(PlanNotAcceleratedError):
        agg.average_params({}, tensors(0), [tensors(1)], avg_plan=mean_plan)
    with pytest.raises(ModelNotAcceleratedError):
        IncrementalCycle(AllEngine(), NUMEL, slots=8, checkpoint=f64_state(tensors(0)))
    inc = IncrementalCycle(AllEngine(), NUMEL, slots=8, checkpoint=CK)
    inc.assigned(0)
    inc.reported(0, f64_state(tensors(1)))
    with pytest.raises(PlanNotAcceleratedError) as e:
        inc.seal()
    assert type(e.value) is ModelNotAcceleratedError and str(e.value) == inc.declined
    # the drop-in close hands such cycles to the node's own averaging: a cached declined plan, a float64 model
    mod = make_node()
    called = []
    drop_in = make_average_plan_diffs(agg, mod.model_manager, mod.process_manager, mod.PlanManager,
                                      original=lambda cm, cfg, cyc: called.append(cyc.id), framing="template")
    for ck, plan in ((CK, key), (f64_state(tensors(0)), None)):
        proc, _, cyc = host_process(mod, {}, ck, plan)
        wc = mod.cycle_manager._worker_cycles.first(request_key=assign(mod, "w", proc))
        wc.is_completed, wc.diff = True, PBS[0]
        drop_in(mod.cycle_manager, {}, cyc)
        assert called[-1] == cyc.id
    assert len(called) == 2


# ---- the installed node ----------------------------------------------------------------------------------------

@rules
@pytest.mark.parametrize("report_time", [True, False], ids=["report-time", "close-time"])
def test_installed_node_fails_closed_on_a_non_float32_model(r, report_time):
    from pygrid_amd import node as pnode

    mod = make_node()
    node = pnode.install(mod, engine=AllEngine(), framing="template", fold_batch=1, report_time=report_time)
    cfg = cfg_of(r, min_diffs=5, max_diffs=5, num_cycles=0, cycle_length=None)
    ck = f64_state(tensors(0))
    proc, model, _ = host_process(mod, cfg, ck)
    keys = {w: assign(mod, w, proc) for w in range(6)}
    for w in range(5):
        mod.cycle_manager.submit_worker_diff(w, keys[w], PBS[w])
    errs = mod.cycle_manager.task_errors
    assert errs and all(type(e) is r.error and r.key in str(e) for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == ck  # nothing averaged another way was saved
    assert node.stats["closes_declined"] == 0
    node.uninstall()


@combos
def test_installed_node_refuses_a_combination_at_the_close(together, winner):
    from pygrid_amd import node as pnode

    mod = make_node()
    pnode.install(mod, engine=AllEngine(), framing="template", fold_batch=1)
    cfg = cfg_of(*together, min_diffs=5, max_diffs=5, num_cycles=0, cycle_length=None)
    proc, model, _ = host_process(mod, cfg, CK)
    keys = {w: assign(mod, w, proc) for w in range(6)}
    for w in range(5):
        mod.cycle_manager.submit_worker_diff(w, keys[w], PBS[w])
    errs = mod.cycle_manager.task_errors
    assert errs and all(type(e) is winner.error for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == CK


# ---- the rule table itself (the module these sites share) ---------------------------------------------------------

def robust():
    return pytest.importorskip("pygrid_amd.robust", reason="the rule table is what this file's other tests pin down")


@pytest.mark.parametrize("r", [None, CLIP, TRIM, MED], ids=["none", "clip", "trim", "median"])
def test_rule_of_resolves_the_single_active_rule(r):
    rule_of = robust().rule_of
    if r is None:
        assert rule_of({}) is None and rule_of({CLIP_KEY: None, TRIM_KEY: None, MEDIAN_KEY: False}) is None
        assert rule_of(cfg_of(CLIP, TRIM, MED), clip_norm=None, trim_count=None, median=False) is None
        return
    for got in (rule_of(cfg_of(r)), rule_of({}, **kw_of(r))):
        assert (got.key, got.value, got.mode, got.error) == (r.key, r.value, r.mode, r.error)
        assert got.lacks in ("does not clip", "does not trim", "takes no median")  # what the node's own averaging lacks
    assert rule_of(cfg_of(r), **{r.arg: None}) is None
    with pytest.raises(AttributeError):
        got.value = 3  # immutable


@combos
def test_rule_of_refuses_combinations(together, winner):
    rule_of = robust().rule_of
    for cfg, kw in ((cfg_of(*together), {}), ({}, kw_of(*together)), (cfg_of(together[0]), kw_of(*together[1:]))):
        with pytest.raises(AggregationError) as e:
            rule_of(cfg, **kw)
        refused(e, winner)


def test_rule_of_parses_every_setting():
    rule_of = robust().rule_of
    for good, bad in ((MED, TRIM), (MED, CLIP), (TRIM, CLIP), (CLIP, MED), (CLIP, TRIM), (TRIM, MED)):
        for cfg, kw in ((cfg_of(good, **{bad.key: BAD[bad.key]}), {}), (cfg_of(good), {bad.arg: BAD[bad.key]})):
            with pytest.raises(AggregationError) as e:
                rule_of(cfg, **kw)
            assert type(e.value) is AggregationError and bad.key in str(e.value)


@pytest.mark.parametrize("r", [None, CLIP, TRIM, MED], ids=["none", "clip", "trim", "median"])
def test_failing_closed_converts_declines_only(r):
    rb = robust()
    rule = rb.rule_of(cfg_of(*([r] if r else [])))
    for exc in (PlanNotAcceleratedError("declined"), ModelNotAcceleratedError("float64")):
        with pytest.raises(Exception) as e:
            with rb.failing_closed(rule):
                raise exc
        if r is None:
            assert e.value is exc
        else:
            refused(e, r)
            assert e.value.__cause__ is exc and str(exc) in str(e.value)
    other = AggregationError("something else", status=-3)
    with pytest.raises(AggregationError) as e:
        with rb.failing_closed(rule):
            raise other
    assert e.value is other


def test_a_trim_count_the_engine_reports_unsupported_is_the_rules_error():
    """PGH_E_UNSUPPORTED from the setter the cycle needs is the rule's error for every rule (it used
    to be for the bound only); any other status, and a setter that is only being cleared, stay as
    they are."""
    rb = robust()

    class Group(AllEngine):
        def set_trim(self, b):
            if b:
                raise AggregationError("a group engine does not trim", status=-6)

    with pytest.raises(AggregationError) as e:
        rb.set_on_engine(Group(), rb.rule_of(cfg_of(TRIM)))
    refused(e, TRIM, cause=AggregationError)
    rb.set_on_engine(Group(), rb.rule_of(cfg_of(CLIP)))  # clearing the count is fine
    other = AllEngine()
    other.set_trim = lambda b: (_ for _ in ()).throw(AggregationError("mid-cycle", status=-3))
    with pytest.raises(AggregationError) as e:
        rb.set_on_engine(other, rb.rule_of(cfg_of(TRIM)))
    assert type(e.value) is AggregationError  # any other status stays what it is
