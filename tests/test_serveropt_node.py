"""CPU: a node wired by pygrid_amd.node.install fails closed when an FL process asks for a server
optimizer that the engine cannot run (tests/fake_engine.py's NumpyEngine has no ``set_server_opt``):
no checkpoint is saved, the error reaches the cycle-close task's log, and the node's own averaging,
which applies no optimizer, is not run.  (The optimizer itself runs on the GPU: tests/test_gpu_serveropt.py.)"""
import pytest

from test_node_wiring import CFG3, Scenario

OPT = {"name": "fedadam", "lr": 0.1}


def run(server_config, **opts):
    sc = Scenario(server_config, True, **opts)
    for w in range(5):
        sc.assign(w)
    for w in (3, 0, 1):
        sc.report(w)
    return sc


@pytest.mark.parametrize("opts", [{}, {"report_time": False}])
def test_close_fails_closed_without_an_engine_that_runs_the_optimizer(opts):
    sc = run(dict(CFG3, server_optimizer=OPT), **opts)
    assert len(sc.checkpoints()) == 1, "no new checkpoint may be saved"
    assert len(sc.cm.task_errors) == 1 and "server_optimizer" in str(sc.cm.task_errors[0])


def user_mean_plan(diffs):  # a hosted non-iterative plan: user code the engine declines by default
    return [sum(p) / len(p) for p in zip(*diffs)]


@pytest.mark.parametrize("k, opts", [(0, {}), (1, {"report_time": False})])
def test_declined_plan_fails_closed_on_every_close_not_only_the_first(monkeypatch, k, opts):
    """The first close probes the plan and caches the decline; later closes meet the cached verdict
    before the aggregator is reached.  Neither may fall back to the node's own averaging."""
    from fake_node import PlanManager
    from pygrid_amd.exceptions import ServerOptUnavailableError

    plan = b"USER_MEAN_PLAN_%d" % k  # (verdicts are cached by plan bytes: a key of this test's own)
    monkeypatch.setitem(PlanManager.PLANS, plan, user_mean_plan)
    sc = Scenario(dict(CFG3, server_optimizer=OPT), True, plan=plan, **opts)
    for w in range(6):
        sc.assign(w)
    for w in (3, 0, 1, 4, 2):  # the third report closes (and fails); the cycle stays open: two more closes
        sc.report(w)
    assert len(sc.checkpoints()) == 1, "the node's own averaging ran: it applies no optimizer"
    assert len(sc.cm.task_errors) == 3
    assert all(isinstance(e, ServerOptUnavailableError) for e in sc.cm.task_errors), sc.cm.task_errors


def test_drop_in_never_calls_original_under_an_optimizer(monkeypatch):
    """``make_average_plan_diffs`` on its own (no ``install``), closed twice."""
    from fake_engine import NumpyEngine
    from fake_node import PlanManager, assign, host_process, make_node
    from pygrid_amd import cycle as pcycle
    from pygrid_amd.exceptions import ServerOptUnavailableError
    from test_node_wiring import ckpt_bytes, diff_bytes

    plan = b"USER_MEAN_PLAN_DROP_IN"
    monkeypatch.setitem(PlanManager.PLANS, plan, user_mean_plan)
    mod = make_node()
    cm, ran = mod.cycle_manager, []
    cfg = dict(CFG3, server_optimizer=OPT)
    proc, _, cyc = host_process(mod, cfg, ckpt_bytes(), plan)
    fn = pcycle.make_average_plan_diffs(pcycle.CycleAggregator(NumpyEngine()), mod.model_manager, mod.process_manager,
                                        mod.PlanManager, original=lambda *a: ran.append(a), framing="template")
    for w in range(3):
        key = assign(mod, w, proc)
        row = cm._worker_cycles.first(worker_id=w, request_key=key)
        row.is_completed, row.diff = True, diff_bytes(w)
    for _ in range(2):
        with pytest.raises(ServerOptUnavailableError):
            fn(cm, cfg, cyc)
    assert ran == [] and len(mod.model_manager._model_checkpoints.rows) == 1


def test_malformed_setting_fails_the_close():
    sc = run(dict(CFG3, server_optimizer={"name": "fedadam"}))  # no lr
    assert len(sc.checkpoints()) == 1
    assert len(sc.cm.task_errors) == 1 and "lr" in str(sc.cm.task_errors[0])


def test_without_the_key_nothing_changes():
    sc = run(dict(CFG3, server_optimizer=None))
    assert len(sc.checkpoints()) == 2 and sc.cm.task_errors == []
