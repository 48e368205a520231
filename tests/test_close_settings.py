"""CPU: what a cycle can ask for at its close -- a rule (``diff_clip_norm``, ``diff_trim_count``,
``diff_median``), a server optimizer, DP noise beside the clip bound -- and what the host layer makes
of every valid combination, as one table.  Rows: {none, clip, trim, median} x {optimizer or not} x
{noise or not}, noise only beside clip.  Per row: which exception class leaves a fail-closed block for
each source of a decline (``LEAVES``), what stands in for the node's own averaging, which setters the
engine sees in which order, and what ``last_close`` reports.

``LEAVES`` and ``tests/golden/close_settings.json`` (the messages, word for word, and each error's
``__cause__``) were recorded from the three nested context managers, the three stand-ins and the two
``set_on_engine`` helpers that the host layer had before ``pygrid_amd/settings.py``; the section
"what the table drives" is the only part of this file that knows which of the two it runs."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from fake_engine import NumpyEngine  # noqa: E402
from pygrid_amd.cycle import CycleAggregator  # noqa: E402
from pygrid_amd.exceptions import AggregationError, ClipUnavailableError, DpNoiseUnavailableError, \
    MedianUnavailableError, ModelNotAcceleratedError, PlanNotAcceleratedError, ServerOptUnavailableError, \
    TrimUnavailableError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.settings import CloseSettings, settings_of  # noqa: E402
from pygrid_amd.state_schema import build_state_fast  # noqa: E402

F = np.float32
RULES = {"none": {}, "clip": {"diff_clip_norm": 1.0}, "trim": {"diff_trim_count": 2}, "median": {"diff_median": True}}
OPT = {"server_optimizer": {"name": "fedadam", "lr": 0.1}}
Z, NKEY, ROUND, CYCLE = float(F(1.1)), 5, 7, 41
NOISE = {"dp_noise": {"multiplier": 1.1, "key": NKEY}}
ROWS = [r + o + n for r in RULES for o in ("", "+opt") for n in ("", "+noise") if r == "clip" or not n]
SOURCES = ("plan", "model", "rule", "other", "none")
WHAT = "the engine cannot average this cycle"  # what the aggregator's entry points say instead of the default

Plan, Model, Agg = PlanNotAcceleratedError, ModelNotAcceleratedError, AggregationError
Clip, Trim, Med = ClipUnavailableError, TrimUnavailableError, MedianUnavailableError
Opt, Dp = ServerOptUnavailableError, DpNoiseUnavailableError

# the class that leaves the block, per source of the decline: a PlanNotAcceleratedError, a
# ModelNotAcceleratedError, the rule's own refusal (no rule: no such source), an unrelated
# AggregationError, no error
LEAVES = {
    #                  plan  model  rule  other none
    "none":           (Plan, Model, None, Agg, None),
    "none+opt":       (Opt,  Opt,   None, Agg, None),
    "clip":           (Clip, Clip,  Clip, Agg, None),
    "clip+noise":     (Dp,   Dp,    Dp,   Agg, None),
    "clip+opt":       (Clip, Clip,  Clip, Agg, None),
    "clip+opt+noise": (Dp,   Dp,    Dp,   Agg, None),
    "trim":           (Trim, Trim,  Trim, Agg, None),
    "trim+opt":       (Trim, Trim,  Trim, Agg, None),
    "median":         (Med,  Med,   Med,  Agg, None),
    "median+opt":     (Med,  Med,   Med,  Agg, None),
}

# the class that the stand-in for the node's own averaging raises (none: there is no stand-in)
STAND_IN = {"none": None, "none+opt": Opt, "clip": Clip, "clip+noise": Dp, "clip+opt": Clip, "clip+opt+noise": Dp,
            "trim": Trim, "trim+opt": Trim, "median": Med, "median+opt": Med}

# the rule and noise setters the engine sees before a cycle's first ingest: the bound, the trim count, the noise
_OFF = ("noise", 0.0, 0, 0)
SETTERS = {
    "none":           [("clip", 0.0), ("trim", 0), _OFF],
    "none+opt":       [("clip", 0.0), ("trim", 0), _OFF],
    "clip":           [("clip", 1.0), ("trim", 0), _OFF],
    "clip+noise":     [("clip", 1.0), ("trim", 0), ("noise", Z, NKEY, ROUND)],
    "clip+opt":       [("clip", 1.0), ("trim", 0), _OFF],
    "clip+opt+noise": [("clip", 1.0), ("trim", 0), ("noise", Z, NKEY, ROUND)],
    "trim":           [("clip", 0.0), ("trim", 2), _OFF],
    "trim+opt":       [("clip", 0.0), ("trim", 2), _OFF],
    "median":         [("clip", 0.0), ("trim", 0), _OFF],
    "median+opt":     [("clip", 0.0), ("trim", 0), _OFF],
}

# the rule, noise (and here: fold) entries of last_close
CLOSE_KEYS = {"clipped", "max_norm", "trim", "median", "noise_multiplier", "noise_std"}
FOLD_KEYS = {"from_hbm", "from_host", "from_db", "refold", "reason", "early", "n", "folded_before_close"}


def config(row):
    rule, *mods = row.split("+")
    return {**RULES[rule], **(OPT if "opt" in mods else {}), **(NOISE if "noise" in mods else {})}


def parsed(row):
    return settings_of(config(row))


# ---- what the table drives ------------------------------------------------------------------------------------

def fail_closed(row, what=None):
    return parsed(row).fail_closed(what) if what else parsed(row).fail_closed()


def stand_in(row, cycle_id):
    return parsed(row).refusing_original(cycle_id)


def put_on_engine(row, engine, key, rnd):
    parsed(row).set_on_engine(engine, key, rnd)


def is_set(row):
    return bool(parsed(row))


# ---- the table --------------------------------------------------------------------------------------------------

def leaving(row, source, what=None):
    """(class, message, classes along the ``__cause__`` chain) of what leaves a fail-closed block in which
    ``source`` is raised.  The chain ends at the error that was raised."""
    rule = parsed(row).rule
    raised = {"plan": PlanNotAcceleratedError("the plan is user code"),
              "model": ModelNotAcceleratedError("the checkpoint holds non-float32 tensors"),
              "rule": rule.refuse("is set but the engine cannot apply it") if rule else None,
              "other": AggregationError("something else", status=-3), "none": None}[source]
    try:
        with fail_closed(row, what):
            if raised is not None:
                raise raised
    except Exception as e:  # noqa: BLE001 -- whatever leaves is the observation
        chain, last = [], e
        while last.__cause__ is not None:
            last = last.__cause__
            chain.append(type(last).__name__)
        assert last is raised
        return type(e), str(e), chain
    return None, None, []


def observed(row):
    """Everything recorded per row, as it goes into the golden file."""
    cells = {}
    for source in SOURCES:
        if source == "rule" and parsed(row).rule is None:
            continue
        cls, msg, cause = leaving(row, source)
        cells[source] = {"class": cls.__name__ if cls else None, "message": msg, "causes": cause,
                         "message_what": leaving(row, source, WHAT)[1]}
    original = stand_in(row, CYCLE)
    refusal = None
    if original is not None:
        with pytest.raises(AggregationError) as e:
            original("cm", {}, "cycle")
        refusal = {"class": type(e.value).__name__, "message": str(e.value)}
    return {"leaves": cells, "stand_in": refusal}


@pytest.fixture(scope="module")
def recorded(gold):
    return json.loads((gold / "close_settings.json").read_text())


def test_the_rows_are_every_valid_combination(recorded):
    assert len(ROWS) == 10 and set(ROWS) == set(LEAVES) == set(STAND_IN) == set(SETTERS) == set(recorded)
    assert not any("noise" in r and not r.startswith("clip") for r in ROWS)
    assert [is_set(r) for r in ROWS] == [r != "none" for r in ROWS]


@pytest.mark.parametrize("row", ROWS)
def test_what_leaves_a_fail_closed_block(row, recorded):
    for source, want in zip(SOURCES, LEAVES[row]):
        if source == "rule" and parsed(row).rule is None:
            assert want is None
            continue
        assert leaving(row, source)[0] is want, (row, source)
        if want is not None:
            assert not issubclass(want, PlanNotAcceleratedError) or row == "none"  # set: nothing falls back
    assert observed(row)["leaves"] == recorded[row]["leaves"]  # the messages and causes, word for word


@pytest.mark.parametrize("row", ROWS)
def test_what_stands_in_for_the_nodes_own_averaging(row, recorded):
    original = stand_in(row, CYCLE)
    if STAND_IN[row] is None:
        assert original is None and recorded[row]["stand_in"] is None
        return
    with pytest.raises(AggregationError) as e:
        original("cm", {}, "cycle")
    assert type(e.value) is STAND_IN[row] and str(CYCLE) in str(e.value)
    assert {"class": type(e.value).__name__, "message": str(e.value)} == recorded[row]["stand_in"]


class Recorder(NumpyEngine):
    """Records every setter; folds every mode as the plain mean (the arithmetic has its own files)."""

    def set_clip_norm(self, c):
        self.calls.append(("clip", float(c)))

    def set_trim(self, b):
        self.calls.append(("trim", int(b)))

    def set_dp_noise(self, z, key=0, rnd=0):
        self.z = float(F(z))
        self.calls.append(("noise", self.z, int(key), int(rnd)))

    def set_server_opt(self, kind, *args):
        self.calls.append(("opt", int(kind)))

    def server_opt_state(self):
        return np.zeros(self.P, F), np.zeros(self.P, F)

    def load_server_opt_state(self, m, v):
        self.calls.append(("opt_state",))

    def server_opt_commit(self):
        self.calls.append(("commit",))

    def row_sumsq(self, slots, wait=True):
        return None

    def clip_stats(self):
        return {"rows": 5, "clipped": 2, "max_norm": 3.5}

    def dp_stats(self):
        return {"multiplier": self.z, "sigma": 0.25, "n": 5}

    def _finish(self, mode, diffs):
        super()._finish(0, diffs)

    def setters(self):
        return [c for c in self.calls if c[0] in ("clip", "trim", "noise")]


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]


def tensors(seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


CK = build_state_fast(tensors(0))
PBS = [build_state_fast(tensors(w + 1)) for w in range(5)]  # 5 = 2 b + 1 diffs: enough for the trim count


def cycle_kwargs(row):
    st = parsed(row)
    kw = {} if st.rule is None else {st.rule.arg: st.rule.value}
    if st.opt is not None:
        kw.update(server_opt=st.opt, opt_key="proc")
    if st.noise is not None:
        kw.update(dp_noise=config(row)["dp_noise"], dp_round=ROUND)
    return kw


@pytest.mark.parametrize("row", ROWS)
def test_the_setters_the_engine_sees(row):
    eng = Recorder()
    put_on_engine(row, eng, NKEY, ROUND)
    assert eng.calls == SETTERS[row]
    # the same calls, before the first ingest, from both users of an engine
    eng = Recorder()
    CycleAggregator(eng).average_plan_diffs(config(row), CK, PBS, framing="template", opt_key="proc", dp_round=ROUND)
    first_ingest = next(i for i, c in enumerate(eng.calls) if c[0] == "ingest")
    assert eng.setters() == SETTERS[row] and eng.calls.index(SETTERS[row][-1]) < first_ingest
    assert [c for c in eng.calls if c[0] == "commit"] == ([("commit",)] if "opt" in row else [])
    eng = Recorder()
    IncrementalCycle(eng, NUMEL, slots=8, checkpoint=CK, **cycle_kwargs(row))
    assert eng.setters() == SETTERS[row] and not any(c[0] == "ingest" for c in eng.calls)


@pytest.mark.parametrize("row", ROWS)
def test_what_last_close_reports(row):
    eng = Recorder()
    inc = IncrementalCycle(eng, NUMEL, slots=8, checkpoint=CK, **cycle_kwargs(row))
    for w in range(5):
        inc.assigned(w)
        inc.reported(w, PBS[w])
    inc.close(CK, framing="template")
    got = inc.last_close
    assert set(got) == CLOSE_KEYS | FOLD_KEYS
    rule = row.split("+")[0]
    want = {"clipped": 2, "max_norm": 3.5} if rule == "clip" else {"clipped": 0, "max_norm": None}
    want.update(trim=2 if rule == "trim" else None, median=rule == "median")
    want.update({"noise_multiplier": Z, "noise_std": 0.25} if "noise" in row else
                {"noise_multiplier": None, "noise_std": None})
    assert {k: got[k] for k in CLOSE_KEYS} == want
    assert type(got["clipped"]) is int and got["n"] == 5
    assert parsed(row).close_stats(eng) == want and list(parsed(row).close_stats(eng)) == list(want)
    if rule != "none":  # the node's log line on such a close
        message = parsed(row).close_message(CYCLE, got)
        assert message.startswith(f"cycle {CYCLE} closed with diff_") and "over 5 diffs" in message
        assert ("noise std 0.25 per parameter" in message) == ("noise" in row)


def test_incremental_cycle_takes_the_parsed_settings_or_the_keywords_not_both():
    st = parsed("clip+opt+noise")
    eng = Recorder()
    inc = IncrementalCycle(eng, NUMEL, slots=8, checkpoint=CK, settings=st, opt_key="proc", dp_round=ROUND)
    assert (inc.clip_norm, inc.trim_count, inc.median) == (1.0, None, False)
    assert eng.setters() == SETTERS["clip+opt+noise"]
    for kw in ({"clip_norm": 1.0}, {"trim_count": 2}, {"median": True}, {"server_opt": st.opt},
               {"dp_noise": NOISE["dp_noise"]}):
        with pytest.raises(AggregationError) as e:
            IncrementalCycle(Recorder(), NUMEL, slots=8, settings=st, opt_key="proc", dp_round=ROUND, **kw)
        assert type(e.value) is AggregationError and next(iter(kw)) in str(e.value)
    with pytest.raises(AggregationError):  # the optimizer's moments need the FL process's id, as before
        IncrementalCycle(Recorder(), NUMEL, slots=8, settings=st, dp_round=ROUND)
    # the optimizer as its dict or parsed; an argument overrides the config, None turns it off
    assert settings_of({}, server_opt=OPT["server_optimizer"]) == settings_of(OPT) == settings_of({}, server_opt=st.opt)
    assert settings_of(OPT, server_opt=None) == CloseSettings() and not CloseSettings()
    with pytest.raises(AggregationError):
        settings_of({}, server_opt={"name": "fedadam"})


# ---- settings that are refused before anything runs -----------------------------------------------------------

def refused_everywhere(cfg, error, kw=None):
    """The drop-in aggregator (both entry points) and, given its keywords, IncrementalCycle."""
    eng = Recorder()
    agg = CycleAggregator(eng)
    if cfg is not None:
        with pytest.raises(AggregationError) as e:
            agg.average_plan_diffs(cfg, CK, PBS, framing="template", dp_round=1, opt_key="proc")
        assert type(e.value) is error
        with pytest.raises(AggregationError) as e:
            agg.average_params(cfg, tensors(0), [tensors(w + 1) for w in range(5)], dp_round=1, opt_key="proc")
        assert type(e.value) is error
    if kw is not None:
        with pytest.raises(AggregationError) as e:
            IncrementalCycle(eng, NUMEL, slots=8, **kw)
        assert type(e.value) is error
    assert eng.calls == []  # refused before the engine was touched
    return e.value


def test_noise_needs_the_clip_bound():
    z = {"multiplier": 1.0}
    refused_everywhere({"dp_noise": z}, Dp, {"dp_noise": z, "dp_round": 1})
    refused_everywhere({"dp_noise": z, "diff_trim_count": 1}, Dp, {"dp_noise": z, "dp_round": 1, "trim_count": 1})
    e = refused_everywhere({"dp_noise": z, "diff_median": True}, Dp, {"dp_noise": z, "dp_round": 1, "median": True})
    assert "dp_noise is set without diff_clip_norm" in str(e)
    refused_everywhere({**OPT, "dp_noise": z}, Dp)


def test_two_rules_at_once_raise_the_earlier_rules_error():
    refused_everywhere({"diff_median": True, "diff_clip_norm": 1.0}, Med, {"median": True, "clip_norm": 1.0})
    refused_everywhere({"diff_median": True, "diff_trim_count": 2}, Med, {"median": True, "trim_count": 2})
    refused_everywhere({"diff_trim_count": 2, "diff_clip_norm": 1.0, **NOISE}, Trim,
                       {"trim_count": 2, "clip_norm": 1.0, "dp_noise": NOISE["dp_noise"], "dp_round": 1})


def test_a_malformed_value_beside_a_valid_one_is_still_malformed():
    for cfg in ({"diff_median": True, "diff_clip_norm": -1.0}, {"diff_clip_norm": 1.0, "diff_trim_count": 0},
                {"diff_clip_norm": 1.0, "dp_noise": {"multiplier": 0}}, {"diff_clip_norm": 1.0, "dp_noise": 1.1},
                {"diff_clip_norm": 1.0, **NOISE, "server_optimizer": {"name": "fedadam"}},
                {"diff_trim_count": 2, "server_optimizer": {"name": "sgd", "lr": 0.1}},
                {"diff_clip_norm": "1", **NOISE, **OPT}):
        refused_everywhere(cfg, AggregationError)
    refused_everywhere(None, AggregationError, {"clip_norm": 1.0, "dp_noise": {"multiplier": -1.0}, "dp_round": 1})
    refused_everywhere(None, AggregationError, {"median": True, "trim_count": 99})


# ---- the installed node: where a declined plan is counted -----------------------------------------------------

def user_mean_plan(diffs):  # a hosted non-iterative plan: user code the engine declines by default
    return [sum(p) / len(p) for p in zip(*diffs)]


@pytest.mark.parametrize("row, counter", [("none", "closes_declined"), ("none+opt", "closes_declined"),
                                          ("clip", "closes_close_time"), ("clip+opt", "closes_close_time"),
                                          ("clip+opt+noise", "closes_close_time"), ("median", "closes_close_time")])
def test_a_declined_plan_at_the_installed_node(monkeypatch, row, counter):
    """Under an optimizer alone the report-time state is _DECLINED, as without any setting, and the
    stand-in refuses the close; under a rule or noise building that state already fails closed, and
    the close-time path refuses the cycle.  Either way no checkpoint is saved."""
    from fake_node import PlanManager
    from test_node_wiring import CFG3, Scenario

    plan = b"USER_MEAN_PLAN_SETTINGS_" + row.encode()
    monkeypatch.setitem(PlanManager.PLANS, plan, user_mean_plan)
    sc = Scenario({**CFG3, **config(row)}, True, plan=plan)
    for w in range(4):
        sc.assign(w)
    for w in (3, 0, 1):
        sc.report(w)
    stats = sc.node.stats
    assert stats[counter] == 1 and stats["closes_declined"] + stats["closes_close_time"] == 1, stats
    if row == "none":
        assert sc.cm.task_errors == [] and len(sc.checkpoints()) == 2  # the node's own averaging ran
    else:
        assert [type(e) for e in sc.cm.task_errors] == [STAND_IN[row]] and len(sc.checkpoints()) == 1
