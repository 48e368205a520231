"""CPU: the Multi-Krum selection -- the library's host step (pgh_krum_select_host, plain C++) against
tests/krum_oracle.py and the golden bits, the ``diff_krum`` setting, its place in ``settings.CloseSettings``, and
the close-time and report-time host logic over the numpy engine.  The GPU side: tests/test_gpu_krum.py."""
import dataclasses
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import krum_oracle as KO  # noqa: E402
import gen_krum_golden as GK  # noqa: E402
from fake_engine import NumpyEngine  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pygrid_amd.cycle import CycleAggregator  # noqa: E402
from pygrid_amd.engine import WEIGHTED_MEAN, Engine  # noqa: E402
from pygrid_amd.exceptions import AggregationError, DpNoiseUnavailableError, KrumUnavailableError, \
    ModelNotAcceleratedError, PlanNotAcceleratedError, ServerOptUnavailableError, TrimUnavailableError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.krum import KRUM_KEY, KrumSpec, krum_of  # noqa: E402
from pygrid_amd.robust import CLIP_KEY, TRIM_KEY  # noqa: E402
from pygrid_amd.settings import CloseSettings, settings_of  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402

F = np.float32
ROOT = Path(__file__).resolve().parent.parent


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def G():
    return np.load(GK.GOLDEN)


def matrix(G, key, n):
    return G[key].view(np.float64).reshape(n, n)


# ---- the definition: oracle, golden file, the library's host step -------------------------------------------

def test_oracle_matches_the_golden_file(G):
    want = GK.cases()
    assert sorted(want) == sorted(G.files)
    for k, v in want.items():
        assert np.array_equal(np.asarray(v).view(np.uint8), G[k].view(np.uint8)), k


def test_golden_pins(G):
    """What the hostile case was built to show."""
    n = 2 * GK.HOSTILE_F + 3
    assert list(G["hostile_included"]) == list(range(11)) and n == 11  # the NaN row (11) is excluded
    D = matrix(G, "hostile_D_bits", n)
    assert np.isinf(D).any() and not np.isnan(D).any() and np.array_equal(u64(D), u64(D.T))
    assert not D.diagonal().any() and not np.signbit(D.diagonal()).any()
    sc = G["hostile_score_bits"]
    assert sc[7] == sc[9]  # the 3e38 and -3e38 rows tie
    assert list(G["hostile_picked"]) == list(GK.HOSTILE_GOOD)
    assert len(G["hostile_picked_m1"]) == 1 and G["hostile_picked_m1"][0] in GK.HOSTILE_GOOD
    assert set(G["hostile_picked_m3"]) <= set(GK.HOSTILE_GOOD)


def test_host_step_matches_oracle_and_golden(G):
    for k, (n, f, m) in enumerate(GK.HOST_SHAPES):
        D = matrix(G, f"host_D_bits_{k}", n)
        picked, sc = Engine.krum_select_host(D, f, m)
        assert picked == list(G[f"host_picked_{k}"]), k
        assert np.array_equal(u64(sc), G[f"host_score_bits_{k}"]), k
        for mm in (0, 1, n - f):
            want, wsc = KO.select(D, f, mm)
            got, gsc = Engine.krum_select_host(D, f, mm)
            assert got == want and np.array_equal(u64(gsc), u64(wsc)) and len(got) == (mm or n - f)
    D = matrix(G, "hostile_D_bits", 11)
    picked, sc = Engine.krum_select_host(D, GK.HOSTILE_F)
    assert picked == list(G["hostile_picked"]) and np.array_equal(u64(sc), G["hostile_score_bits"])
    assert Engine.krum_select_host(D, GK.HOSTILE_F, 1)[0] == list(G["hostile_picked_m1"])
    assert Engine.krum_select_host(D, GK.HOSTILE_F, 3)[0] == list(G["hostile_picked_m3"])


def test_ties_break_towards_the_earlier_row(G):
    n, f, _ = GK.HOST_SHAPES[4]  # every distance alike
    D = matrix(G, "host_D_bits_4", n)
    assert Engine.krum_select_host(D, 3, 5)[0] == [0, 1, 2, 3, 4]
    inf = np.full((7, 7), np.inf)
    np.fill_diagonal(inf, 0.0)
    picked, sc = Engine.krum_select_host(inf, 2, 2)  # +inf orders and ties like any other value
    assert picked == [0, 1] and np.isinf(sc).all()


def test_host_step_statuses():
    D = np.ones((6, 6)) - np.eye(6)
    with pytest.raises(AggregationError) as e:
        Engine.krum_select_host(D, 2)  # 6 < 2 f + 3
    assert e.value.status == -3
    with pytest.raises(AggregationError) as e:
        Engine.krum_select_host(D, 1, 6)  # m > n - f
    assert e.value.status == -3
    assert Engine.krum_select_host(D, 1, 5)[0] == [0, 1, 2, 3, 4]
    for bad in (np.nan, -1.0):
        B = D.copy()
        B[4, 2] = bad
        with pytest.raises(AggregationError) as e:
            Engine.krum_select_host(B, 1)
        assert e.value.status == -1
    for f, m in ((-1, 0), (1, -1)):
        with pytest.raises(AggregationError) as e:
            Engine.krum_select_host(D, f, m)
        assert e.value.status == -1
    with pytest.raises(KO.TooFewRows):
        KO.select(D, 2)
    with pytest.raises(KO.BadDistance):
        KO.select(np.full((6, 6), np.nan), 1)


def test_abi_is_additive():
    from pygrid_amd import _lib, robust

    header = (ROOT / "include" / "pgh_api.h").read_text()
    assert "#define PGH_ABI_VERSION 10" in header and _lib.load().pgh_abi_version() == 10
    assert "#define PGH_KRUM_MAX_ROWS 1024" in header
    assert "PGH_GEOMETRIC_MEDIAN = 6" in header and not re.search(r"PGH_[A-Z_]+\s*=\s*7\b", header)  # no new pgh_mode
    assert "PGH_KRUM" not in header.replace("PGH_KRUM_MAX_ROWS", "")
    for name in ("pgh_row_pairdist", "pgh_krum_select_host", "pgh_krum_select", "pgh_krum_stats"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and f"int {name}(" in header
    assert KRUM_KEY not in [k.key for k in robust.KINDS] and len(robust.KINDS) == 4


# ---- server_config["diff_krum"] ---------------------------------------------------------------------------------

def test_krum_of():
    assert krum_of({}) is None and krum_of({KRUM_KEY: None}) is None and krum_of({KRUM_KEY: False}) is None
    assert krum_of({KRUM_KEY: {"byzantine": 3}}) == KrumSpec(3, None)
    assert krum_of({KRUM_KEY: {"byzantine": 0, "keep": 1}}) == KrumSpec(0, 1)
    assert krum_of({KRUM_KEY: {"byzantine": np.int64(2), "keep": 4.0}}) == KrumSpec(2, 4)
    assert krum_of({KRUM_KEY: {"byzantine": 2, "keep": None}}) == KrumSpec(2, None)
    assert krum_of({KRUM_KEY: {"byzantine": 9}}, krum=None) is None  # the argument overrides the key
    assert krum_of({}, krum={"byzantine": 1}) == KrumSpec(1) and krum_of({}, krum=KrumSpec(5, 2)) == KrumSpec(5, 2)
    with pytest.raises(dataclasses.FrozenInstanceError):
        krum_of({KRUM_KEY: {"byzantine": 3}}).byzantine = 4
    for bad in (True, 3, "on", [2], {}, {"keep": 2}, {"byzantine": True}, {"byzantine": 1.5}, {"byzantine": -1},
                {"byzantine": "2"}, {"byzantine": 2, "keep": 0}, {"byzantine": 2, "keep": False},
                {"byzantine": 2, "keep": 2.5}, {"byzantine": 2, "m": 3}, {"byzantine": float("nan")}):
        with pytest.raises(AggregationError):
            krum_of({KRUM_KEY: bad})


def test_settings_of_and_precedence():
    s = settings_of({KRUM_KEY: {"byzantine": 2}})
    assert s == CloseSettings(None, None, None, KrumSpec(2)) and bool(s) and s.rule_kwargs() == {}
    assert settings_of({}).select is None and not settings_of({})
    assert settings_of({KRUM_KEY: {"byzantine": 2}}, krum=None).select is None
    assert settings_of({}, krum={"byzantine": 1, "keep": 3}).select == KrumSpec(1, 3)
    both = settings_of({KRUM_KEY: {"byzantine": 2}, TRIM_KEY: 1, "server_optimizer": {"name": "fedadam", "lr": 0.1}})
    assert both.rule.key == TRIM_KEY and both.select == KrumSpec(2) and both.opt is not None
    with pytest.raises(AggregationError):  # parsed even beside something that would speak first
        settings_of({KRUM_KEY: {"byzantine": -2}, CLIP_KEY: 1.0})
    # a data-dependent selection beside the noise is refused
    with pytest.raises(KrumUnavailableError):
        settings_of({KRUM_KEY: {"byzantine": 2}, CLIP_KEY: 1.0, "dp_noise": {"multiplier": 1.0}})

    def closed(settings):
        with settings.fail_closed():
            raise ModelNotAcceleratedError("a float64 model")

    with pytest.raises(KrumUnavailableError) as e:
        closed(s)
    assert "selects nothing" in str(e.value)
    with pytest.raises(both.rule.error):  # the rule speaks before the selection
        closed(both)
    opt = settings_of({KRUM_KEY: {"byzantine": 2}, "server_optimizer": {"name": "fedadam", "lr": 0.1}})
    with pytest.raises(KrumUnavailableError):  # the selection before the optimizer
        closed(opt)
    with pytest.raises(ServerOptUnavailableError):
        closed(settings_of({"server_optimizer": {"name": "fedadam", "lr": 0.1}}))
    with pytest.raises(PlanNotAcceleratedError):
        closed(settings_of({}))
    noise = CloseSettings(settings_of({CLIP_KEY: 1.0}).rule, None, settings_of(
        {CLIP_KEY: 1.0, "dp_noise": {"multiplier": 1.0}}).noise, KrumSpec(1))  # (not constructible by settings_of)
    with pytest.raises(DpNoiseUnavailableError):  # the noise first of all
        closed(noise)
    with pytest.raises(DpNoiseUnavailableError):
        noise.refusing_original(3)()
    with pytest.raises(KrumUnavailableError) as e:
        s.refusing_original(3)()
    assert "selects nothing" in str(e.value)
    with pytest.raises(both.rule.error):
        both.refusing_original(3)()
    with pytest.raises(KrumUnavailableError):
        opt.refusing_original(3)()


# ---- a numpy engine that selects with the oracle ----------------------------------------------------------------

class KrumEngine(NumpyEngine):
    def __init__(self):
        super().__init__()
        self.kstats = None
        self.trim = 0

    def set_trim(self, b):
        self.trim = int(b)

    def krum_select(self, slots, f, m=0):
        slots = [int(s) for s in slots]
        try:
            g = KO.krum([self.slot[s] for s in slots], int(f), int(m))
        except KO.TooFewRows as e:
            raise AggregationError(str(e), status=-3)
        self.kstats = {"rows": len(slots), "excluded": g["excluded"], "picked": len(g["picked"]),
                       "max_picked_score": g["max_picked_score"], "min_dropped_score": g["min_dropped_score"]}
        self.calls.append(("krum_select", tuple(slots), int(f), int(m)))
        return [slots[k] for k in g["picked"]]

    def krum_stats(self):
        return dict(self.kstats)

    def clip_stats(self):
        return {"rows": 0, "clipped": 0, "max_norm": 0.0}


class GroupEngine(KrumEngine):
    def krum_select(self, slots, f, m=0):
        raise AggregationError("pgh_krum_select: a group's shards each hold part of a row", status=-6)


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]
GOOD = [0, 1, 3, 4, 6, 8]  # of 9 workers; 2 and 5 are hostile, 7 holds a NaN
CFG = {KRUM_KEY: {"byzantine": 2}}


def ckpt_tensors(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


def diff_tensors(w):
    rng = np.random.default_rng([7, w])
    t = [(rng.standard_normal(s) * 0.1 + 1).astype(F) for s in SHAPES]
    if w == 2:
        t[2][:] = F(1e30)
    if w == 5:
        t = [(x * F(-10)).astype(F) for x in t]
    if w == 7:
        t[0][0, 0] = np.nan
    return t


def flat(ts):
    return np.concatenate([np.asarray(t, F).reshape(-1) for t in ts])


def test_close_time_aggregator_selects_then_averages():
    eng = KrumEngine()
    agg = CycleAggregator(eng)
    ckpt, diffs = ckpt_tensors(), [diff_tensors(w) for w in range(9)]
    ck_pb, pbs = build_state_fast(ckpt), [build_state_fast(d) for d in diffs]
    new = agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template")
    assert ("krum_select", tuple(range(9)), 2, 0) in eng.calls and eng.calls[-1] == ("finish", 6)
    want = O.fedavg_mean(ckpt, [diffs[w] for w in GOOD])
    assert all(np.array_equal(u32(g), u32(w)) for g, w in zip(parse_state(new), want))
    assert eng.kstats["excluded"] == 1 and eng.kstats["picked"] == 6
    # the same as the call without the selection over the picked diffs alone; all nine give something else
    same = agg.average_plan_diffs({}, ck_pb, [pbs[w] for w in GOOD], framing="template")
    assert same == new
    assert not np.isfinite(flat(parse_state(agg.average_plan_diffs({}, ck_pb, pbs, framing="template")))).all()
    # the argument overrides the key; keep = 1 is Krum
    one = agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", krum={"byzantine": 2, "keep": 1})
    best = KO.krum([flat(d) for d in diffs], 2, 1)["picked"]
    assert len(best) == 1 and one == agg.average_plan_diffs({}, ck_pb, [pbs[best[0]]], framing="template", krum=None)
    # weights: the picked diffs' alone
    wts = [1.0, 2.0, 50.0, 3.0, 4.0, 60.0, 5.0, 70.0, 6.0]
    got = agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", weights=wts)
    assert got == agg.average_plan_diffs({}, ck_pb, [pbs[w] for w in GOOD], framing="template",
                                         weights=[wts[w] for w in GOOD])
    # a trim count is checked against the picked count: 6 picked, b = 3 needs 7
    with pytest.raises(TrimUnavailableError):
        agg.average_plan_diffs({**CFG, TRIM_KEY: 3}, ck_pb, pbs, framing="template")
    # too few finite diffs for f, an engine without krum_select, a group: all fail closed
    with pytest.raises(KrumUnavailableError):
        agg.average_plan_diffs({KRUM_KEY: {"byzantine": 3}}, ck_pb, pbs, framing="template")
    with pytest.raises(KrumUnavailableError):
        CycleAggregator(NumpyEngine()).average_plan_diffs(CFG, ck_pb, pbs, framing="template")
    with pytest.raises(KrumUnavailableError):
        CycleAggregator(GroupEngine()).average_plan_diffs(CFG, ck_pb, pbs, framing="template")
    with pytest.raises(KrumUnavailableError):  # a plan the engine declines must not reach the node's own averaging
        agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", avg_plan=lambda *a: None)
    with pytest.raises(AggregationError):
        agg.average_plan_diffs({KRUM_KEY: 2}, ck_pb, pbs, framing="template")


def drive(n, reporters, slots, engine=None, **kw):
    eng = engine or KrumEngine()
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    inc = IncrementalCycle(eng, NUMEL, slots=slots, fold_batch=1, checkpoint=ck_pb, **kw)
    for w in range(n):
        inc.assigned(w, key=w)
    latest = {}
    for w in reporters:
        latest[w] = diff_tensors(w)
        inc.reported(w, build_state_fast(latest[w]))
    return inc, eng, ckpt, ck_pb, latest


def test_incremental_selects_at_the_close_and_folds_nothing_early():
    reporters = [4, 2, 0, 1, 6, 5, 8, 7, 3]
    inc, eng, ckpt, ck_pb, latest = drive(10, reporters, slots=10, krum={"byzantine": 2})
    assert inc.early_fold is False and inc._whole
    new = inc.close(ck_pb, framing="template")
    assert not any(c[0] == "fold" for c in eng.calls) and [c for c in eng.calls if c[0] == "finish"] == [("finish", 6)]
    want = O.fedavg_mean(ckpt, [latest[w] for w in GOOD])  # the close's order with the others left out
    assert all(np.array_equal(u32(g), u32(w)) for g, w in zip(parse_state(new), want))
    lc = inc.last_close
    assert lc["n"] == 9 and lc["early"] == 0
    assert lc["krum"] == {"byzantine": 2, "picked": 6, "excluded": 1, "max_picked_score": eng.kstats["max_picked_score"]}
    msg = settings_of(CFG).close_message(3, lc)
    assert "picked 6" in msg and "1 excluded" in msg
    # without the selection last_close has no such key, and its keys are what they were
    inc, eng, ckpt, ck_pb, latest = drive(4, [1, 3, 0], slots=4)
    inc.close(ck_pb, framing="template")
    assert "krum" not in inc.last_close
    assert list(inc.last_close)[-6:] == ["clipped", "max_norm", "trim", "median", "noise_multiplier", "noise_std"]
    # weights by worker: the picked workers' alone
    wts = {w: float(w + 1) for w in range(10)}
    inc, eng, ckpt, ck_pb, latest = drive(10, reporters, slots=10, krum=KrumSpec(2), mode=WEIGHTED_MEAN,
                                          weights_by_worker=wts)
    new = inc.close(ck_pb, framing="template")
    assert [float(x) for x in eng.weights] == [wts[w] for w in GOOD]
    # a trim count beside it: of the picked
    inc, eng, ckpt, ck_pb, latest = drive(10, reporters, slots=10, krum={"byzantine": 2}, trim_count=3)
    with pytest.raises(TrimUnavailableError):
        inc.close(ck_pb, framing="template")


def test_incremental_fails_closed():
    reporters = list(range(9))
    with pytest.raises(AggregationError):
        IncrementalCycle(KrumEngine(), NUMEL, slots=4, krum={"byzantine": -1})
    with pytest.raises(AggregationError):
        IncrementalCycle(KrumEngine(), NUMEL, slots=4, krum={"byzantine": 1}, settings=settings_of(CFG))
    # more reporters than slots: refused before anything is folded or any slot given up
    inc, eng, ckpt, ck_pb, latest = drive(9, reporters, slots=6, krum={"byzantine": 1})
    with pytest.raises(KrumUnavailableError):
        inc.close(ck_pb, framing="template", fetch=lambda w: build_state_fast(latest[w]))
    assert not any(c[0] in ("fold", "finish") for c in eng.calls)
    # an engine without krum_select, and one that answers PGH_E_UNSUPPORTED
    for engine in (NumpyEngine(), GroupEngine()):
        inc, eng, ckpt, ck_pb, latest = drive(9, reporters, slots=9, engine=engine, krum={"byzantine": 2})
        with pytest.raises(KrumUnavailableError):
            inc.close(ck_pb, framing="template")
        assert not any(c[0] == "finish" for c in eng.calls)
    # a non-float32 diff declines the cycle: under a selection that fails the close
    inc, eng, ckpt, ck_pb, latest = drive(9, reporters[:8], slots=9, krum={"byzantine": 2})
    inc._declined = "a float64 diff"
    with pytest.raises(KrumUnavailableError):
        inc.close(ck_pb, framing="template")
