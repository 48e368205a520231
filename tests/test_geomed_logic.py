"""CPU: geometric-median FedAvg (PGH_GEOMETRIC_MEDIAN) -- the definition's oracle against its golden file and
against what makes it Weiszfeld, the parsing of server_config["diff_geometric_median"], the rule's place in
robust.KINDS and settings.CloseSettings, and the host logic that wires it (select_mode, CycleAggregator,
IncrementalCycle) against a numpy engine that takes the geometric median with the oracle."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import geomed_oracle as GO  # noqa: E402
import gen_geomed_golden as GG  # noqa: E402
from fake_engine import NumpyEngine  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pygrid_amd import robust  # noqa: E402
from pygrid_amd.cycle import CycleAggregator, select_mode  # noqa: E402
from pygrid_amd.engine import GEOMETRIC_MEDIAN, ITERATIVE_MEAN, MEAN, MODE_NAMES, WEIGHTED_MEAN  # noqa: E402
from pygrid_amd.exceptions import AggregationError, ClipUnavailableError, DpNoiseUnavailableError, \
    GeometricMedianUnavailableError, MedianUnavailableError, ModelNotAcceleratedError, PlanNotAcceleratedError, \
    TrimUnavailableError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.robust import CLIP_KEY, GEOMED_KEY, MEDIAN_KEY, TRIM_KEY, geomed_of, rule_of  # noqa: E402
from pygrid_amd.settings import settings_of  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402

F = np.float32
DEFAULTS = (3, 1e-6)


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def G():
    return np.load(GG.GOLDEN)


# ---- the oracle: golden pins and what makes it Weiszfeld ------------------------------------------------------

def test_oracle_matches_the_golden_file(G):
    fresh = GG.cases()
    assert sorted(fresh) == sorted(G.files)
    for k in G.files:
        a, b = fresh[k], G[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            a, b = a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")
        assert np.array_equal(a, b), k


def test_golden_pins(G):
    ckpt, diffs = G["fold_ckpt"], G["fold_diffs"]
    for it in GG.FOLD_ITERS:
        g = GO.geomed(diffs, it)
        assert np.array_equal(u32(g["weights"]), G[f"fold_w_bits_{it}"])
        assert np.array_equal(u64(g["objectives"]), G[f"fold_obj_bits_{it}"])
        assert np.array_equal(u32(ckpt - g["v"]), G[f"fold_out_bits_{it}"])
    # iteration 0 starts from v = 0: its distances are the norms, its weights those of 1 / norm
    g1 = GO.geomed(diffs, 1)
    norms = np.sqrt(np.array([float(np.sum(d.astype(np.float64) ** 2)) for d in diffs]))
    np.testing.assert_allclose(g1["weights"], (1 / norms) / np.sum(1 / norms), rtol=1e-6)
    # K12 against row 1 itself: exactly +0.0 for that row
    assert G["distsq_bits"][1] == 0 and np.all(G["distsq_bits"][[0, 2, 3, 4]] != 0)
    # the zero point: K12's sum is K7's
    for d in diffs:
        assert u64([GO.row_distsq(d, np.zeros_like(d))])[0] == u64([GO.CO.row_sumsq(d)])[0]


def test_one_row_is_returned_as_it_is():
    rng = np.random.default_rng(1)
    for p in (1, 5, 4097):
        ckpt, d = rng.standard_normal(p).astype(F), rng.standard_normal(p).astype(F)
        for it in (1, 2, 16):
            g = GO.geomed([d], it)
            assert g["weights"][0] == F(1) and g["W"] == F(1)
            assert np.array_equal(u32(GO.fedavg_geomed(ckpt, [d], it)), u32(ckpt - d))


SLACK = 1e-6  # relative, for rounding: the oracle meets it on these seeds (asserted below)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_objective_does_not_increase(seed):
    """Weiszfeld's iteration decreases the sum of distances; iteration 0 (from v = 0) is the exception the
    definition makes, so the claim starts at iteration 1.  objectives[t] is the sum of distances to v^(t)."""
    rng = np.random.default_rng(seed)
    n, p = int(rng.integers(3, 12)), int(rng.integers(2, 300))
    centre = rng.standard_normal(p)
    diffs = [(centre + rng.standard_normal(p) * 10.0 ** rng.integers(-2, 2)).astype(F) for _ in range(n)]
    obj = GO.geomed(diffs, 16)["objectives"]
    assert len(obj) == 16
    for t in range(1, 15):
        assert obj[t + 1] <= obj[t] * (1 + SLACK), (t, obj)
    # and it is the objective: the oracle's figure is the plain f64 sum of distances to its own iterate
    v15 = GO.geomed(diffs, 15)["v"]
    np.testing.assert_allclose(obj[15], GO.objective_at(diffs, v15), rtol=1e-5)
    assert obj[15] < GO.objective_at(diffs, np.mean(np.stack(diffs).astype(np.float64), axis=0)) * (1 + SLACK)


def test_hostile_rows(G):
    ckpt, diffs, mean = GG.hostile_inputs()
    g = GO.geomed(diffs, 3)
    assert g["excluded"] == 2 and g["included"] == [0, 1, 2, 3, 4, 5, 7, 8]  # the NaN and the inf row are out
    out = GO.fedavg_geomed(ckpt, diffs, 3)
    assert np.isfinite(out).all() and np.array_equal(u32(out), G["hostile_out_bits"])
    # the all-1e30 row is in, and weighs next to nothing: the result stays with the seven
    assert np.max(np.abs(g["v"] - mean)) < 0.2
    with pytest.raises(GO.NoFiniteRow):
        GO.geomed([diffs[6], diffs[9]], 3)


def test_collinear_rows_land_near_the_middle():
    rng = np.random.default_rng(9)
    d = rng.standard_normal(50).astype(F)
    v = GO.geomed([d, F(2) * d, F(3) * d], 16)["v"]  # the geometric median of three collinear points: the middle one
    # one row replaced by 1e6 d: the plain mean of (d, 2d, 1e6 d) is ~3.3e5 |d| from 2d
    mean_dist = np.linalg.norm((d.astype(np.float64) * (1 + 2 + 1e6) / 3) - 2 * d.astype(np.float64))
    for rows in ([d, F(2) * d, F(3) * d], [d, F(2) * d, F(1e6) * d]):
        v = GO.geomed(rows, 16)["v"]
        assert np.linalg.norm(v.astype(np.float64) - 2 * d.astype(np.float64)) < 1e-3 * mean_dist


# ---- the ABI -----------------------------------------------------------------------------------------------------

def test_abi_and_mode_constant():
    from pygrid_amd import _lib

    assert MODE_NAMES[GEOMETRIC_MEDIAN] == "geometric_median" and GEOMETRIC_MEDIAN == 6
    assert _lib.load().pgh_abi_version() == 10
    header = (Path(__file__).resolve().parent.parent / "include" / "pgh_api.h").read_text()
    assert "PGH_GEOMETRIC_MEDIAN = 6" in header and "#define PGH_ABI_VERSION 10" in header
    assert "#define PGH_GEOMED_MAX_ITERS 16" in header
    for fn in ("int pgh_set_geomed(pgh_ctx* ctx, int iters, float nu);",
               "int pgh_row_distsq(pgh_ctx* ctx, const int32_t* slots, int n, const float* point, double* out);",
               "int pgh_geomed_stats(pgh_ctx* ctx, int* iters, int64_t* n_rows, int64_t* n_excluded, double* objective,"):
        assert fn in header
    for name in ("pgh_set_geomed", "pgh_row_distsq", "pgh_geomed_stats"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


# ---- server_config["diff_geometric_median"] ----------------------------------------------------------------------

def test_geomed_of():
    assert GEOMED_KEY == "diff_geometric_median"
    for off in ({}, {GEOMED_KEY: None}, {GEOMED_KEY: False}, {GEOMED_KEY: np.bool_(False)}):
        assert geomed_of(off) is None
    assert geomed_of({GEOMED_KEY: True}) == DEFAULTS and geomed_of({GEOMED_KEY: np.bool_(True)}) == DEFAULTS
    assert geomed_of({GEOMED_KEY: {}}) == DEFAULTS
    assert geomed_of({GEOMED_KEY: {"iterations": 1}}) == (1, 1e-6)
    assert geomed_of({GEOMED_KEY: {"iterations": 16.0, "smoothing": 0.5}}) == (16, 0.5)
    assert geomed_of({GEOMED_KEY: {"smoothing": np.float32(1e-3)}}) == (3, float(np.float32(1e-3)))
    assert geomed_of({GEOMED_KEY: {"iterations": np.int64(4), "smoothing": 1}}) == (4, 1.0)
    bad = (1, 0, 3, "true", 1.0, [3, 1e-6], (3, 1e-6),
           {"iterations": 0}, {"iterations": 17}, {"iterations": -1}, {"iterations": 2.5}, {"iterations": True},
           {"iterations": "3"}, {"iterations": None}, {"iterations": float("nan")}, {"iterations": float("inf")},
           {"smoothing": 0}, {"smoothing": -1e-6}, {"smoothing": float("nan")}, {"smoothing": float("inf")},
           {"smoothing": 1e-60}, {"smoothing": 1e60}, {"smoothing": True}, {"smoothing": "1e-6"}, {"smoothing": None},
           {"iters": 3}, {"iterations": 3, "nu": 1e-6}, {"tolerance": 1e-3})
    for b in bad:
        with pytest.raises(AggregationError):
            geomed_of({GEOMED_KEY: b})


# ---- KINDS, rule_of, settings_of ------------------------------------------------------------------------------------

def test_kinds_and_precedence():
    assert [k.key for k in robust.KINDS] == [GEOMED_KEY, MEDIAN_KEY, TRIM_KEY, CLIP_KEY]
    k = robust.KINDS[0]
    assert (k.arg, k.mode, k.error, k.setter) == ("geometric_median", GEOMETRIC_MEDIAN, GeometricMedianUnavailableError,
                                                  "set_geomed")
    assert k.off[0] == 0
    r = rule_of({GEOMED_KEY: True})
    assert r.key == GEOMED_KEY and r.value == DEFAULTS and r.mode == GEOMETRIC_MEDIAN
    assert rule_of({GEOMED_KEY: {"iterations": 2}}, geometric_median=None) is None  # an argument overrides the key
    assert rule_of({}, geometric_median=True).value == DEFAULTS
    assert rule_of({}, geometric_median=(5, 0.25)).value == (5, 0.25)  # the parsed form comes back as it went
    for other, val in ((MEDIAN_KEY, True), (TRIM_KEY, 2), (CLIP_KEY, 1.5)):
        with pytest.raises(GeometricMedianUnavailableError) as e:  # the first row speaks
            rule_of({GEOMED_KEY: True, other: val})
        assert f"cannot be combined with {other}" in str(e.value)
        with pytest.raises(AggregationError):  # a malformed setting raises beside a valid rule
            rule_of({GEOMED_KEY: {"iterations": 99}, other: val})
    # the pairs among the three other rules are what they were
    for cfg, err in (({MEDIAN_KEY: True, TRIM_KEY: 1}, MedianUnavailableError), ({MEDIAN_KEY: True, CLIP_KEY: 1.0}, MedianUnavailableError),
                     ({TRIM_KEY: 1, CLIP_KEY: 1.0}, TrimUnavailableError)):
        with pytest.raises(err):
            rule_of(cfg)
    assert not issubclass(GeometricMedianUnavailableError, PlanNotAcceleratedError)
    assert issubclass(GeometricMedianUnavailableError, AggregationError)


def test_settings_of():
    s = settings_of({GEOMED_KEY: {"iterations": 2, "smoothing": 1e-3}})
    assert s.rule.key == GEOMED_KEY and s.rule.value == (2, 1e-3) and s.rule_kwargs() == {"geometric_median": (2, 1e-3)}
    assert settings_of({}, geometric_median=True).rule.value == DEFAULTS
    assert settings_of({GEOMED_KEY: True}, geometric_median=None).rule is None
    assert not settings_of({GEOMED_KEY: False})
    # noise needs the clip rule: beside this one it is refused (the noise speaks first)
    with pytest.raises(DpNoiseUnavailableError):
        settings_of({GEOMED_KEY: True, "dp_noise": {"multiplier": 1.0}})
    with pytest.raises((GeometricMedianUnavailableError, DpNoiseUnavailableError)):
        settings_of({GEOMED_KEY: True, CLIP_KEY: 1.0, "dp_noise": {"multiplier": 1.0}})
    # an optimizer goes beside it
    s = settings_of({GEOMED_KEY: True, "server_optimizer": {"name": "fedadam", "lr": 0.1}})
    assert s.rule.key == GEOMED_KEY and s.opt is not None


def canonical(avg, item, num):
    return [(a * num + i) / (num + 1) for a, i in zip(avg, item)]


def test_select_mode():
    assert select_mode({}, geometric_median=True) == GEOMETRIC_MEDIAN
    assert select_mode({}, geometric_median=(3, 1e-6)) == GEOMETRIC_MEDIAN
    refusals = (
        lambda: select_mode({"iterative_plan": True}, canonical, geometric_median=True),
        lambda: select_mode({}, weights=[1.0, 2.0], geometric_median=True),
        lambda: select_mode({}, clip_norm=1.0, geometric_median=True),
        lambda: select_mode({}, trim_count=2, geometric_median=True),
        lambda: select_mode({}, median=True, geometric_median=True),
    )
    for call in refusals:
        with pytest.raises(GeometricMedianUnavailableError) as e:
            call()
        assert not isinstance(e.value, PlanNotAcceleratedError)
    assert select_mode({}) == MEAN and select_mode({}, geometric_median=None) == MEAN
    assert select_mode({"iterative_plan": True}, canonical) == ITERATIVE_MEAN and select_mode({}, weights=[1.0]) == WEIGHTED_MEAN


# ---- a numpy engine that takes the geometric median with the oracle ----------------------------------------------

class GeomedEngine(NumpyEngine):
    """Records the setters; GEOMETRIC_MEDIAN closes through the oracle, refused early like the engine's."""

    def __init__(self):
        super().__init__()
        self.geomed = (0, 0.0)
        self.clip = 0.0
        self.trim = 0
        self.stats = None

    def set_geomed(self, iters=3, nu=1e-6):
        self.geomed = (int(iters), float(nu))
        self.calls.append(("set_geomed", int(iters), float(nu)))

    def set_clip_norm(self, c):
        self.clip = float(c)
        self.calls.append(("set_clip_norm", float(c)))

    def set_trim(self, b):
        self.trim = int(b)
        self.calls.append(("set_trim", int(b)))

    def geomed_stats(self):
        return dict(self.stats)

    def fold_slots(self, mode, slots):
        if mode == GEOMETRIC_MEDIAN:
            raise AggregationError("a geometric median needs every row at once", status=-6)
        super().fold_slots(mode, slots)

    def _finish(self, mode, diffs):
        if mode != GEOMETRIC_MEDIAN:
            return super()._finish(mode, diffs)
        if self.ckpt is None:
            raise AggregationError("no resident checkpoint")
        if self.geomed[0] == 0:
            raise AggregationError("the mode without the setting", status=-3)
        g = GO.geomed(diffs, *self.geomed)
        self.stats = {"iterations": self.geomed[0], "rows": len(diffs), "excluded": g["excluded"],
                      "objective": float(g["objective"]), "max_weight": float(g["max_weight"])}
        with np.errstate(all="ignore"):
            self.ckpt = (self.ckpt - g["v"]).astype(F)


class UnsupportingEngine(GeomedEngine):
    """A group or a sub-range shard: the setter answers PGH_E_UNSUPPORTED."""

    def set_geomed(self, iters=3, nu=1e-6):
        if iters:
            raise AggregationError("pgh_set_geomed: a group's shards each hold part of a row", status=-6)


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]


def ckpt_tensors(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


def diff_tensors(w, version=0):
    rng = np.random.default_rng([version, w])
    t = [(rng.standard_normal(s) * 0.1 + 1).astype(F) for s in SHAPES]
    if w == 0:
        t[0][0, 0] = np.nan       # excluded
    if w == 5:
        t[2][:] = F(1e30)         # kept, with next to no weight
    return t


def flat(ts):
    return np.concatenate([np.asarray(t, F).reshape(-1) for t in ts])


def want_close(ckpt, diffs, iters=3, nu=1e-6):
    return GO.fedavg_geomed(flat(ckpt), [flat(d) for d in diffs], iters, nu)


def test_set_on_engine_fail_closed_and_refusing_original():
    eng = GeomedEngine()
    s = settings_of({GEOMED_KEY: {"iterations": 4}})
    s.set_on_engine(eng)
    assert eng.calls == [("set_clip_norm", 0.0), ("set_trim", 0), ("set_geomed", 4, 1e-6)] and eng.geomed == (4, 1e-6)
    eng.calls.clear()
    settings_of({CLIP_KEY: 2.0}).set_on_engine(eng)  # the next FL process on the engine: the rule is cleared
    assert eng.calls == [("set_clip_norm", 2.0), ("set_trim", 0), ("set_geomed", 0, 1e-6)] and eng.geomed[0] == 0
    settings_of({}).set_on_engine(NumpyEngine())  # an engine without the setter that no cycle needs is left alone
    with pytest.raises(GeometricMedianUnavailableError):
        s.set_on_engine(NumpyEngine())
    with pytest.raises(GeometricMedianUnavailableError):
        s.set_on_engine(UnsupportingEngine())
    with pytest.raises(GeometricMedianUnavailableError) as e:
        with s.fail_closed():
            raise ModelNotAcceleratedError("a float64 model")
    assert "takes no geometric median" in str(e.value)
    with pytest.raises(GeometricMedianUnavailableError):
        s.refusing_original(7)()
    assert settings_of({}).refusing_original(7) is None


def test_close_time_aggregator_and_last_close_key():
    eng = GeomedEngine()
    agg = CycleAggregator(eng)
    ckpt = ckpt_tensors()
    diffs = [diff_tensors(w) for w in range(7)]
    pbs = [build_state_fast(d) for d in diffs]
    ck_pb = build_state_fast(ckpt)
    new = agg.average_plan_diffs({GEOMED_KEY: True}, ck_pb, pbs, framing="template")
    got = flat(parse_state(new))
    assert np.isfinite(got).all() and np.array_equal(u32(got), u32(want_close(ckpt, diffs)))
    assert eng.stats["excluded"] == 1
    new2 = agg.average_plan_diffs({}, ck_pb, pbs, framing="template", geometric_median={"iterations": 2})
    assert np.array_equal(u32(flat(parse_state(new2))), u32(want_close(ckpt, diffs, 2)))
    new3 = agg.average_plan_diffs({GEOMED_KEY: False}, ck_pb, pbs[1:4], framing="template")  # the next process: the mean
    assert all(np.array_equal(u32(g), u32(w)) for g, w in zip(parse_state(new3), O.fedavg_mean(ckpt, diffs[1:4])))
    assert eng.geomed[0] == 0
    for cfg, kw in (({GEOMED_KEY: True}, {"weights": [1.0] * 7}), ({GEOMED_KEY: True, CLIP_KEY: 1.0}, {}),
                    ({GEOMED_KEY: True, TRIM_KEY: 1}, {}), ({GEOMED_KEY: True, MEDIAN_KEY: True}, {}),
                    ({GEOMED_KEY: True, "iterative_plan": True}, {"avg_plan": canonical})):
        with pytest.raises(GeometricMedianUnavailableError):
            agg.average_plan_diffs(cfg, ck_pb, pbs, framing="template", **kw)
        with pytest.raises(GeometricMedianUnavailableError):
            agg.average_params(cfg, ckpt, diffs, **kw)
    with pytest.raises(AggregationError):
        agg.average_plan_diffs({GEOMED_KEY: 1}, ck_pb, pbs, framing="template")
    # an engine that cannot apply the rule fails closed instead of falling back
    with pytest.raises(GeometricMedianUnavailableError):
        CycleAggregator(UnsupportingEngine()).average_plan_diffs({GEOMED_KEY: True}, ck_pb, pbs, framing="template")


def drive(n, reporters, slots, **kw):
    eng = kw.pop("engine", None) or GeomedEngine()
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


def test_incremental_one_finish_in_the_close_order():
    reporters = [4, 2, 0, 1, 6, 5]
    inc, eng, ckpt, ck_pb, latest = drive(8, reporters, slots=8, geometric_median=True)
    assert inc.geometric_median == DEFAULTS and inc.early_fold is False
    new = inc.close(ck_pb, framing="template")
    order = sorted(reporters)  # assignment order
    assert np.array_equal(u32(flat(parse_state(new))), u32(want_close(ckpt, [latest[w] for w in order])))
    assert not any(c[0] == "fold" for c in eng.calls) and [c for c in eng.calls if c[0] == "finish"] == [("finish", 6)]
    lc = inc.last_close
    assert lc["n"] == 6 and lc["early"] == 0 and lc["median"] is False and lc["trim"] is None
    assert lc["geometric_median"] == {"iterations": 3, "excluded": 1, "objective": eng.stats["objective"],
                                      "max_weight": eng.stats["max_weight"]}
    assert "1 excluded" in settings_of({GEOMED_KEY: True}).close_message(3, lc)
    # without the rule last_close has no such key
    inc, eng, ckpt, ck_pb, latest = drive(4, [1, 2, 3], slots=4)
    inc.close(ck_pb, framing="template")
    assert "geometric_median" not in inc.last_close
    assert list(inc.last_close)[-6:] == ["clipped", "max_norm", "trim", "median", "noise_multiplier", "noise_std"]


def test_incremental_refusals():
    for kw in ({"mode": ITERATIVE_MEAN}, {"clip_norm": 1.0}, {"trim_count": 1}, {"median": True},
               {"weights_by_worker": {0: 1.0}}):
        with pytest.raises(GeometricMedianUnavailableError):
            IncrementalCycle(GeomedEngine(), NUMEL, slots=4, geometric_median=True, **kw)
    with pytest.raises(AggregationError):
        IncrementalCycle(GeomedEngine(), NUMEL, slots=4, geometric_median={"iterations": 0})
    with pytest.raises(GeometricMedianUnavailableError):
        IncrementalCycle(UnsupportingEngine(), NUMEL, slots=4, geometric_median=True)
    # more reporters than slots: refused before anything is folded or any slot given up
    inc, eng, ckpt, ck_pb, latest = drive(7, range(1, 7), slots=4, geometric_median=(2, 1e-6))
    held = dict(inc._slot_of)
    db = {w: build_state_fast(d) for w, d in latest.items()}
    with pytest.raises(GeometricMedianUnavailableError):
        inc.close(ck_pb, framing="template", order=list(range(1, 7)), fetch=db.__getitem__)
    assert not any(c[0] in ("fold", "finish") for c in eng.calls) and inc._slot_of == held
