"""CPU: trust-bootstrapped FedAvg (PGH_TRUSTED_MEAN, FLTrust) -- the numpy oracle against its golden file and its
own properties, the library's host step (plain C++, no GPU) against the oracle, the parsing of
``server_config["diff_trust_root"]``, every combination in ``settings_of``, and the host layer (``select_mode``,
``CycleAggregator``, ``IncrementalCycle``, the installed node) against a numpy engine that applies the rule with
the oracle."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import gen_trust_golden as GT  # noqa: E402
import trust_oracle as TO  # noqa: E402
from fake_engine import NumpyEngine  # noqa: E402
from fake_node import assign, host_process, make_node  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pygrid_amd import state  # noqa: E402
from pygrid_amd.cycle import CycleAggregator, select_mode  # noqa: E402
from pygrid_amd.engine import MEAN, MODE_NAMES, TRUSTED_MEAN, Engine  # noqa: E402
from pygrid_amd.exceptions import AggregationError, PlanNotAcceleratedError, TrustUnavailableError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.krum import KRUM_KEY  # noqa: E402
from pygrid_amd.settings import CloseSettings, settings_of  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402
from pygrid_amd.trust import TRUST_KEY, TrustSpec, root_flat, trust_of  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
ARG, STATE = -1, -3


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def G():
    return np.load(GT.GOLDEN)


# ---- the oracle ---------------------------------------------------------------------------------------------------

def test_oracle_regenerates_the_golden_file(G):
    fresh = GT.cases()
    assert sorted(fresh) == sorted(G.files)
    for k, v in fresh.items():
        a, b = np.asarray(v), G[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_row_dot_is_k7_over_products():
    rng = np.random.default_rng(1)
    for p in (1, 3, 4095, 4096, 4097, 3 * 4096 + 5):
        d = (rng.standard_normal(p) * 10.0 ** rng.integers(-3, 4, p)).astype(F)
        assert u64([TO.row_dot(d, d)])[0] == u64([CO.row_sumsq(d)])[0]  # a row against itself: K7's bits
        assert u64([TO.row_dot(d, np.zeros(p, F))])[0] == 0            # against zeros: +0.0, never -0.0
        assert u64([TO.row_dot(-d, np.zeros(p, F))])[0] == 0
        g = rng.standard_normal(p).astype(F)
        assert abs(TO.row_dot(d, g) - np.dot(d.astype(np.float64), g.astype(np.float64))) <= 1e-9 * np.abs(d).max() * p


def test_one_trusted_row_comes_back_rescaled_to_the_root_norm():
    rng = np.random.default_rng(2)
    root = rng.standard_normal(5000).astype(F)
    for scale in (1e-3, 1.0, 250.0):
        row = ((root + rng.standard_normal(5000) * 0.3) * scale).astype(F)
        t = TO.trust([row], root)
        assert t["trusted"] == 1 and len(t["weights"]) == 1
        n_acc = np.linalg.norm(t["acc"].astype(np.float64))
        assert abs(n_acc / t["root_norm"] - 1) < 1e-6  # (two f32 roundings per element)
        # and along the row: acc = row * (n0 / n_row), the cosine cancels against T
        assert np.allclose(t["acc"], row * (t["root_norm"] / np.sqrt(CO.row_sumsq(row))), rtol=1e-6, atol=0)


def test_a_hostile_majority_moves_nothing(G):
    ckpt, diffs, root = G["hostile_ckpt"], G["hostile_diffs"], G["hostile_root"]
    assert np.abs(diffs).max() <= 1e30 and len(diffs) == 10 and len(GT.HONEST) == 3
    t = TO.trust(diffs, root)
    assert t["excluded"] == 0 and t["trusted"] == 3  # the 7 hostile rows stay included, with trust 0
    assert [k for k in range(10) if t["ts"][k] > 0] == list(GT.HONEST)
    all_rows = TO.fedavg_trust(ckpt, diffs, root)
    honest = TO.fedavg_trust(ckpt, diffs[list(GT.HONEST)], root)
    assert np.array_equal(all_rows, honest)  # as values: signed zeros may differ
    assert np.isfinite(all_rows).all()


def test_nonfinite_rows_are_excluded_and_a_subnormal_norm_is_clamped(G):
    ckpt, diffs, root = G["fold_ckpt"], G["fold_diffs"].copy(), G["fold_root"]
    diffs[1, 17] = np.nan
    diffs[4, 4098] = np.inf
    t = TO.trust(diffs, root)
    assert t["included"] == [0, 2, 3] and t["excluded"] == 2 and np.isnan(t["dot"][[1, 4]]).all()
    assert np.array_equal(u32(TO.fedavg_trust(ckpt, diffs, root)), u32(TO.fedavg_trust(ckpt, diffs[[0, 2, 3]], root)))
    # a hostile row of subnormal norm along the root: its rescale n0 / n_c overflows f32 and is clamped to FLT_MAX
    tiny = np.zeros_like(root)
    tiny[0] = np.copysign(F(1e-45), root[0])
    t = TO.trust([G["fold_diffs"][0], tiny], root)
    assert t["weights"][1] == np.finfo(F).max and np.isfinite(t["weights"]).all() and np.isfinite(t["acc"]).all()
    s0, ss, dt = GT.weights_inputs()
    w = TO.trust_weights(s0, ss, dt)
    assert w["included"] == [0, 1, 2, 5, 6, 7] and w["weights"][3] == np.finfo(F).max
    assert w["weights"][1] == 0 and w["weights"][2] == 0 and w["weights"][4] == 0  # away, all zero, orthogonal


def test_oracle_refusals(G):
    diffs, root = G["fold_diffs"], G["fold_root"]
    with pytest.raises(TO.NoTrustedRow):
        TO.trust(-np.abs(diffs), np.abs(root) + F(0.1))  # every row points away: T == 0
    with pytest.raises(TO.NoTrustedRow):
        TO.trust(np.full_like(diffs, np.nan), root)       # no finite row
    with pytest.raises(TO.NoTrustedRow):
        TO.trust(np.zeros_like(diffs), root)              # all-zero rows: ts = 0
    for bad in (np.zeros_like(root), np.where(np.arange(root.size) == 3, np.nan, root),
                np.where(np.arange(root.size) == 5, -np.inf, root)):
        with pytest.raises(TO.BadRoot):
            TO.trust(diffs, bad.astype(F))


def test_the_result_stays_inside_the_ball_of_the_root_norm():
    """||acc|| <= n0 (1 + m).  Exactly, acc = sum (ts_c / T) n0 u_c over unit vectors u_c: a convex combination
    of vectors of norm n0, so rows at an angle to each other land well inside the ball (excess -0.12 .. -0.26
    below) and only rows parallel to the root reach its surface, where the f32 weights and the f32 fold decide the
    sign of the excess.  Each seed therefore gets both kinds.  The largest excess the oracle shows on these seeds is
    1.3691410005733928e-08 (seed 1, parallel rows); m is twice that."""
    m = 2 * 1.3691410005733928e-08
    worst = -np.inf
    for seed in range(8):
        rng = np.random.default_rng(seed)
        p, n = 3000 + 517 * seed, 3 + 4 * seed
        root = (rng.standard_normal(p) * 10.0 ** rng.integers(-2, 3)).astype(F)
        rows = [((root * rng.choice([-1.0, 1.0, 1.0]) + rng.standard_normal(p) * np.abs(root).mean() * rng.uniform(0, 3))
                 * 10.0 ** rng.integers(-4, 9)).astype(F) for _ in range(n)]
        rows[0] = (root * F(1e6)).astype(F)  # (at least one trusted row)
        parallel = [(root * F(10.0 ** rng.uniform(-4, 8))).astype(F) for _ in range(n)]
        for kind, rs in (("mixed", rows), ("parallel", parallel)):
            t = TO.trust(rs, root)
            excess = np.linalg.norm(t["acc"].astype(np.float64)) / t["root_norm"] - 1
            print(f"seed {seed} {kind}: excess {excess!r}")
            worst = max(worst, excess)
            assert excess <= m, (seed, kind, excess)
    assert abs(worst - m / 2) < 1e-13  # the figure m was taken from: a change of the seeds moves both


# ---- the library's host step (no GPU) -----------------------------------------------------------------------------

def test_host_step_matches_oracle_and_golden(G):
    s0, ss, dt = float(G["w_s0"][0]), G["w_sumsq"], G["w_dot"]
    w, inc, T = Engine.trust_weights_host(s0, ss, dt)
    assert np.array_equal(u32(w), G["w_bits"]) and inc == list(G["w_included"]) and u64([T])[0] == G["w_T_bits"][0]
    for key in ("fold", "hostile"):
        t = TO.trust(G[f"{key}_diffs"], G[f"{key}_root"])
        w, inc, T = Engine.trust_weights_host(t["s0"], t["sumsq"], t["dot"])
        assert np.array_equal(u32(w), u32(t["weights"])) and inc == t["included"] and u64([T])[0] == u64([t["T"]])[0]
    assert np.array_equal(u32(Engine.trust_weights_host(G["fold_s0_bits"].view(np.float64)[0], G["fold_sumsq_bits"].view(np.float64),
                                                        G["fold_dot_bits"].view(np.float64))[0]), G["fold_w_bits"])
    rng = np.random.default_rng(9)
    for _ in range(50):  # random sums and dots, Cauchy-Schwarz respected, a few special rows
        n = int(rng.integers(1, 12))
        s0 = float(10.0 ** rng.uniform(-30, 30))
        ss = 10.0 ** rng.uniform(-60, 60, n)
        dt = rng.uniform(-1, 1, n) * np.sqrt(ss) * np.sqrt(s0)
        ss[rng.random(n) < 0.15] = np.inf
        ss[rng.random(n) < 0.1] = 0.0
        try:
            o = TO.trust_weights(s0, ss, dt)
        except TO.NoTrustedRow:
            with pytest.raises(AggregationError) as e:
                Engine.trust_weights_host(s0, ss, dt)
            assert e.value.status == STATE
            continue
        w, inc, T = Engine.trust_weights_host(s0, ss, dt)
        assert np.array_equal(u32(w), u32(o["weights"])) and inc == o["included"] and u64([T])[0] == u64([o["T"]])[0]


def test_host_step_statuses():
    def status(*a):
        with pytest.raises(AggregationError) as e:
            Engine.trust_weights_host(*a)
        return e.value.status

    ok = ([1.0, 4.0], [0.5, 1.0])
    for s0 in (0.0, -1.0, float("nan"), float("inf")):
        assert status(s0, *ok) == ARG
    assert status(1.0, [np.nan, np.inf], [0.0, 0.0]) == STATE   # no row included
    assert status(1.0, [], []) == STATE
    assert status(1.0, [1.0, 4.0], [-0.5, 0.0]) == STATE        # T == 0
    assert status(1.0, [0.0], [0.0]) == STATE                   # an all-zero row has no direction
    with pytest.raises(AggregationError):
        Engine.trust_weights_host(1.0, [1.0, 2.0], [1.0])


def test_abi_header_and_names():
    from pygrid_amd import _lib, robust

    header = (ROOT / "include" / "pgh_api.h").read_text()
    assert "#define PGH_ABI_VERSION 10" in header and _lib.load().pgh_abi_version() == 10
    assert re.search(r"PGH_GEOMETRIC_MEDIAN = 6,\s*PGH_TRUSTED_MEAN\b[^,}]*\}\s*pgh_mode;", header)
    assert "trust-bootstrapped FedAvg (PGH_TRUSTED_MEAN, FLTrust; kernel K14)" in header
    for proto in ("int pgh_set_trust(pgh_ctx* ctx, int on);",
                  "int pgh_trust_root(pgh_ctx* ctx, const float* root, size_t nbytes);",
                  "int pgh_row_dot(pgh_ctx* ctx, const int32_t* slots, int n, const float* point, double* out);",
                  "int pgh_trust_weights_host(double s0, const double* sumsq, const double* dot, int n, float* weights,",
                  "int pgh_trust_stats(pgh_ctx* ctx, int* on, int64_t* n_rows, int64_t* n_excluded, int64_t* n_trusted,"):
        assert proto in header, proto
    for name in ("pgh_set_trust", "pgh_trust_root", "pgh_row_dot", "pgh_trust_weights_host", "pgh_trust_stats"):
        assert hasattr(_lib.load(), name)
    assert TRUSTED_MEAN == 7 and MODE_NAMES[7] == "trusted_mean"
    assert len(robust.KINDS) == 4  # the rule is not a row of robust.KINDS
    for name in ("set_trust", "trust_root", "row_dot", "trust_weights_host", "trust_stats"):
        assert callable(getattr(Engine, name))


# ---- the key and the settings -------------------------------------------------------------------------------------

def test_trust_of():
    assert TRUST_KEY == "diff_trust_root"
    for off in ({}, {TRUST_KEY: None}, {TRUST_KEY: False}, {TRUST_KEY: np.bool_(False)}):
        assert trust_of(off) is None
    assert trust_of({TRUST_KEY: True}) == TrustSpec() and trust_of({TRUST_KEY: np.bool_(True)}) == TrustSpec()
    assert trust_of({TRUST_KEY: True}, trust=None) is None and trust_of({}, trust=True) == TrustSpec()
    assert trust_of({}, trust=TrustSpec()) == TrustSpec()
    for bad in (1, 0, "yes", 1.0, {"on": True}, [True], b"root"):
        with pytest.raises(AggregationError) as e:
            trust_of({TRUST_KEY: bad})
        assert type(e.value) is AggregationError and TRUST_KEY in str(e.value)


def test_settings_of_every_combination():
    s = settings_of({TRUST_KEY: True})
    assert s == CloseSettings(None, None, None, None, TrustSpec()) and bool(s) and s.rule_kwargs() == {}
    assert CloseSettings(None, None, None, None).trust is None and not CloseSettings()  # the positional forms still work
    assert settings_of({}).trust is None and settings_of({TRUST_KEY: True}, trust=None).trust is None
    assert settings_of({}, trust=True).trust == TrustSpec()
    # beside every rule of robust.KINDS, and beside noise: refused
    for rule in ({"diff_clip_norm": 1.0}, {"diff_trim_count": 1}, {"diff_median": True}, {"diff_geometric_median": True}):
        with pytest.raises(TrustUnavailableError) as e:
            settings_of({TRUST_KEY: True, **rule})
        assert TRUST_KEY in str(e.value) and next(iter(rule)) in str(e.value)
    for cfg in ({TRUST_KEY: True, "diff_clip_norm": 1.0, "dp_noise": {"multiplier": 1.0}},
                {TRUST_KEY: True, "dp_noise": {"multiplier": 1.0}}):
        with pytest.raises(TrustUnavailableError):
            settings_of(cfg)
    # beside a selection and beside a server optimizer: allowed
    s = settings_of({TRUST_KEY: True, KRUM_KEY: {"byzantine": 1}, "server_optimizer": {"name": "fedadam", "lr": 0.1}})
    assert s.trust == TrustSpec() and s.select is not None and s.opt is not None
    # a malformed key raises the plain error
    with pytest.raises(AggregationError) as e:
        settings_of({TRUST_KEY: "on"})
    assert type(e.value) is AggregationError
    # the one fail-closed decision and the stand-in for the node's own averaging
    s = settings_of({TRUST_KEY: True})
    with pytest.raises(TrustUnavailableError) as e:
        with s.fail_closed():
            raise PlanNotAcceleratedError("a user plan")
    assert "trusts every diff" in str(e.value) and isinstance(e.value.__cause__, PlanNotAcceleratedError)
    with pytest.raises(TrustUnavailableError) as e:
        s.refusing_original(3)()
    assert "trusts every diff" in str(e.value)
    assert settings_of({}).refusing_original(3) is None
    msg = s.close_message(3, {"n": 5, "trust": {"trusted": 4, "excluded": 1, "total_trust": 2.5, "max_weight": 0.5, "root_norm": 1.5}})
    assert "4 trusted" in msg and "1 excluded" in msg and TRUST_KEY in msg


def test_select_mode():
    t = TrustSpec()
    assert select_mode({}, trust=t) == TRUSTED_MEAN and select_mode({}, trust=None) == MEAN
    with pytest.raises(TrustUnavailableError):
        select_mode({}, weights=[1.0, 2.0], trust=t)
    with pytest.raises(TrustUnavailableError):  # the canonical iterative plan: the engine runs it, not under the rule
        select_mode({"iterative_plan": True}, lambda avg, item, num: [(a * num + i) / (num + 1) for a, i in zip(avg, item)], trust=t)
    with pytest.raises(TrustUnavailableError) as e:  # a plan the engine declines
        select_mode({}, lambda *a: None, trust=t)
    assert isinstance(e.value.__cause__, PlanNotAcceleratedError)


def test_root_flat():
    numel = [15, 3, 7]
    rng = np.random.default_rng(0)
    ts = [rng.standard_normal(s).astype(F) for s in ((5, 3), (3,), (7,))]
    want = np.concatenate([t.reshape(-1) for t in ts])
    for form in (build_state_fast(ts), ts, tuple(ts), want, want.astype(np.float64)):
        got = root_flat(form, numel)
        assert got.dtype == F and got.shape == (25,) and np.array_equal(got, want)
    for bad in (None, want[:-1], ts[:2], [ts[1], ts[0], ts[2]], build_state_fast(ts[:2]), b"not a state"):
        with pytest.raises(TrustUnavailableError):
            root_flat(bad, numel)


# ---- a numpy engine that applies the rule with the oracle ---------------------------------------------------------

class TrustEngine(NumpyEngine):
    def __init__(self):
        super().__init__()
        self.trust_on = False
        self.root = None
        self.tstats = {"on": False, "rows": 0, "excluded": 0, "trusted": 0, "total_trust": 0.0, "max_weight": 0.0, "root_norm": 0.0}

    def set_layout(self, numel):
        super().set_layout(numel)
        self.trust_on, self.root = False, None

    def reserve(self, n, dtype=0, parties=1):
        super().reserve(n, dtype, parties)
        self.root = None

    def reset(self):
        super().reset()
        self.root = None

    def set_trust(self, on=True):
        self.trust_on = bool(on)
        self.calls.append(("set_trust", bool(on)))

    def trust_root(self, root):
        if not self.trust_on:
            raise AggregationError("pgh_trust_root: the rule is off", status=STATE)
        r = np.ascontiguousarray(root, F).reshape(-1)
        s0 = CO.row_sumsq(r)
        self.root = None
        if r.size != self.P or not (np.isfinite(s0) and s0 > 0):
            raise AggregationError("pgh_trust_root: bad root", status=ARG)
        self.root = r.copy()
        self.calls.append(("trust_root", len(self.slot)))

    def _finish(self, mode, diffs):
        if mode != TRUSTED_MEAN:
            return super()._finish(mode, diffs)
        if not self.trust_on or self.root is None:
            raise AggregationError("PGH_TRUSTED_MEAN needs its setting and the cycle's root", status=STATE)
        try:
            t = TO.trust(diffs, self.root)
        except TO.NoTrustedRow as e:
            raise AggregationError(str(e), status=STATE)
        self.tstats = {"on": True, "rows": len(diffs), "excluded": t["excluded"], "trusted": t["trusted"],
                       "total_trust": float(t["T"]), "max_weight": float(t["max_weight"]), "root_norm": float(t["root_norm"])}
        with np.errstate(all="ignore"):
            self.ckpt = (self.ckpt - t["acc"]).astype(F)

    def trust_stats(self):
        return dict(self.tstats)

    def krum_select(self, slots, f, m=0):
        import krum_oracle as KO

        slots = [int(s) for s in slots]
        g = KO.krum([self.slot[s] for s in slots], int(f), int(m))
        self.kstats = {"rows": len(slots), "excluded": g["excluded"], "picked": len(g["picked"]),
                       "max_picked_score": g["max_picked_score"], "min_dropped_score": g["min_dropped_score"]}
        return [slots[k] for k in g["picked"]]

    def krum_stats(self):
        return dict(self.kstats)

    def clip_stats(self):
        return {"rows": 0, "clipped": 0, "max_norm": 0.0}

    def fedavg(self, mode, flat):
        self.ckpt = np.ascontiguousarray(flat, F).copy()
        n = len(self.slot)
        self._finish(mode, [self.slot[k] for k in range(n)])
        return self.ckpt.copy()

    def ingest(self, k, flat):
        self.slot[k] = np.ascontiguousarray(flat, F).reshape(-1).copy()


class GroupEngine(TrustEngine):
    def set_trust(self, on=True):
        if on:
            raise AggregationError("pgh_set_trust: a group's shards each hold part of a row", status=-6)


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]
HOSTILE = (2, 5, 6, 7, 8)  # of 9 workers: a hostile majority; 7 holds a NaN besides
CFG = {TRUST_KEY: True}


def ckpt_tensors(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


def root_tensors(cycle=0):
    rng = np.random.default_rng([11, cycle])
    return [(rng.standard_normal(s) * 0.1).astype(F) for s in SHAPES]


def diff_tensors(w, cycle=0):
    rng = np.random.default_rng([7, w, cycle])
    t = [(r + rng.standard_normal(r.shape) * 0.02).astype(F) for r in root_tensors(cycle)]
    if w in HOSTILE:
        t = [(x * F(-1e4 * (w + 1))).astype(F) for x in t]
    if w == 7:
        t[0][0, 0] = np.nan
    return t


def flat(ts):
    return np.concatenate([np.asarray(t, F).reshape(-1) for t in ts])


def want_flat(ckpt, workers, cycle=0):
    return TO.fedavg_trust(flat(ckpt), [flat(diff_tensors(w, cycle)) for w in workers], flat(root_tensors(cycle)))


def test_close_time_aggregator():
    eng = TrustEngine()
    agg = CycleAggregator(eng)
    ckpt, diffs, root = ckpt_tensors(), [diff_tensors(w) for w in range(9)], root_tensors()
    ck_pb, pbs = build_state_fast(ckpt), [build_state_fast(d) for d in diffs]
    want = want_flat(ckpt, range(9))
    assert np.isfinite(want).all()
    for form in (build_state_fast(root), root, flat(root)):  # State bytes, arrays, a flat array
        new = agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", trust_root=form)
        assert np.array_equal(u32(flat(parse_state(new))), u32(want))
    i_root = max(i for i, c in enumerate(eng.calls) if c[0] == "trust_root")
    assert eng.calls[i_root] == ("trust_root", 0)  # ahead of the ingests: the dots ride behind them
    assert eng.tstats["trusted"] == 4 and eng.tstats["excluded"] == 1
    # the hostile majority moved nothing: the four honest diffs alone give the same values
    honest = [w for w in range(9) if w not in HOSTILE]
    assert np.array_equal(want, want_flat(ckpt, honest))
    assert np.array_equal(u32(flat(agg.average_params(CFG, ckpt, diffs, trust_root=root))), u32(want))
    assert np.array_equal(u32(flat(agg.average_params({}, ckpt, diffs, trust=True, trust_root=flat(root)))), u32(want))
    # the next cycle without the key: the plain mean, the rule switched off on the shared engine
    new2 = agg.average_plan_diffs({}, ck_pb, pbs[:2], framing="template")
    for got, w in zip(parse_state(new2), O.fedavg_mean(ckpt, diffs[:2])):
        assert np.array_equal(u32(got), u32(w))
    assert eng.trust_on is False
    # after a selection: the rule over the picked diffs
    new3 = agg.average_plan_diffs({**CFG, KRUM_KEY: {"byzantine": 1}}, ck_pb, pbs[:5], framing="template", trust_root=root)
    import krum_oracle as KO

    picked = KO.krum([flat(d) for d in diffs[:5]], 1, 0)["picked"]
    assert np.array_equal(u32(flat(parse_state(new3))), u32(want_flat(ckpt, picked)))
    # no root, an unusable root, no trusted diff, weights, a declined plan, engines that cannot: all fail closed
    with pytest.raises(TrustUnavailableError):
        agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template")
    for bad in ([np.zeros(s, F) for s in SHAPES], flat(root)[:-1], [np.full(s, np.nan, F) for s in SHAPES]):
        with pytest.raises(TrustUnavailableError):
            agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", trust_root=bad)
    with pytest.raises(TrustUnavailableError):
        agg.average_plan_diffs(CFG, ck_pb, [pbs[w] for w in HOSTILE], framing="template", trust_root=root)
    with pytest.raises(TrustUnavailableError):
        agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", trust_root=root, weights=[1.0] * 9)
    with pytest.raises(TrustUnavailableError):
        agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", trust_root=root, avg_plan=lambda *a: None)
    with pytest.raises(TrustUnavailableError):
        CycleAggregator(NumpyEngine()).average_plan_diffs(CFG, ck_pb, pbs, framing="template", trust_root=root)
    with pytest.raises(TrustUnavailableError):
        CycleAggregator(GroupEngine()).average_plan_diffs(CFG, ck_pb, pbs, framing="template", trust_root=root)
    with pytest.raises(AggregationError):
        agg.average_plan_diffs({TRUST_KEY: "yes"}, ck_pb, pbs, framing="template", trust_root=root)


def drive(n, reporters, slots, engine=None, **kw):
    eng = engine or TrustEngine()
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    inc = IncrementalCycle(eng, NUMEL, slots=slots, fold_batch=1, checkpoint=ck_pb, **kw)
    for w in range(n):
        inc.assigned(w, key=w)
    for w in reporters:
        inc.reported(w, build_state_fast(diff_tensors(w)))
    return inc, eng, ckpt, ck_pb


def test_incremental_cycle():
    reporters = [4, 2, 0, 1, 6, 5, 8, 7, 3]
    want = want_flat(ckpt_tensors(), range(9))  # the close's order is the assignment order
    # the root at construction: it is on the engine before the first report
    inc, eng, ckpt, ck_pb = drive(10, reporters, slots=10, trust=True, trust_root=root_tensors())
    assert inc.early_fold is False and inc._whole
    assert [c for c in eng.calls if c[0] == "trust_root"] == [("trust_root", 0)]
    new = inc.close(ck_pb, framing="template")
    assert not any(c[0] == "fold" for c in eng.calls) and [c for c in eng.calls if c[0] == "finish"] == [("finish", 9)]
    assert np.array_equal(u32(flat(parse_state(new))), u32(want))
    lc = inc.last_close
    assert lc["n"] == 9 and lc["early"] == 0
    assert lc["trust"] == {"trusted": 4, "excluded": 1, "total_trust": eng.tstats["total_trust"],
                           "max_weight": eng.tstats["max_weight"], "root_norm": eng.tstats["root_norm"]}
    # the root at finish: the same bits
    inc, eng, ckpt, ck_pb = drive(10, reporters, slots=10, settings=settings_of(CFG))
    new2 = inc.close(ck_pb, framing="template", trust_root=build_state_fast(root_tensors()))
    assert new2 == new and [c for c in eng.calls if c[0] == "trust_root"] == [("trust_root", 9)]
    # without the rule last_close has no such key
    inc, eng, ckpt, ck_pb = drive(4, [1, 3, 0], slots=4)
    inc.close(ck_pb, framing="template")
    assert "trust" not in inc.last_close
    # fail closed: no root at all, more reporters than slots, weights, the iterative mode, an engine that cannot
    inc, eng, ckpt, ck_pb = drive(10, reporters, slots=10, trust=True)
    with pytest.raises(TrustUnavailableError):
        inc.close(ck_pb, framing="template")
    assert not any(c[0] == "finish" for c in eng.calls)
    inc, eng, ckpt, ck_pb = drive(9, reporters, slots=6, trust=True, trust_root=root_tensors())
    with pytest.raises(TrustUnavailableError):
        inc.close(ck_pb, framing="template", fetch=lambda w: build_state_fast(diff_tensors(w)))
    assert not any(c[0] in ("fold", "finish") for c in eng.calls)
    with pytest.raises(TrustUnavailableError):
        IncrementalCycle(TrustEngine(), NUMEL, slots=4, trust=True, weights_by_worker={0: 1.0}, mode=2)
    with pytest.raises(TrustUnavailableError):
        IncrementalCycle(TrustEngine(), NUMEL, slots=4, trust=True, mode=1)
    for engine in (NumpyEngine(), GroupEngine()):
        with pytest.raises(TrustUnavailableError):
            IncrementalCycle(engine, NUMEL, slots=4, trust=True)
    inc, eng, ckpt, ck_pb = drive(9, [2, 5, 6], slots=9, trust=True, trust_root=root_tensors())
    with pytest.raises(TrustUnavailableError):  # no reporter points along the root
        inc.close(ck_pb, framing="template")
    inc, eng, ckpt, ck_pb = drive(9, reporters[:8], slots=9, trust=True, trust_root=root_tensors())
    inc._declined = "a float64 diff"
    with pytest.raises(TrustUnavailableError):
        inc.close(ck_pb, framing="template")


# ---- the installed node -------------------------------------------------------------------------------------------

NODE_CFG = {"min_diffs": 5, "max_diffs": 5, "num_cycles": 0, "cycle_length": None, TRUST_KEY: True}


@pytest.mark.parametrize("report_time", [True, False], ids=["report-time", "close-time"])
def test_installed_node_asks_the_provider_once_per_cycle(report_time):
    from pygrid_amd import node as pnode

    asked = []

    def provider(process, cycle, checkpoint):
        asked.append((process, cycle.id, checkpoint))
        return build_state_fast(root_tensors(len(asked) - 1))

    mod = make_node()
    eng = TrustEngine()
    node = pnode.install(mod, engine=eng, framing="template", fold_batch=1, report_time=report_time, trust_root=provider)
    ck_pb = build_state_fast(ckpt_tensors())
    proc, model, _ = host_process(mod, NODE_CFG, ck_pb)
    want, before = flat(ckpt_tensors()), ck_pb
    for cycle in range(2):
        keys = {w: assign(mod, w, proc) for w in range(7)}
        for w in (3, 0, 2, 6, 5):  # three of five are hostile
            mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w, cycle)))
        assert mod.cycle_manager.task_errors == []
        want = TO.fedavg_trust(want, [flat(diff_tensors(w, cycle)) for w in (0, 2, 3, 5, 6)], flat(root_tensors(cycle)))
        saved = mod.model_manager.load(model_id=model.id).value
        assert saved == state.serialize_model_params(ck_pb, want) and np.isfinite(want).all()
        assert len(asked) == cycle + 1 and asked[-1][0] == proc.id and asked[-1][2] == before  # once, with the cycle's checkpoint
        before = saved
    assert node.stats["closes_report_time" if report_time else "closes_close_time"] == 2
    assert node.stats["closes_declined"] == 0 and not any(c[0] == "fold" for c in eng.calls)
    node.uninstall()


@pytest.mark.parametrize("provider", [None, lambda p, c, ck: None, lambda p, c, ck: 1 / 0,
                                      lambda p, c, ck: [np.zeros(s, F) for s in SHAPES], lambda p, c, ck: np.ones(3, F)],
                         ids=["none registered", "returns None", "raises", "all zero", "another layout"])
@pytest.mark.parametrize("report_time", [True, False], ids=["report-time", "close-time"])
def test_installed_node_fails_closed_without_a_usable_root(provider, report_time):
    from pygrid_amd import node as pnode

    mod = make_node()
    node = pnode.install(mod, engine=TrustEngine(), framing="template", fold_batch=1, trust_root=provider,
                         report_time=report_time)
    ck_pb = build_state_fast(ckpt_tensors())
    proc, model, _ = host_process(mod, NODE_CFG, ck_pb)
    keys = {w: assign(mod, w, proc) for w in range(6)}
    for w in (0, 1, 3, 4, 2):
        mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w)))
    errs = mod.cycle_manager.task_errors
    assert errs and all(isinstance(e, TrustUnavailableError) for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == ck_pb  # no checkpoint of another average was saved
    assert node._trust_roots == {}  # neither a root nor a refusal outlives its close: a retried close asks again
    node.uninstall()


def test_a_retried_close_asks_the_provider_again():
    """A provider that failed once is asked again by the next close of the cycle, and within one close once."""
    from pygrid_amd import node as pnode

    asked = []

    def provider(process, cycle, checkpoint):
        asked.append(cycle.id)
        if len(asked) == 1:
            raise RuntimeError("the root dataset is not mounted yet")
        return root_tensors()

    mod = make_node()
    node = pnode.install(mod, engine=TrustEngine(), framing="template", fold_batch=1, trust_root=provider)
    ck_pb = build_state_fast(ckpt_tensors())
    proc, model, cyc = host_process(mod, NODE_CFG, ck_pb)
    keys = {w: assign(mod, w, proc) for w in range(6)}
    for w in (0, 1, 3, 4, 2):
        mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w)))
    errs = mod.cycle_manager.task_errors
    assert len(asked) == 1 and errs and all(isinstance(e, TrustUnavailableError) for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == ck_pb
    mod.complete_cycle(mod.cycle_manager, cyc.id)  # the retry
    assert len(asked) == 2 and asked[0] == asked[1] == cyc.id
    want = want_flat(ckpt_tensors(), (0, 1, 2, 3, 4))
    assert mod.model_manager.load(model_id=model.id).value == state.serialize_model_params(ck_pb, want)
    assert node._trust_roots == {}
    node.uninstall()
