"""CPU: the DP noise of the clipped close -- the definition (tests/dp_oracle.py against known answers, a
scalar restatement, the library's plain C++ restatement and the golden file), the sampler's quality, the
``dp_noise`` parser and the host logic (drop-in, IncrementalCycle, installed node) over a numpy engine that
clips and noises with the oracles: bit-exact closes, and every way of not adding the noise fails closed."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import dp_oracle as DO  # noqa: E402
import gen_dp_golden as GG  # noqa: E402
import serveropt_oracle as SO  # noqa: E402
from fake_engine import NumpyEngine  # noqa: E402
from fake_node import assign, host_process, make_node  # noqa: E402
from pygrid_amd import dp, state  # noqa: E402
from pygrid_amd.cycle import CycleAggregator, make_average_plan_diffs  # noqa: E402
from pygrid_amd.engine import CLIPPED_MEAN, ITERATIVE_MEAN, Engine  # noqa: E402
from pygrid_amd.exceptions import AggregationError, ClipUnavailableError, DpNoiseUnavailableError, \
    PlanNotAcceleratedError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402

F = np.float32
KEY, ROUND = 0x0000567800001234, 7


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the definition -------------------------------------------------------------------------------------------

KATS = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KATS)
def test_philox_known_answers(ctr, key, want):
    assert " ".join("%08x" % int(x[0]) for x in DO.philox(*ctr, *key)) == want
    assert " ".join("%08x" % x for x in DO.philox_scalar(ctr, key)) == want


def test_oracle_is_its_scalar_restatement_on_4096_pairs():
    for base in (0, (1 << 32) - 2048):  # the second run crosses into the counter's second word
        z0, z1 = DO.pair_normals(KEY, ROUND, np.arange(base, base + 4096, dtype=np.uint64))
        for k in range(4096):
            assert (z0[k], z1[k]) == DO.pair_normals_scalar(KEY, ROUND, base + k), base + k


@pytest.mark.parametrize("i0,n", [(0, 100_000), (12_345, 4_099), ((1 << 33) + 5, 4_099)], ids=["zero", "odd", "above-2^33"])
def test_library_host_normals_are_the_oracle(i0, n):
    got = Engine.dp_normals_host(KEY, ROUND, i0, n)
    assert np.array_equal(DO.bits64(got), DO.bits64(DO.normals(KEY, ROUND, i0, n)))


def test_library_host_normals_argument_checks():
    assert Engine.dp_normals_host(KEY, ROUND, 5, 0).size == 0
    with pytest.raises(AggregationError):
        Engine.dp_normals_host(KEY, ROUND, -1, 4)


def test_oracle_matches_the_golden_file(gold):
    G = np.load(gold / "dp_cases.npz")
    want = GG.build()
    assert sorted(G.files) == sorted(want)
    for k in G.files:
        a, b = np.asarray(G[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k
    # and the library's host restatement reproduces the golden normals
    for k in range(len(GG.SPANS)):
        i0, n = (int(x) for x in G[f"span_{k}"])
        assert np.array_equal(DO.bits64(Engine.dp_normals_host(int(G["key"]), int(G["round"]), i0, n)), G[f"z_{k}"])


@pytest.fixture(scope="module")
def big_sample():
    return DO.pair_normals(KEY, ROUND, np.arange(1 << 21, dtype=np.uint64), want_attempts=True)


def test_sampler_quality(big_sample):
    z0, z1, took = big_sample
    z = np.concatenate([z0, z1])
    print("mean", z.mean(), "var", z.var(), "m4", (z ** 4).mean(), "corr", np.corrcoef(z0, z1)[0, 1], "attempts", took.max())
    assert abs(z.mean()) < 0.002
    assert abs(z.var() - 1.0) < 0.003
    assert abs((z ** 4).mean() - 3.0) < 0.02
    assert abs(np.corrcoef(z0, z1)[0, 1]) < 0.004
    assert took.max() < DO.ATTEMPTS  # every pair accepted within 32 attempts
    zs = np.sort(z)
    cdf = 0.5 * (1.0 + np.array([math.erf(x) for x in zs / math.sqrt(2.0)]))
    n = zs.size
    ks = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))
    print("ks", ks)
    assert ks < 0.0008


def test_plog_within_2_ulp_of_libm():
    rng = np.random.default_rng(3)
    s = np.concatenate([rng.uniform(0.0, 1.0, 60_000), 2.0 ** rng.uniform(-105, 0, 40_000)])
    s = s[(s > 0) & (s < 1)]
    got = DO.plog(s)
    want = np.array([math.log(x) for x in s])
    ulps = np.abs(got - want) / np.spacing(np.abs(want))
    print("plog max ulp", ulps.max())
    assert ulps.max() <= 2.0
    assert all(DO.plog_scalar(float(x)) == float(g) for x, g in zip(s[:2000], got[:2000]))


def test_noise_is_one_f64_product_rounded_to_f32():
    z = DO.normals(KEY, ROUND, 0, 64)
    sig = DO.sigma_of(1.1, 0.5, 3)
    assert sig == (float(F(1.1)) * 0.5) / 3.0
    n = DO.noise(KEY, ROUND, 1.1, 0.5, 3, 64)
    assert n.dtype == F and np.array_equal(u32(n), u32(np.array([F(sig * float(x)) for x in z])))
    g = np.linspace(-1, 1, 64).astype(F)
    ck = np.ones(64, F)
    assert np.array_equal(u32(DO.close(ck, g, KEY, ROUND, 1.1, 0.5, 3)), u32(ck - (g + n)))


# ---- the parser -----------------------------------------------------------------------------------------------

def test_dp_noise_of():
    assert dp.dp_noise_of({}) is None and dp.dp_noise_of({"dp_noise": None}) is None
    assert dp.dp_noise_of({"dp_noise": {"multiplier": 1.1}}) == dp.DpNoiseSpec(float(F(1.1)), None)
    assert dp.dp_noise_of({"dp_noise": {"multiplier": 2, "key": 5}}) == dp.DpNoiseSpec(2.0, 5)
    assert dp.dp_noise_of({"dp_noise": {"multiplier": np.float32(0.5), "key": np.int64(7)}}) == dp.DpNoiseSpec(0.5, 7)
    assert dp.dp_noise_of({"dp_noise": {"multiplier": 1.0}}, dp_noise=None) is None  # the argument overrides
    assert dp.dp_noise_of({}, dp_noise={"multiplier": 1.0, "key": (1 << 64) - 1}).key == (1 << 64) - 1
    bad = [1.1, "1.1", [1.1], True, {}, {"key": 3}, {"multiplier": 1.0, "sigma": 2.0}, {"multiplier": None},
           {"multiplier": True}, {"multiplier": "1"}, {"multiplier": 0}, {"multiplier": 0.0}, {"multiplier": -1.0},
           {"multiplier": float("nan")}, {"multiplier": float("inf")}, {"multiplier": 1e39}, {"multiplier": 1e-60},
           {"multiplier": 1.0, "key": -1}, {"multiplier": 1.0, "key": 1 << 64}, {"multiplier": 1.0, "key": 1.0},
           {"multiplier": 1.0, "key": True}, {"multiplier": 1.0, "key": "k"}]
    for cfg in bad:
        with pytest.raises(AggregationError):
            dp.dp_noise_of({"dp_noise": cfg})


def test_round_and_keys():
    assert dp.round_of(5) == 5 and dp.round_of((1 << 32) + 9) == 9 and dp.round_of(np.int64(3)) == 3
    for bad in ("5", 5.0, None, True):
        with pytest.raises(AggregationError):
            dp.round_of(bad)
    keys = dp.DpKeys()
    spec = dp.DpNoiseSpec(1.0, None)
    a, b = keys.key_for("proc-a", spec), keys.key_for("proc-b", spec)
    assert a == keys.key_for("proc-a", spec) and 0 <= a < 1 << 64 and a != b  # one draw per process, kept
    assert keys.key_for("proc-a", dp.DpNoiseSpec(1.0, 42)) == 42              # the setting's own key wins
    assert dp.DpKeys().key_for("proc-a", spec) != a                           # held by the process object


def test_noise_needs_the_clip_bound():
    assert not issubclass(DpNoiseUnavailableError, PlanNotAcceleratedError)
    agg = CycleAggregator(NoisyEngine())
    ck, pbs = build_state_fast(ckpt_tensors()), [build_state_fast(diff_tensors(w)) for w in range(3)]
    for cfg in ({"dp_noise": {"multiplier": 1.0}}, {"dp_noise": {"multiplier": 1.0}, "diff_trim_count": 1},
                {"dp_noise": {"multiplier": 1.0}, "diff_median": True}):
        with pytest.raises(DpNoiseUnavailableError):
            agg.average_plan_diffs(cfg, ck, pbs, dp_round=1)
    with pytest.raises(DpNoiseUnavailableError):
        IncrementalCycle(NoisyEngine(), NUMEL, slots=4, dp_noise={"multiplier": 1.0}, dp_round=1)
    assert agg.engine.calls == []  # refused before the engine was touched


# ---- a numpy engine that clips and noises with the oracles -----------------------------------------------------

class NoisyEngine(NumpyEngine):
    def __init__(self):
        super().__init__()
        self.clip = None
        self.noise = None  # (z, key, round)
        self.last = (0.0, 0)

    def set_clip_norm(self, c):
        self.clip = float(c) or None
        self.calls.append(("clip", float(c)))

    def ingest(self, k, flat):
        self.slot[k] = np.ascontiguousarray(flat, F).reshape(-1)
        self.calls.append(("ingest", k))

    def fedavg(self, mode, flat):
        self.ckpt = np.ascontiguousarray(flat, F).reshape(-1)
        self.fedavg_resident(mode)
        return self.ckpt.copy()

    def row_sumsq(self, slots, wait=True):
        return np.array([CO.row_sumsq(self.slot[int(s)]) for s in slots]) if wait else None

    def clip_stats(self):
        return {"rows": 0, "clipped": 0, "max_norm": 0.0}

    def set_dp_noise(self, z, key=0, rnd=0):
        self.noise = (float(F(z)), int(key), int(rnd)) if z else None
        self.calls.append(("noise", float(F(z)), int(key), int(rnd)))

    def dp_stats(self):
        return {"multiplier": self.noise[0] if self.noise else 0.0, "sigma": self.last[0], "n": self.last[1]}

    def _finish(self, mode, diffs):
        if self.noise is not None and mode != CLIPPED_MEAN:
            raise AggregationError("DP noise is set: only PGH_CLIPPED_MEAN may close a cycle", status=-3)
        if mode != CLIPPED_MEAN:
            return super()._finish(mode, diffs)
        if self.clip is None:
            raise AggregationError("PGH_CLIPPED_MEAN with clipping off", status=-3)
        if self.ckpt is None or not diffs:
            raise AggregationError("nothing to fold")
        if self.noise is None:
            self.ckpt = CO.fedavg_clipped(self.ckpt, diffs, self.clip)
            return
        z, key, rnd = self.noise
        g = SO.avg_from(lambda ck: CO.fedavg_clipped(ck, diffs, self.clip), self.P)
        self.last = (DO.sigma_of(z, self.clip, len(diffs)), len(diffs))
        self.ckpt = DO.close(self.ckpt, g, key, rnd, z, self.clip, len(diffs))


class GroupLikeEngine(NoisyEngine):
    def set_dp_noise(self, z, key=0, rnd=0):
        if z:
            raise AggregationError("pgh_set_dp_noise: a group's shards each hold part of a row", status=-6)


SHAPES = [(5, 3), (3,), (7,)]
NUMEL = [15, 3, 7]
C, Z, NKEY = 1.0, 1.1, 0xDEADBEEF0BADF00D
CFG = {"diff_clip_norm": C, "dp_noise": {"multiplier": Z, "key": NKEY}}


def ckpt_tensors(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(F) for s in SHAPES]


def diff_tensors(w, version=0):
    rng = np.random.default_rng([version, w])
    return [(rng.standard_normal(s) * 10.0 ** (w % 4 - 2)).astype(F) for s in SHAPES]  # norms 0.05 .. 50


def want_close(ckpt, diffs, rnd, key=NKEY):
    ck, ds = CO.flat(ckpt), [CO.flat(d) for d in diffs]
    g = SO.avg_from(lambda c0: CO.fedavg_clipped(c0, ds, C), ck.size)
    return DO.close(ck, g, key, rnd, Z, C, len(ds))


def test_drop_in_aggregator_noises_sets_and_clears():
    eng = NoisyEngine()
    agg = CycleAggregator(eng)
    ckpt = ckpt_tensors()
    diffs = [diff_tensors(w) for w in range(5)]
    ck_pb, pbs = build_state_fast(ckpt), [build_state_fast(d) for d in diffs]
    new = agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", dp_round=(1 << 32) + 12)
    want = want_close(ckpt, diffs, 12)  # the round is the id mod 2^32
    assert np.array_equal(u32(np.concatenate([t.reshape(-1) for t in parse_state(new)])), u32(want))
    assert not np.array_equal(u32(want), u32(CO.fedavg_clipped(CO.flat(ckpt), [CO.flat(d) for d in diffs], C)))
    first_ingest = next(i for i, c in enumerate(eng.calls) if c[0] == "ingest")
    assert eng.calls.index(("clip", C)) < eng.calls.index(("noise", float(F(Z)), NKEY, 12)) < first_ingest
    # the same close again (a retry): the same noise, bit for bit
    again = agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", dp_round=12)
    assert again == new
    # another round: other noise
    other = agg.average_plan_diffs(CFG, ck_pb, pbs, framing="template", dp_round=13)
    assert other != new
    # tensor lists in and out take the same path
    res = agg.average_params(CFG, ckpt, diffs, dp_round=12)
    assert np.array_equal(u32(np.concatenate([t.reshape(-1) for t in res])), u32(want))
    # the next process has no noise: cleared before its first ingest
    agg.average_plan_diffs({"diff_clip_norm": C}, ck_pb, pbs, framing="template")
    assert eng.noise is None and eng.calls[-1][0] != "noise"
    # a key not given is the process's own, drawn once
    cfg = {"diff_clip_norm": C, "dp_noise": {"multiplier": Z}}
    a = agg.average_plan_diffs(cfg, ck_pb, pbs, framing="template", dp_round=1, opt_key="p1")
    k1 = eng.noise[1]
    assert a == agg.average_plan_diffs(cfg, ck_pb, pbs, framing="template", dp_round=1, opt_key="p1") and eng.noise[1] == k1
    agg.average_plan_diffs(cfg, ck_pb, pbs, framing="template", dp_round=1, opt_key="p2")
    assert eng.noise[1] != k1


def test_drop_in_fails_closed():
    ckpt = ckpt_tensors()
    ck_pb, pbs = build_state_fast(ckpt), [build_state_fast(diff_tensors(w)) for w in range(3)]
    agg = CycleAggregator(NoisyEngine())
    with pytest.raises(DpNoiseUnavailableError):  # no round: two cycles must never share one
        agg.average_plan_diffs(CFG, ck_pb, pbs)
    with pytest.raises(DpNoiseUnavailableError):  # weights: the engine does not clip them
        agg.average_plan_diffs(CFG, ck_pb, pbs, weights=[1.0] * 3, dp_round=1)
    with pytest.raises(DpNoiseUnavailableError):  # a hosted plan the engine declines
        agg.average_plan_diffs(CFG, ck_pb, pbs, avg_plan=lambda d: d, dp_round=1)
    with pytest.raises(DpNoiseUnavailableError):  # an engine that cannot add it (a group)
        CycleAggregator(GroupLikeEngine()).average_plan_diffs(CFG, ck_pb, pbs, dp_round=1)

    class NoSetter(NoisyEngine):
        set_dp_noise = property()  # AttributeError, as on an engine built before the noise existed

    with pytest.raises(DpNoiseUnavailableError):
        CycleAggregator(NoSetter()).average_plan_diffs(CFG, ck_pb, pbs, dp_round=1)
    with pytest.raises(AggregationError):  # a malformed setting is not "no noise"
        agg.average_plan_diffs({"diff_clip_norm": C, "dp_noise": {"multiplier": 0}}, ck_pb, pbs, dp_round=1)
    # without the key, engines that know no noise keep working
    plain = NumpyEngine()
    CycleAggregator(plain).average_plan_diffs({}, ck_pb, pbs, framing="template")


def test_incremental_close_is_noised_and_reports_it():
    eng = NoisyEngine()
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    inc = IncrementalCycle(eng, NUMEL, slots=3, fold_batch=1, checkpoint=ck_pb, clip_norm=C,
                           dp_noise=CFG["dp_noise"], dp_round=77)
    for w in range(6):
        inc.assigned(w, key=w)
    db = {}
    for w in (2, 0, 1, 4, 3):  # worker 5 never reports
        db[w] = build_state_fast(diff_tensors(w))
        inc.reported(w, db[w])
    new = inc.close(ck_pb, framing="template", fetch=db.__getitem__)
    assert inc.last_close["early"] > 0  # early folds ran un-noised: K11 follows the FINAL pass alone
    want = want_close(ckpt, [diff_tensors(w) for w in range(5)], 77)
    assert np.array_equal(u32(np.concatenate([t.reshape(-1) for t in parse_state(new)])), u32(want))
    assert inc.last_close["noise_multiplier"] == float(F(Z))
    assert inc.last_close["noise_std"] == DO.sigma_of(Z, C, 5) == (float(F(Z)) * C) / 5
    # without noise the entries are there and empty, and a shared engine's setting is cleared
    inc2 = IncrementalCycle(eng, NUMEL, slots=3, checkpoint=ck_pb, clip_norm=C)
    assert eng.noise is None
    for w in range(2):
        inc2.assigned(w)
        inc2.reported(w, db[w])
    inc2.close(ck_pb, framing="template")
    assert inc2.last_close["noise_multiplier"] is None and inc2.last_close["noise_std"] is None
    with pytest.raises(DpNoiseUnavailableError):
        IncrementalCycle(GroupLikeEngine(), NUMEL, slots=3, clip_norm=C, dp_noise=CFG["dp_noise"], dp_round=1)
    with pytest.raises(DpNoiseUnavailableError):
        IncrementalCycle(NoisyEngine(), NUMEL, slots=3, clip_norm=C, dp_noise=CFG["dp_noise"])  # no round
    with pytest.raises((DpNoiseUnavailableError, ClipUnavailableError)):
        IncrementalCycle(NoisyEngine(), NUMEL, slots=3, clip_norm=C, mode=ITERATIVE_MEAN, dp_noise=CFG["dp_noise"], dp_round=1)


@pytest.mark.parametrize("report_time", [True, False], ids=["report-time", "close-time"])
def test_installed_node_saves_the_noised_checkpoint(report_time, caplog):
    from pygrid_amd import node as pnode

    mod = make_node()
    eng = NoisyEngine()
    node = pnode.install(mod, engine=eng, framing="template", fold_batch=1, report_time=report_time)
    cfg = {"min_diffs": 3, "max_diffs": 3, "num_cycles": 0, "cycle_length": None, **CFG}
    ckpt = ckpt_tensors()
    ck_pb = build_state_fast(ckpt)
    proc, model, first = host_process(mod, cfg, ck_pb)
    want = ckpt
    rounds = []
    with caplog.at_level("INFO"):
        for cycle in range(2):
            rnd = mod.cycle_manager.last(proc.id).id  # the round is the open cycle's id
            keys = {w: assign(mod, w, proc) for w in range(5)}
            for w in (3, 0, 1):
                mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w, cycle)))
            assert mod.cycle_manager.task_errors == []
            assert ("noise", float(F(Z)), NKEY, rnd) in eng.calls
            rounds.append(rnd)
            flat = want_close(want, [diff_tensors(w, cycle) for w in (0, 1, 3)], rnd)
            saved = mod.model_manager.load(model_id=model.id).value
            assert saved == state.serialize_model_params(ck_pb, flat)
            want = [flat]
    assert rounds[0] == first.id and rounds[1] != rounds[0]  # the round is the cycle's id
    assert node.stats["closes_report_time" if report_time else "closes_close_time"] == 2
    if report_time:
        assert any("noise std" in r.getMessage() for r in caplog.records)
    node.uninstall()


def test_installed_node_fails_closed():
    from pygrid_amd import node as pnode

    # an iterative plan: the engine neither clips nor noises it, and the node's own averaging must not run
    mod = make_node()
    pnode.install(mod, engine=NoisyEngine(), framing="template", fold_batch=1)
    cfg = {"min_diffs": 2, "max_diffs": 2, "num_cycles": 0, "cycle_length": None, "iterative_plan": True, **CFG}
    ck_pb = build_state_fast(ckpt_tensors())
    proc, model, _ = host_process(mod, cfg, ck_pb, b"ITERATIVE_AVG_PLAN")
    keys = {w: assign(mod, w, proc) for w in range(3)}
    for w in (0, 1):
        mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w)))
    errs = mod.cycle_manager.task_errors
    assert errs and all(isinstance(e, DpNoiseUnavailableError) for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == ck_pb  # no un-noised checkpoint was saved
    # noise without the bound
    mod = make_node()
    pnode.install(mod, engine=NoisyEngine(), framing="template", fold_batch=1)
    cfg = {"min_diffs": 2, "max_diffs": 2, "num_cycles": 0, "cycle_length": None, "dp_noise": {"multiplier": Z}}
    proc, model, _ = host_process(mod, cfg, ck_pb)
    keys = {w: assign(mod, w, proc) for w in range(3)}
    for w in (0, 1):
        mod.cycle_manager.submit_worker_diff(w, keys[w], build_state_fast(diff_tensors(w)))
    errs = mod.cycle_manager.task_errors
    assert errs and all(isinstance(e, DpNoiseUnavailableError) for e in errs)
    assert mod.model_manager.load(model_id=model.id).value == ck_pb


def test_drop_in_uses_the_cycle_id_and_never_the_node_averaging():
    mod = make_node()
    called = []
    eng = NoisyEngine()
    drop_in = make_average_plan_diffs(CycleAggregator(eng), mod.model_manager, mod.process_manager, mod.PlanManager,
                                      original=lambda *a: called.append(1), framing="template")
    ckpt = ckpt_tensors()
    proc, model, cyc = host_process(mod, CFG, build_state_fast(ckpt))
    key = assign(mod, "w", proc)
    wc = mod.cycle_manager._worker_cycles.first(request_key=key)
    wc.is_completed, wc.diff = True, build_state_fast(diff_tensors(1))
    drop_in(mod.cycle_manager, dict(CFG, num_cycles=1), cyc)
    assert ("noise", float(F(Z)), NKEY, cyc.id) in eng.calls and called == []
    saved = mod.model_manager.load(model_id=model.id).value
    assert saved == state.serialize_model_params(build_state_fast(ckpt), want_close(ckpt, [diff_tensors(1)], cyc.id))
    # noise without the bound: the close fails, the node's own averaging is not called
    proc, model, cyc = host_process(mod, {"dp_noise": {"multiplier": Z}}, build_state_fast(ckpt))
    with pytest.raises(DpNoiseUnavailableError):
        drop_in(mod.cycle_manager, {"dp_noise": {"multiplier": Z}}, cyc)
    assert called == []
