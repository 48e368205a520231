"""GPU: server optimizers at the close (pgh_set_server_opt, kernel K10), bit-exact against
tests/serveropt_oracle.py with any NaN equal to any NaN: every kind x averaging mode over consecutive
committed cycles, ranges and entry points, commit semantics, state lifetime, NaN propagation, groups
and the Python layer.  The definition is in include/pgh_api.h and DESIGN.md section 5.

    python tests/test_gpu_serveropt.py median-passes     (the child process of the K9p matrix)
"""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import clip_oracle as CO  # noqa: E402
import gen_serveropt_golden as GG  # noqa: E402
import median_oracle as MO  # noqa: E402
import serveropt_oracle as SO  # noqa: E402
import trim_oracle as TO  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MEAN, ITERATIVE, WEIGHTED, CLIPPED, TRIMMED, MEDIAN = 0, 1, 2, 3, 4, 5
MODES = (MEAN, WEIGHTED, ITERATIVE, CLIPPED, TRIMMED, MEDIAN)
ARG, STATE = -1, -3
HP = {"lr": 0.3, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
WG, MAX_WGS = 1024, 2048  # SERVER_OPT_WG_PARAMS, SERVER_OPT_MAX_WGS (pgh_kernels.h)
GRID = WG * MAX_WGS        # past this many params of a launch K10's lanes take a second grid step
MATRIX_P = (1, 3, 4, 5, 255, 4097, WG - 1, WG, WG + 1, GRID - 1, GRID, GRID + 1)
MATRIX_N = (3, 4)
CYCLES = 3
WEIGHTS = (1.0, 2.5, 0.5, 3.0)


def device():
    return int(os.environ.get("PGH_DEVICE", "0"))


@pytest.fixture(scope="module")
def eng():
    from pygrid_amd import Engine

    with Engine(device()) as e:
        yield e


def set_opt(e, kind, **over):
    hp = dict(HP, **over)
    e.set_server_opt(kind, hp["lr"], hp["beta1"], hp["beta2"], hp["tau"])
    return hp


@functools.lru_cache(maxsize=4)
def rows_of(p, n_rows, seed=0):
    """n_rows diffs of p floats (signed zeros and subnormals among them) and a checkpoint."""
    rng = np.random.default_rng(1000 * seed + p)
    d = (rng.standard_normal((n_rows, p)) * 1e-2).astype(F)
    flat = d.reshape(-1)
    k = np.arange(0, flat.size, 7)
    flat[k[0::4]] = F(0.0)
    flat[k[1::4]] = F(-0.0)
    flat[k[2::4]] = np.array([0x00000003], np.uint32).view(F)[0]
    return d, (rng.standard_normal(p) * 0.1).astype(F)


def clip_bound(p):
    return float(F(1e-2 * np.sqrt(p)))  # about the rows' norm: some are clipped, some are not


def close_of(mode, diffs, p):
    """The averaging oracle of the mode as ``ckpt -> ckpt - g`` over flat arrays."""
    n = len(diffs)
    if mode == MEAN:
        return lambda ck: O.fedavg_mean([ck], [[d] for d in diffs])[0]
    if mode == WEIGHTED:
        return lambda ck: O.fedavg_weighted([ck], [[d] for d in diffs], WEIGHTS[:n])[0]
    if mode == ITERATIVE:
        return lambda ck: O.fedavg_iterative([ck], [[d] for d in diffs])[0]
    if mode == CLIPPED:
        return lambda ck: CO.fedavg_clipped(ck, diffs, F(clip_bound(p)))
    if mode == TRIMMED:
        return lambda ck: TO.fedavg_trimmed(ck, diffs, 1)
    return lambda ck: MO.fedavg_median(ck, diffs)


def prepare(e, mode, p, n):
    """Layout, slab and the mode's setting (a new layout drops the optimizer: set it afterwards)."""
    e.set_layout([p])
    e.reserve(n)
    e.set_clip_norm(clip_bound(p) if mode == CLIPPED else 0.0)
    e.set_trim(1 if mode == TRIMMED else 0)


def ingest(e, mode, diffs):
    e.reset()
    for k, d in enumerate(diffs):
        e.ingest(k, d)
    if mode == WEIGHTED:
        e.set_weights(WEIGHTS[:len(diffs)])


def check_state(e, kind, m, v, what):
    gm, gv = e.server_opt_state()
    assert SO.same_bits(gm, m), (what, "m")
    if kind != SO.MOMENTUM:
        assert SO.same_bits(gv, v), (what, "v")
    else:
        assert gv is None


def run_matrix(e, mode, kinds=SO.KINDS, ps=MATRIX_P, ns=MATRIX_N):
    for p in ps:
        rows, ckpt = rows_of(p, CYCLES * max(ns))
        for n in ns:
            cyc = [rows[c * n:(c + 1) * n] for c in range(CYCLES)]
            gs = [SO.avg_from(close_of(mode, d, p), p) for d in cyc]
            prepare(e, mode, p, n)
            for kind in kinds:
                e.set_server_opt(SO.NONE)
                hp = set_opt(e, kind)
                want = SO.run_cycles(kind, ckpt, gs, hp)
                ck = ckpt
                for c in range(CYCLES):
                    ingest(e, mode, cyc[c])
                    ck = e.fedavg(mode, ck)
                    e.server_opt_commit()
                    assert SO.same_bits(ck, want[c][0]), (mode, kind, p, n, c, "out")
                    check_state(e, kind, want[c][1], want[c][2], (mode, kind, p, n, c))
                assert e.server_opt_steps() == CYCLES
    e.set_server_opt(SO.NONE)


# ---- the main matrix -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_matrix_three_committed_cycles(eng, mode):
    if mode == MEDIAN:
        prepare(eng, mode, 8, 3)
        assert eng.effective_variant(MEDIAN) == 50  # K9; the K9p path runs in the child below
    run_matrix(eng, mode)


def test_matrix_median_passes_in_a_fresh_process():
    env = dict(os.environ, PGH_MEDIAN_PATH="passes")
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "median-passes"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "median-passes ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_special_values_match_the_golden_file(eng):
    """One diff under PGH_MEAN is the average itself (d / 1.0f); the state comes from an upload."""
    G = np.load(GG.GOLDEN)
    ck, g, m, v = G["ckpt"], G["g"], G["m"], G["v"]
    lr, b1, b2, tau = (float(x) for x in G["hp"])
    prepare(eng, MEAN, g.size, 1)
    for kind in SO.KINDS:
        eng.set_server_opt(kind, lr, b1, b2, tau)
        eng.load_server_opt_state(m, v if kind != SO.MOMENTUM else None)
        ingest(eng, MEAN, [g])
        out = eng.fedavg(MEAN, ck)
        eng.server_opt_commit()
        assert SO.same_bits(out, G[f"out_{kind}"]), kind
        check_state(eng, kind, G[f"m_{kind}"], G[f"v_{kind}"], kind)
    eng.set_server_opt(SO.NONE)


# ---- ranges and entry points ----------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [4, 8])
def test_device_range(eng, off):
    import torch

    p, n = 64, 3
    rows, ckpt = rows_of(p, n)
    g = SO.avg_from(close_of(MEAN, rows, p), p)
    for r in range(4):
        ln = 20 + r
        prepare(eng, MEAN, p, n)
        hp = set_opt(eng, SO.ADAM)
        ingest(eng, MEAN, rows)
        m0, v0 = SO.init_state(p, hp["tau"])
        want, wm, wv = SO.step(SO.ADAM, ckpt, g, m0, v0, **hp)
        ck = torch.from_numpy(ckpt).cuda()
        out = torch.full((p,), 77.0, dtype=torch.float32, device="cuda")
        eng.fedavg_device_range(MEAN, off, ln, ck.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        eng.server_opt_commit()
        got = out.cpu().numpy()
        sel = np.zeros(p, bool)
        sel[off:off + ln] = True
        assert SO.same_bits(got[sel], want[sel]), (off, ln)
        assert np.all(got[~sel] == F(77.0)), (off, ln)  # nothing outside the range is written
        gm, gv = eng.server_opt_state()
        assert SO.same_bits(gm[sel], wm[sel]) and SO.same_bits(gv[sel], wv[sel])
        assert SO.same_bits(gm[~sel], m0[~sel]) and SO.same_bits(gv[~sel], v0[~sel])
        # later partial closes too: a param outside the range keeps its committed moments, here uploaded
        # ones and then, a commit later, the same again (the planes were swapped in between)
        um, uv = (np.arange(p) * 1e-3).astype(F), (np.arange(p) * 1e-5 + 1e-6).astype(F)
        eng.load_server_opt_state(um, uv)
        wm, wv = um, uv
        for _ in range(2):
            eng.fedavg_device_range(MEAN, off, ln, ck.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            eng.server_opt_commit()
            want, sm, sv = SO.step(SO.ADAM, ckpt, g, wm, wv, **hp)
            wm, wv = np.where(sel, sm, wm), np.where(sel, sv, wv)
            assert SO.same_bits(out.cpu().numpy()[sel], want[sel]), (off, ln)
            gm, gv = eng.server_opt_state()
            assert SO.same_bits(gm, wm) and SO.same_bits(gv, wv), (off, ln)
    eng.set_server_opt(SO.NONE)


BIG_P = (1 << 20) + 7


@functools.lru_cache(maxsize=1)
def big_case():
    rows, ckpt = rows_of(BIG_P, 3)
    g = SO.avg_from(close_of(MEAN, rows, BIG_P), BIG_P)
    m0, v0 = SO.init_state(BIG_P, HP["tau"])
    return rows, ckpt, SO.step(SO.ADAM, ckpt, g, m0, v0, **HP)


def make_engine(**env):
    from pygrid_amd import Engine

    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return Engine(device())
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize("form", ["resident", "resident-4-ranges", "slots"])
def test_both_ranged_final_forms(eng, form):
    """2^20 + 7 params: pgh_fedavg_resident as one launch and as PGH_FINAL_RANGES=4 ranges over two
    streams, and pgh_fold_slots_finish_resident's FINAL pass in 4 MiB ranges."""
    rows, ckpt, (want, wm, wv) = big_case()
    e = make_engine(PGH_FINAL_RANGES="4") if form == "resident-4-ranges" else eng
    try:
        prepare(e, MEAN, BIG_P, 3)
        set_opt(e, SO.ADAM)
        ingest(e, MEAN, rows)
        e.ckpt_upload(ckpt)
        e.reset_stats()
        if form == "slots":
            e.fold_slots_finish_resident(MEAN, [0, 1, 2])
        else:
            e.fedavg_resident(MEAN)
        got = e.ckpt_download()
        launches = e.stats()["kernel_launches"]
        assert launches == {"resident": 2, "resident-4-ranges": 8, "slots": 4}[form]  # a K10 behind every FINAL launch
        e.server_opt_commit()
        assert SO.same_bits(got, want)
        check_state(e, SO.ADAM, wm, wv, form)
        e.set_server_opt(SO.NONE)
    finally:
        if e is not eng:
            e.close()


def test_stream_finish_resident(eng):
    p, n = 4097, 4
    rows, ckpt = rows_of(p, n)
    g = SO.avg_from(close_of(MEAN, rows, p), p)
    prepare(eng, MEAN, p, 2)  # a ring of 2 slots: the first fold is not the FINAL one
    hp = set_opt(eng, SO.YOGI)
    m0, v0 = SO.init_state(p, hp["tau"])
    want, wm, wv = SO.step(SO.YOGI, ckpt, g, m0, v0, **hp)
    eng.ckpt_upload(ckpt)
    eng.stream_begin(MEAN, 2)
    for k in range(n):
        eng.ingest(k, rows[k])
    eng.stream_finish_resident()
    eng.server_opt_commit()
    assert SO.same_bits(eng.ckpt_download(), want)
    check_state(eng, SO.YOGI, wm, wv, "stream")
    eng.set_server_opt(SO.NONE)


# ---- commit semantics, state lifetime ------------------------------------------------------------------------------

def test_repeated_final_is_identical_until_the_commit(eng):
    from pygrid_amd import AggregationError

    p, n = 4097, 3
    rows, ckpt = rows_of(p, n)
    g = SO.avg_from(close_of(MEAN, rows, p), p)
    prepare(eng, MEAN, p, n)
    hp = set_opt(eng, SO.ADAM)
    with pytest.raises(AggregationError) as ei:
        eng.server_opt_commit()  # no FINAL yet
    assert ei.value.status == STATE
    ingest(eng, MEAN, rows)
    a = eng.fedavg(MEAN, ckpt)
    b = eng.fedavg(MEAN, ckpt)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    m0, v0 = SO.init_state(p, hp["tau"])
    check_state(eng, SO.ADAM, m0, v0, "before the commit")  # the committed state has not moved
    assert eng.server_opt_steps() == 0
    eng.server_opt_commit()
    assert eng.server_opt_steps() == 1
    with pytest.raises(AggregationError) as ei:
        eng.server_opt_commit()  # nothing since the commit
    assert ei.value.status == STATE
    o1, m1, v1 = SO.step(SO.ADAM, ckpt, g, m0, v0, **hp)
    assert SO.same_bits(a, o1)
    c = eng.fedavg(MEAN, ckpt)  # now from the committed step
    assert SO.same_bits(c, SO.step(SO.ADAM, ckpt, g, m1, v1, **hp)[0])
    eng.load_server_opt_state(m1, v1)  # an upload clears what is pending
    with pytest.raises(AggregationError) as ei:
        eng.server_opt_commit()
    assert ei.value.status == STATE
    eng.set_server_opt(SO.NONE)


def test_state_lifetime(eng):
    from pygrid_amd import AggregationError

    p, n = 255, 3
    rows, ckpt = rows_of(p, n)
    g = SO.avg_from(close_of(MEAN, rows, p), p)
    prepare(eng, MEAN, p, n)
    hp = set_opt(eng, SO.ADAGRAD)
    ingest(eng, MEAN, rows)
    eng.fedavg(MEAN, ckpt)
    eng.server_opt_commit()
    m0, v0 = SO.init_state(p, hp["tau"])
    _, m1, v1 = SO.step(SO.ADAGRAD, ckpt, g, m0, v0, **hp)
    check_state(eng, SO.ADAGRAD, m1, v1, "one step")
    # a round trip through the host
    gm, gv = eng.server_opt_state()
    eng.load_server_opt_state(gm * F(2), gv * F(2))
    check_state(eng, SO.ADAGRAD, m1 * F(2), v1 * F(2), "uploaded")
    eng.load_server_opt_state(gm, gv)
    # pgh_reset and pgh_reserve keep it, and so does the same setting again
    eng.reset()
    eng.reserve(n + 2)
    set_opt(eng, SO.ADAGRAD)
    check_state(eng, SO.ADAGRAD, m1, v1, "after reset / reserve / same setting")
    assert eng.server_opt_steps() == 1
    # a changed lr starts again
    set_opt(eng, SO.ADAGRAD, lr=0.31)
    check_state(eng, SO.ADAGRAD, m0, v0, "changed lr")
    assert eng.server_opt_steps() == 0
    # a new layout drops the state and the setting
    eng.set_layout([p])
    eng.reserve(n)
    with pytest.raises(AggregationError) as ei:
        eng.server_opt_state()
    assert ei.value.status == STATE
    # validation
    for bad in (dict(lr=0.0), dict(lr=float("inf")), dict(lr=float("nan")), dict(beta1=1.0), dict(beta1=-0.5),
                dict(beta2=1.0), dict(tau=0.0), dict(tau=float("inf"))):
        with pytest.raises(AggregationError) as ei:
            set_opt(eng, SO.ADAM, **bad)
        assert ei.value.status == ARG, bad
    with pytest.raises(AggregationError) as ei:
        eng.set_server_opt(9, 0.1, 0.9, 0.99, 1e-3)
    assert ei.value.status == ARG
    set_opt(eng, SO.MOMENTUM, beta2=7.0, tau=-1.0)  # not FedAvgM's: ignored
    set_opt(eng, SO.ADAGRAD, beta2=7.0)
    eng.set_server_opt(SO.NONE)


def test_none_restores_the_plain_path(eng):
    from pygrid_amd import Engine

    p, n = 4097, 3
    rows, ckpt = rows_of(p, n)
    prepare(eng, MEAN, p, n)
    set_opt(eng, SO.ADAM)
    ingest(eng, MEAN, rows)
    eng.fedavg(MEAN, ckpt)
    eng.set_server_opt(SO.NONE)
    eng.reset_stats()
    got = eng.fedavg(MEAN, ckpt)
    launches = eng.stats()["kernel_launches"]
    with Engine(device()) as plain:
        prepare(plain, MEAN, p, n)
        ingest(plain, MEAN, rows)
        plain.reset_stats()
        want = plain.fedavg(MEAN, ckpt)
        assert launches == plain.stats()["kernel_launches"] == 1
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert SO.same_bits(got, O.fedavg_mean([ckpt], [[d] for d in rows])[0])


def test_nan_propagates_under_mean_and_not_under_median(eng):
    p, n = 255, 3
    rows, ckpt = rows_of(p, n)
    rows = rows.copy()
    rows[1, 5] = F("nan")
    rows[2, 9] = F("inf")
    for mode in (MEAN, MEDIAN):
        gs = [SO.avg_from(close_of(mode, rows, p), p), SO.avg_from(close_of(mode, rows_of(p, n, 1)[0], p), p)]
        prepare(eng, mode, p, n)
        hp = set_opt(eng, SO.ADAM)
        want = SO.run_cycles(SO.ADAM, ckpt, gs, hp)
        ck = ckpt
        for c, d in enumerate((rows, rows_of(p, n, 1)[0])):
            ingest(eng, mode, d)
            ck = eng.fedavg(mode, ck)
            eng.server_opt_commit()
            assert SO.same_bits(ck, want[c][0])
            check_state(eng, SO.ADAM, want[c][1], want[c][2], (mode, c))
        m, v = eng.server_opt_state()
        if mode == MEAN:  # the NaN stays in that parameter's state through the clean second cycle
            # (the infinity too: m and v stay infinite, and inf / inf makes the parameter a NaN)
            assert np.isnan(m[5]) and np.isnan(v[5]) and np.isnan(ck[5])
            assert np.isinf(m[9]) and np.isinf(v[9]) and np.isnan(ck[9])
            assert np.isfinite(np.delete(m, [5, 9])).all()
        else:
            assert np.isfinite(m).all() and np.isfinite(v).all() and np.isfinite(ck).all()
    eng.set_server_opt(SO.NONE)


# ---- groups ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kids", [2, 3])
def test_groups_are_bit_identical_to_one_context(eng, kids):
    from pygrid_amd import Engine

    p, n = 4097, 3
    rows, ckpt = rows_of(p, 2 * n)
    with Engine(devices=[device()] * kids) as grp:
        res = []
        for e in (eng, grp):
            prepare(e, TRIMMED, p, n)
            set_opt(e, SO.YOGI)
            ck = ckpt
            for c in range(2):
                ingest(e, TRIMMED, rows[c * n:(c + 1) * n])
                if c == 1:
                    e.reserve(n)  # a reserve between the cycles keeps the state (the children's too)
                    ingest(e, TRIMMED, rows[c * n:(c + 1) * n])
                e.ckpt_upload(ck)
                e.fedavg_resident(TRIMMED)
                ck = e.ckpt_download()
                e.server_opt_commit()
            assert e.server_opt_steps() == 2
            res.append((ck, *e.server_opt_state()))
        for a, b in zip(*res):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        gs = [SO.avg_from(close_of(TRIMMED, rows[c * n:(c + 1) * n], p), p) for c in range(2)]
        want = SO.run_cycles(SO.YOGI, ckpt, gs, HP)[-1]
        for a, b in zip(res[1], want):
            assert SO.same_bits(a, b)
        # upload through the group, slice by slice, and back
        m, v = res[1][1], res[1][2]
        grp.load_server_opt_state(m * F(3), v * F(3))
        gm, gv = grp.server_opt_state()
        assert SO.same_bits(gm, m * F(3)) and SO.same_bits(gv, v * F(3))
        grp.set_server_opt(SO.NONE)
        # a client-sharded int64 reserve re-shards the children: the moments are parked on the host first
        from pygrid_amd.serveropt import ServerOptStates, server_opt_of

        st, spec = ServerOptStates(), server_opt_of({"server_optimizer": {"name": "fedyogi", "lr": HP["lr"]}})
        st.bind(grp, "G", spec, p)
        grp.load_server_opt_state(m, v)
        grp.set_client_sharding(True)
        grp.reserve(n, 1, 2)
        assert grp.opt_owner is None and grp.opt_kind == SO.NONE
        grp.set_client_sharding(False)
        grp.reserve(n)
        st.bind(grp, "G", spec, p)
        gm, gv = grp.server_opt_state()
        assert SO.same_bits(gm, m) and SO.same_bits(gv, v)
        grp.set_server_opt(SO.NONE)
    eng.set_server_opt(SO.NONE)


# ---- the Python layer ------------------------------------------------------------------------------------------------

def test_cycle_aggregator_two_processes_alternate_on_one_engine(eng):
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.state_schema import build_state_fast, parse_state

    shapes = [(30, 10), (17,)]
    p = 317
    agg = CycleAggregator(eng)
    cfgs = {"A": {"server_optimizer": {"name": "fedadam", "lr": HP["lr"]}},
            "B": {"server_optimizer": {"name": "fedavgm", "lr": 0.5, "beta1": 0.5}, "diff_median": True},
            "C": {}}
    hps = {"A": dict(HP), "B": dict(HP, lr=0.5, beta1=0.5)}
    kinds = {"A": SO.ADAM, "B": SO.MOMENTUM}
    mode = {"A": MEAN, "B": MEDIAN, "C": MEAN}

    def split(flat):
        return [flat[:300].reshape(shapes[0]), flat[300:]]

    ck = {k: rows_of(p, 3, 40 + i)[1] for i, k in enumerate("ABC")}
    state = {k: SO.init_state(p, hps[k]["tau"]) for k in "AB"}
    for cyc in range(3):
        for i, k in enumerate("ABC"):
            rows = rows_of(p, 3, 10 * cyc + i + 1)[0]
            new = agg.average_plan_diffs(cfgs[k], build_state_fast(split(ck[k])),
                                         [build_state_fast(split(d)) for d in rows], opt_key=k)
            got = np.concatenate([np.asarray(t, F).reshape(-1) for t in parse_state(new)])
            if k == "C":
                want = close_of(MEAN, rows, p)(ck[k])
            else:
                g = SO.avg_from(close_of(mode[k], rows, p), p)
                want, m, v = SO.step(kinds[k], ck[k], g, *state[k], **hps[k])
                state[k] = (m, v)
            assert SO.same_bits(got, want), (cyc, k)
            ck[k] = got
    assert agg.opt_states.steps("A") == agg.opt_states.steps("B") == 3
    m, v, steps = agg.opt_states.state(eng, "A")
    assert SO.same_bits(m, state["A"][0]) and SO.same_bits(v, state["A"][1]) and steps == 3
    eng.set_server_opt(SO.NONE)


def test_incremental_cycle_binds_before_the_final_pass_and_commits_after(eng):
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.serveropt import ServerOptStates, server_opt_of
    from pygrid_amd.state_schema import build_state_fast, parse_state

    p = 317
    spec = server_opt_of({"server_optimizer": {"name": "fedyogi", "lr": HP["lr"]}})
    states = ServerOptStates()
    ck = rows_of(p, 4, 70)[1]
    m, v = SO.init_state(p, HP["tau"])
    for cyc in range(2):
        rows = rows_of(p, 4, 71 + cyc)[0]
        pb = build_state_fast([ck])
        inc = IncrementalCycle(eng, [p], slots=4, fold_batch=2, checkpoint=pb, server_opt=spec, opt_key="P",
                               opt_states=states)
        for w in range(4):
            inc.assigned(w)
        for w in (1, 0, 2, 3):
            inc.reported(w, build_state_fast([rows[w]]))
        states.bind(eng, None, None, p)  # a process without an optimizer had the engine meanwhile: the close binds again
        new = inc.close(pb)
        got = np.asarray(parse_state(new)[0], F).reshape(-1)
        g = SO.avg_from(close_of(MEAN, rows, p), p)
        want, m, v = SO.step(SO.YOGI, ck, g, m, v, **HP)
        assert SO.same_bits(got, want), cyc
        ck = got
    assert states.steps("P") == 2
    gm, gv, _ = states.state(eng, "P")
    assert SO.same_bits(gm, m) and SO.same_bits(gv, v)
    eng.set_server_opt(SO.NONE)


if __name__ == "__main__":
    if sys.argv[1:] != ["median-passes"]:
        sys.exit("usage: test_gpu_serveropt.py median-passes")
    from pygrid_amd import Engine

    with Engine(device()) as child:
        prepare(child, MEDIAN, 8, 3)
        assert child.effective_variant(MEDIAN) == 51, "PGH_MEDIAN_PATH=passes did not reach the context"
        run_matrix(child, MEDIAN)
    print("median-passes ok")
