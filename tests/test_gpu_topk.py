"""GPU: the top-k sparsified update (pgh_set_topk, kernel K18), bit-exact against the numpy restatement of its
definition in tests/test_topk_logic.py (NaNs by position).  The definition is in include/pgh_api.h."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import serveropt_oracle as SO  # noqa: E402
import test_topk_logic as TL  # noqa: E402
from trim_oracle import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
MEAN, CLIPPED, MEDIAN, ARG, UNSUPPORTED = 0, 3, 5, -1, -6
SWEEP = 8192 * 1024  # params of one grid sweep: 8,192 workgroups of 1,024
# one lane, a ragged column, a workgroup's edge, several workgroups (the global merge), the stride loop
SIZES = (1, 3, 4, 5, 1023, 1025, 4099, SWEEP + 5)
KINDS = ("normal", "special", "digit2", "digit3")


@pytest.fixture(autouse=True)
def settings_off(engine):
    yield
    engine.set_topk(0)
    engine.set_server_opt(0)
    engine.set_clip_norm(0.0)


def ranks(p):
    return sorted({k for k in (1, 2, math.ceil(p / 100), p - 1, p) if 1 <= k <= p})


def column(kind, p, k, rng):
    """The value every one of the three diffs holds per param (their mean keeps ties tied and every class)."""
    sign = np.where(rng.integers(0, 2, p) == 1, F(-1), F(1))
    if kind == "digit2":  # magnitudes in [1, 1.125): the top 11 key bits agree, the second histogram decides
        return (U(0x3f800000) | rng.permutation(1 << 20)[:p].astype(U)).view(F) * sign
    if kind == "digit3":  # 1 + j 2^-23, j < 1,024: the top 21 key bits agree, the third histogram decides
        return (U(0x3f800000) | rng.integers(0, 1024, p).astype(U)).view(F) * sign
    v = rng.standard_normal(p).astype(F)
    if kind == "special":
        at = rng.permutation(p)
        sp = np.array([np.nan, -np.inf, 0.0, -0.0, 1e-45, -3e-45, np.inf, -np.nan], F)[:p // 2]
        v[at[:sp.size]] = sp
        m = np.sort(np.abs(v))[::-1][k - 1]  # (NaNs sort first here, as they rank) the magnitude at rank k ...
        tie = at[p // 2:p // 2 + p // 8 + 2]  # ... in a block of mixed signs that straddles it
        v[tie] = m * sign[tie]
    return v


def mean3(col):
    return ((col + col + col) / F(3)).astype(F)


def load(eng, rows):
    eng.set_layout([rows.shape[1]])
    eng.reserve(len(rows))
    for i, d in enumerate(rows):
        eng.ingest(i, d)


@pytest.mark.parametrize("p, kind", [(p, kind) for p in SIZES[:-1] for kind in KINDS] + [(SIZES[-1], "normal")])
def test_selection(engine, p, kind):
    rng = np.random.default_rng(p)
    ckpt = rng.standard_normal(p).astype(F)
    for k in ranks(p) if p < SWEEP else [math.ceil(p / 100)]:
        col = column(kind, p, k, rng)
        load(engine, np.stack([col] * 3))
        engine.set_topk(k, False)
        got, st = engine.fedavg(MEAN, ckpt), engine.topk_stats()
        want, _, tau, kept = TL.close(ckpt, mean3(col), None, k)
        assert same_bits(got, want), (kind, p, k)
        assert (st["k"], st["tau_bits"], st["kept"]) == (k, tau, kept), (kind, p, k)
        if k == p:  # everything applied, nothing remembered: the plain close of the same rows
            engine.set_topk(0)
            assert same_bits(got, engine.fedavg(MEAN, ckpt))


def test_error_memory_chain_repeat_and_commit(engine):
    p, k = 1025, 16
    rng = np.random.default_rng(2)
    ckpt = rng.standard_normal(p).astype(F)
    e = np.zeros(p, F)
    for rnd in range(3):
        rows = rng.standard_normal((3, p)).astype(F)
        if rnd == 0:
            load(engine, rows)
            engine.set_topk(k, True)
        else:
            engine.reset()  # the setting and the memory stay
            for i, d in enumerate(rows):
                engine.ingest(i, d)
        got = engine.fedavg(MEAN, ckpt)
        want, e2, tau, kept = TL.close(ckpt, ((rows[0] + rows[1] + rows[2]) / F(3)).astype(F), e, k)
        assert same_bits(got, want), rnd
        assert np.array_equal(engine.fedavg(MEAN, ckpt).view(U), got.view(U))  # repeated before the commit
        assert np.array_equal(engine.topk_state().view(U), e.view(U))  # not committed: e as it was
        engine.topk_commit()
        assert np.array_equal(engine.topk_state().view(U), e2.view(U)) and engine.topk_stats()["kept"] == kept
        ckpt, e = got, e2
    assert np.count_nonzero(e) > 0
    with pytest.raises(Exception) as err:  # nothing pending
        engine.topk_commit()
    assert err.value.status == -3
    mem = rng.standard_normal(p).astype(F)
    engine.load_topk_state(mem)
    assert np.array_equal(engine.topk_state().view(U), mem.view(U))


@pytest.mark.parametrize("mode", [CLIPPED, MEDIAN])
def test_behind_a_rule(engine, mode):
    p, k = 1025, 11
    rng = np.random.default_rng(mode)
    rows, ckpt = rng.standard_normal((5, p)).astype(F), rng.standard_normal(p).astype(F)
    load(engine, rows)
    engine.set_clip_norm(20.0 if mode == CLIPPED else 0.0)  # (some rows are clipped: their norms are about 32)
    g = SO.avg_from(lambda ck: engine.fedavg(mode, ck), p)  # the mode's own average, the setting off
    engine.set_topk(k, True)
    want, e2, tau, kept = TL.close(ckpt, g, np.zeros(p, F), k)
    assert same_bits(engine.fedavg(mode, ckpt), want)
    engine.topk_commit()
    assert same_bits(engine.topk_state(), e2) and engine.topk_stats()["tau_bits"] == tau


def test_ahead_of_fedadam(engine):
    p, k, hp = 1025, 32, (0.1, 0.9, 0.99, 1e-3)
    rng = np.random.default_rng(4)
    rows, ckpt = rng.standard_normal((3, p)).astype(F), rng.standard_normal(p).astype(F)
    load(engine, rows)
    engine.set_server_opt(SO.ADAM, *hp)
    engine.set_topk(k, False)
    s = TL.topk(((rows[0] + rows[1] + rows[2]) / F(3)).astype(F), None, k)[0]
    want, m2, _ = SO.step(SO.ADAM, ckpt, s, *SO.init_state(p, hp[3]), *hp)
    assert same_bits(engine.fedavg(MEAN, ckpt), want)
    engine.server_opt_commit()
    assert same_bits(engine.server_opt_state()[0], m2) and np.count_nonzero(m2) == k


def test_from_server_config_through_both_aggregators(engine):
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.state_schema import build_state_fast, parse_state

    shapes, rng = [(40, 25), (25,)], np.random.default_rng(6)
    p = 1025
    cfg = {"update_top_k": {"fraction": 0.01}}  # ceil(1025 / 100) = 11
    ck = [rng.standard_normal(s).astype(F) for s in shapes]
    flat = lambda ts: np.concatenate([np.asarray(t, F).reshape(-1) for t in ts])  # noqa: E731
    agg, e = CycleAggregator(engine), np.zeros(p, F)
    for _ in range(2):  # the second close takes the memory the first one committed
        ds = [[rng.standard_normal(s).astype(F) for s in shapes] for _ in range(3)]
        got = agg.average_params(cfg, ck, ds)
        want, e, _, kept = TL.close(flat(ck), ((flat(ds[0]) + flat(ds[1]) + flat(ds[2])) / F(3)).astype(F), e, 11)
        assert same_bits(flat(got), want) and engine.topk_stats()["kept"] == kept == 11
        ck = got
    assert same_bits(engine.topk_state(), e)
    ck_pb = build_state_fast(ck)
    inc = IncrementalCycle(engine, [1000, 25], slots=4, checkpoint=ck_pb, top_k={"count": 7, "error_feedback": False})
    ds = [[rng.standard_normal(s).astype(F) for s in shapes] for _ in range(3)]
    for w, d in enumerate(ds):
        inc.assigned(w)
        inc.reported(w, build_state_fast(d))
    got = flat(parse_state(inc.close(ck_pb)))
    want, _, tau, kept = TL.close(flat(ck), ((flat(ds[0]) + flat(ds[1]) + flat(ds[2])) / F(3)).astype(F), None, 7)
    assert same_bits(got, want)
    lc = inc.last_close
    assert (lc["top_k"], lc["top_k_kept"]) == (7, kept) and F(lc["top_k_threshold"]).view(U) == tau


@pytest.mark.parametrize("what, status", [("subrange", UNSUPPORTED), ("noise", UNSUPPORTED), ("k>P", ARG)])
def test_refusals_leave_the_context_usable(engine, what, status):
    import torch

    p, k = 1025, 9
    rng = np.random.default_rng(8)
    rows, ckpt = rng.standard_normal((3, p)).astype(F), rng.standard_normal(p).astype(F)
    load(engine, rows)
    engine.set_clip_norm(1e9)  # (nothing is clipped: the scales are 1)
    engine.set_topk(k, False)
    with pytest.raises(Exception) as err:
        if what == "subrange":
            ck, out = torch.from_numpy(ckpt).cuda(), torch.empty(p, device="cuda")
            engine.fedavg_device_range(MEAN, 0, 512, ck.data_ptr(), out.data_ptr())
        elif what == "noise":
            engine.set_dp_noise(1.0, 5, 1)
            engine.fedavg(CLIPPED, ckpt)
        else:
            engine.set_topk(p + 1, False)
    assert err.value.status == status, err.value
    engine.set_dp_noise(0.0)
    want = TL.close(ckpt, ((rows[0] + rows[1] + rows[2]) / F(3)).astype(F), None, k)[0]
    assert same_bits(engine.fedavg(MEAN, ckpt), want)  # the setting is as it was and the close runs
