"""CPU: the rank-trimmed mean's settings (``server_config["diff_trimmed_mean"]``) and the numpy restatement of its
definition (include/pgh_api.h) that tests/test_gpu_rank_trim.py compares kernel K17 against."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from trim_oracle import key, unkey  # noqa: E402

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32
KEY = "diff_trimmed_mean"
SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0, 0x80000000, 0x7149F2CA,  # +-NaN, +-inf, +-0, 1e30
                     1, 0x80000001, 0x007FFFFF, 0x7FFFFFFF], U32)  # subnormals, the bit pattern of the kernel's padding


def rank_trim(diffs, b):
    """``(mean [P], interior count [P], kL [P], kH [P])`` of N x [P] rows in fold order: the definition, step by step."""
    x = np.ascontiguousarray(diffs, F32)
    n, p = x.shape
    u = key(x).view(U32) ^ U32(0x80000000)
    s = np.sort(u, axis=0)
    L, H = s[b], s[n - 1 - b]
    inside, xd, S = (u > L) & (u < H), x.astype(F64), None
    with np.errstate(all="ignore"):
        for g in range(0, n, 64):
            sg = np.zeros(p, F64)
            for k in range(g, min(g + 64, n)):
                sg = np.where(inside[k], sg + xd[k], sg)
            S = sg if S is None else S + sg
        kL = np.where(L < H, (u <= L).sum(0) - b, n - 2 * b)
        kH = np.where(L < H, (n - b) - (u < H).sum(0), 0)
        value = lambda t: unkey((t ^ U32(0x80000000)).view(I32)).astype(F64)  # noqa: E731
        S = S + kL.astype(F64) * value(L)
        S = np.where(kH > 0, S + kH.astype(F64) * value(H), S)
        return (S / F64(n - 2 * b)).astype(F32), inside.sum(0), kL, kH


def fedavg(ckpt, diffs, b):
    return (np.asarray(ckpt, F32) - rank_trim(diffs, b)[0]).astype(F32)


def tall(kind, p=257):
    """1,024 rows: a grid of integers in [-3, 3], or normals with a special value in every fifth place of every row."""
    rng = np.random.default_rng(len(kind) + p)
    if kind == "grid":
        return rng.integers(-3, 4, (1024, p)).astype(F32)
    rows = rng.standard_normal((1024, p)).astype(F32).view(U32)
    for r in range(1024):
        rows[r, r % 5::5] = rng.choice(SPECIALS, size=rows[r, r % 5::5].size)
    return rows.view(F32)


def trims(n):
    return sorted({1, n // 4, (n - 1) // 2} - {0})


@pytest.mark.parametrize("n", [3, 9, 65, 129, 1024])
@pytest.mark.parametrize("kind", ["grid", "special"])
def test_oracle_keeps_the_sorted_middle(kind, n):
    rows = tall(kind, 33)[:n]
    u = np.sort(key(rows).view(U32) ^ U32(0x80000000), axis=0)
    for b in trims(n):
        _, interior, kL, kH = rank_trim(rows, b)
        assert np.array_equal(interior + kL + kH, np.full(33, n - 2 * b)) and kL.min() >= 1
        kept, L, H = u[b:n - b], u[b], u[n - 1 - b]  # the multiset against a plain sort
        assert np.array_equal(kL, (kept == L).sum(0)) and np.array_equal(kH, np.where(L < H, (kept == H).sum(0), 0))
        assert np.array_equal(interior, ((kept > L) & (kept < H)).sum(0))
    assert rank_trim(np.array([[5], [1], [4], [1], [2]], F32), 1)[0][0] == F32(7.0 / 3.0)  # the header's example


def test_rank_trim_of_and_the_fraction_rule():
    from pygrid_amd.exceptions import AggregationError, RankTrimUnavailableError
    from pygrid_amd.robust import RankTrim, rank_trim_count, rank_trim_of

    assert rank_trim_of({}) is None and rank_trim_of({KEY: None}) is None and rank_trim_of({KEY: False}) is None
    assert rank_trim_of({KEY: {"count": 100}}) == RankTrim(count=100) == rank_trim_of({KEY: RankTrim(count=100)})
    assert rank_trim_of({KEY: {"count": np.int64(3)}}) == RankTrim(count=3) and rank_trim_of({KEY: {"fraction": 0.1}}) == RankTrim(fraction=0.1)
    for bad in (True, 3, 0.1, "0.1", [1], {}, {"count": 1, "fraction": 0.1}, {"count": 0}, {"count": True}, {"count": 1.5},
                {"count": "2"}, {"fraction": 0}, {"fraction": 1}, {"fraction": 0.0}, {"fraction": 0.5}, {"fraction": -0.1},
                {"fraction": True}, {"fraction": "0.1"}, {"fraction": float("nan")}, {"beta": 0.1}):
        with pytest.raises(AggregationError):
            rank_trim_of({KEY: bad})
    assert rank_trim_count(RankTrim(fraction=0.1), 1000) == 100  # the decimal as written, not the double nearest it
    assert rank_trim_count(RankTrim(fraction=0.1), 15) == 2 and rank_trim_count(RankTrim(count=8), 17) == 8
    for trim, n in ((RankTrim(fraction=0.49), 3), (RankTrim(count=8), 16)):
        with pytest.raises(RankTrimUnavailableError):
            rank_trim_count(trim, n)


def test_precedence_and_combinations():
    from pygrid_amd import RANK_TRIMMED_MEAN, exceptions as X, robust
    from pygrid_amd.cycle import select_mode
    from pygrid_amd.settings import settings_of

    on = {KEY: {"fraction": 0.2}}
    rule = robust.rule_of(on)
    assert rule.mode == RANK_TRIMMED_MEAN == 9 and rule.value == robust.RankTrim(fraction=0.2) and rule.at_close
    assert len(robust.KINDS) == 4 and not issubclass(X.RankTrimUnavailableError, X.PlanNotAcceleratedError)
    assert robust.rule_of(on, rank_trim=None) is None and robust.rule_of({}, rank_trim=rule.value) == rule
    for other, err in (({"diff_trim_count": 2}, X.TrimUnavailableError), ({"diff_median": True}, X.MedianUnavailableError),
                       ({"diff_clip_norm": 1.0}, X.ClipUnavailableError), ({"dp_noise": {"multiplier": 1.0}}, X.AggregationError),
                       ({"diff_mean_around_median": {"drop": 2}}, X.MeanAroundMedianUnavailableError),
                       ({"diff_bulyan": {"byzantine": 1}}, X.MeanAroundMedianUnavailableError)):
        with pytest.raises(err):
            settings_of({**on, **other})
    s = settings_of({**on, "diff_krum": {"byzantine": 2}, "server_optimizer": {"name": "fedadam", "lr": 0.1}})
    assert s.rule == rule and s.select is not None and s.opt is not None  # a selection ahead, an optimizer behind
    assert select_mode({}, **s.rule_kwargs()) == RANK_TRIMMED_MEAN
    with pytest.raises(X.RankTrimUnavailableError):
        select_mode({}, weights=[1.0, 2.0], **s.rule_kwargs())
