"""CPU: the mean around the median -- the oracle's hand pin, its golden file and scalar restatement, the proof that
the inputs of the GPU tests tell wrong variants of the definition apart, the parsers of ``diff_mean_around_median`` and
``diff_bulyan``, the Bulyan expansion and its refusals."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_mam_golden as GM  # noqa: E402
import mam_oracle as MM  # noqa: E402
import median_oracle as MO  # noqa: E402
import trim_oracle as TO  # noqa: E402
from pygrid_amd.exceptions import AggregationError, MeanAroundMedianUnavailableError  # noqa: E402
from pygrid_amd.krum import KrumSpec, select  # noqa: E402
from pygrid_amd.robust import MAM_KEY  # noqa: E402
from pygrid_amd.settings import BULYAN_KEY, settings_of  # noqa: E402


F32, F64, U32 = np.float32, np.float64, np.uint32


def test_hand_pin():
    """(1, 2, 4, 5), c = 1: m = 3, distances (2, 1, 1, 2); positions 1, 2 and 0 are kept (0 wins the tie over 3)."""
    mean, at_e, kept_at_e, _ = MM.mean_around_median(np.array([[1], [2], [4], [5]], np.float32), 1)
    assert mean.dtype == np.float32 and mean[0] == np.float32(7.0 / 3.0) and (at_e[0], kept_at_e[0]) == (2, 1)
    assert MM.fedavg([10.0], [[1], [2], [4], [5]], 1)[0] == np.float32(10.0) - np.float32(7.0 / 3.0)


@pytest.fixture(scope="module")
def G():
    return np.load(GM.GOLDEN)


def test_golden_file_pins_the_oracle_and_the_scalar_restatement_agrees(G):
    assert [tuple(c) for c in G["cases"]] == list(GM.CASES)
    for n, c in GM.CASES:
        rows, ckpt = GM.columns(n)
        assert np.array_equal(G[f"diffs_{n}"].view(U32), rows.view(U32)) and np.array_equal(G[f"ckpt_{n}"].view(U32), ckpt.view(U32))
        mean, _, kept_at_e, _ = MM.mean_around_median(rows, c)
        assert MM.same_bits(MM.fedavg(ckpt, rows, c), G[f"out_{n}"]) and np.array_equal(kept_at_e, G[f"kept_{n}"]), (n, c)
        mean_s, kept_s = MM.mean_around_median_scalar(rows, c)
        assert MM.same_bits(mean_s, mean) and np.array_equal(kept_s, kept_at_e), (n, c)
        assert not np.isfinite(mean[GM.COLS["nonfinite"]]).all()  # (the non-finite medians are in the pinned cases)


def test_nan_payload_case_tells_whose_payload_a_difference_of_nans_carries(G):
    d, ckpt, c = GM.nan_payload_case()
    assert MO.median_of_rows(d).view(U32).tolist() == [GM.PNAN] * d.shape[1]
    x_wins, m_wins = GM.nan_payload_out("x"), GM.nan_payload_out("m")
    assert np.isfinite(x_wins).all() and np.isnan(m_wins).all()
    assert MM.same_bits(G["out_nan"], MM.fedavg(ckpt, d, c)) and np.array_equal(G["diffs_nan"].view(U32), d.view(U32))
    assert MM.same_bits(MM.mean_around_median_scalar(d, c)[0], MM.mean_around_median(d, c)[0])


def variant(ckpt, d, drop, *, later=False, block=64, acc=F64, div32=False, lower=False, mask=True, keep=0, ftz=False):
    """The definition with one step changed (every default: the definition itself, written once more)."""
    d = np.asarray(d, F32)
    n, beta = d.shape[0], d.shape[0] - drop + keep
    with np.errstate(all="ignore"):
        m = TO.unkey(np.sort(TO.key(d).reshape(d.shape), axis=0)[(n - 1) // 2]) if lower else MO.median_of_rows(d)
        diff = (d - m[None, :]).astype(F32)
        if ftz:
            diff = np.where(np.abs(diff) < np.finfo(F32).tiny, np.copysign(F32(0), diff), diff)
        e = diff.view(U32) & U32(0x7FFFFFFF if mask else 0xFFFFFFFF)
        order = n - 1 - np.argsort(e[::-1], axis=0, kind="stable") if later else np.argsort(e, axis=0, kind="stable")
        kept = np.zeros(d.shape, bool)
        np.put_along_axis(kept, order[:beta], True, axis=0)
        S = None
        for g in range(0, n, block or n):
            s = np.zeros(d.shape[1], acc)
            for k in range(g, min(n, g + (block or n))):
                s = np.where(kept[k], (s + d[k].astype(acc)).astype(acc), s)
            S = s if S is None else (S + s).astype(acc)
        mean = (S.astype(F32) / F32(beta)).astype(F32) if div32 else (S.astype(F64) / F64(beta)).astype(F32)
        return (np.asarray(ckpt, F32) - mean).astype(F32)


# name: (the changed step, whether (N, beta) can tell it from the definition at all).  A sum of one value has no
# order and no rounding, and x / 1 is x: the sum's variants need beta >= 2, its orders three addends.  At N = 65
# the second block is one position and s_0 + (0.0 + x) = s_0 + x, so a plain fold needs N >= 66 and blocks of 128
# N >= 129.  keep - 1 needs a value left.  The one value kept of an odd N is the median itself, at the distance +0,
# the smallest key with the mask and without it.
MUTANTS = {
    "ties_to_the_later_position": (dict(later=True), lambda n, beta: True),
    "plain_left_fold": (dict(block=None), lambda n, beta: n >= 66 and beta >= 3),
    "blocks_of_128": (dict(block=128), lambda n, beta: n >= 129 and beta >= 3),
    "f32_accumulation": (dict(acc=F32), lambda n, beta: beta >= 2),
    "f32_division": (dict(div32=True), lambda n, beta: beta >= 2),
    "lower_middle_of_an_even_n": (dict(lower=True), lambda n, beta: n % 2 == 0),
    "distance_key_without_the_mask": (dict(mask=False), lambda n, beta: beta >= 2 or n % 2 == 0),
    "keep_one_more": (dict(keep=1), lambda n, beta: True),
    "keep_one_less": (dict(keep=-1), lambda n, beta: beta >= 2),
    "flushed_difference": (dict(ftz=True), lambda n, beta: True),
}


def test_the_gpu_tests_run_columns_at_these_row_counts_only():
    assert set(GM.TIER_N) | set(GM.OTHER_N) | {n for n, _ in GM.CASES} == set(GM.N_USED)
    assert GM.drops_used(129) == [1, 64, 128] and GM.drops_used(70) == [1, 9, 35, 69] and GM.drops_used(130) == [1, 65, 129]


@pytest.mark.parametrize("n", GM.N_USED)
def test_every_wrong_variant_shows_in_some_column(n):
    """A condition on ``columns(n)``, not on the kernel: it is what makes bit-equal GPU results mean something.
    Every (N, drop) a GPU test or a golden case runs ``columns`` with.  The two orders of the sum must show in the
    order column built for the drop (1 or N // 2), not somewhere by chance."""
    rows, ckpt = GM.columns(n)
    unseen = []
    for drop in GM.drops_used(n):
        want = MM.fedavg(ckpt, rows, drop)
        assert np.array_equal(variant(ckpt, rows, drop).view(U32), want.view(U32))
        for name, (change, applies) in MUTANTS.items():
            if not applies(n, n - drop):
                continue
            got = variant(ckpt, rows, drop, **change)
            if name in ("plain_left_fold", "blocks_of_128") and drop in (1, n // 2):
                col = GM.COLS["order"][0 if drop == 1 else 1]
                got, want_here = got[col:col + 1], want[col:col + 1]
            else:
                want_here = want
            if MM.same_bits(got, want_here):
                unseen.append((name, n, drop))
    assert not unseen


@pytest.mark.parametrize("n", GM.N_USED)
def test_every_prefix_has_every_kind_of_column(n):
    rows, _ = GM.columns(n)
    u, m = rows.view(U32), MO.median_of_rows(rows)
    s = np.sort(TO.key(rows).reshape(rows.shape), axis=0)
    if n % 2 == 0:  # even-N middles that differ, both finite: 0.5 a + 0.5 b lies between them
        a, b = TO.unkey(s[n // 2 - 1]), TO.unkey(s[n // 2])
        assert (np.isfinite(a) & np.isfinite(b) & (a < m) & (m < b)).any()
        assert np.isnan(m[GM.COLS["inf_middles"][0]]) and np.isinf(rows[:, GM.COLS["inf_middles"][0]]).all()
    for i, bits in enumerate(GM.SPECIALS):  # a non-finite median of each kind, finite rows at both ends from N = 4
        cols = [c for c in GM.COLS["nonfinite"][4 * i:4 * i + 4]
                if (np.isnan(m[c]) and m.view(U32)[c] >> 31 == bits >> 31 if bits in (GM.PNAN, GM.NNAN) else m.view(U32)[c] == bits)
                and set(u[~np.isfinite(rows[:, c]), c]) == {bits}
                and (n < 4 or (np.isfinite(rows[0, c]) and np.isfinite(rows[n - 1, c])))]
        assert cols, (n, hex(bits))
    sub = rows[:, GM.COLS["subnormal"]]
    assert (sub > 0).all() and (sub < np.finfo(F32).tiny).all() and (m[GM.COLS["subnormal"]] < np.finfo(F32).tiny).all()
    for drop in GM.drops_used(n):
        _, at_e, kept_at_e, where = MM.mean_around_median(rows, drop)
        cut = at_e > kept_at_e  # columns whose ties at E are only partly kept: the quota walk
        if n >= 8:
            assert cut[GM.COLS["grid"]].any(), (n, drop)
            if n > 64:  # ... and in one of them the tied rows lie in more than one block of 64
                assert any(len(set(np.flatnonzero(where[:, c]) // 64)) > 1 for c in np.flatnonzero(cut)), (n, drop)
        if n >= 66 and drop in (1, n // 2):  # both powers of two are kept, the largest kept values, and odd integers after the second
            col = GM.COLS["order"][0 if drop == 1 else 1]
            e = (rows[:, col] - m[col]).view(U32) & U32(0x7FFFFFFF)
            kept = np.argsort(e, kind="stable")[:n - drop]
            assert set(GM.BIG_AT) <= set(kept) and (kept > GM.BIG_AT[1]).sum() >= 1 and np.abs(rows[kept, col]).max() == 2.0 ** 62


@pytest.mark.parametrize("key, field", [(MAM_KEY, "drop"), (BULYAN_KEY, "byzantine")])
@pytest.mark.parametrize("value, ok", [(1, True), (3.0, True), (np.int64(2), True), (0, False), (-1, False), (True, False),
                                       (1.5, False), ("1", False), (None, False), (float("nan"), False)])
def test_parsers(key, field, value, ok):
    if not ok:
        with pytest.raises(AggregationError):
            settings_of({key: {field: value}})
        return
    s = settings_of({key: {field: value}})
    assert s.rule.key == MAM_KEY and s.rule.value == int(value) * (2 if key == BULYAN_KEY else 1)
    assert (s.bulyan, s.select) == ((int(value), KrumSpec(int(value), None, True)) if key == BULYAN_KEY else (None, None))


@pytest.mark.parametrize("key, field", [(MAM_KEY, "drop"), (BULYAN_KEY, "byzantine")])
@pytest.mark.parametrize("cfg", [True, 1, "x", [1], {}, {"count": 1}, "extra"])
def test_parsers_refuse_other_shapes(key, field, cfg):
    with pytest.raises(AggregationError):
        settings_of({key: {field: 1, "extra": 1} if cfg == "extra" else cfg})
    assert not settings_of({key: None}) and not settings_of({key: False})


@pytest.mark.parametrize("other", [{"diff_krum": {"byzantine": 1}}, {"diff_median": True}, {"diff_trim_count": 1},
                                   {MAM_KEY: {"drop": 2}}, {"diff_clip_norm": 1.0, "dp_noise": {"multiplier": 1.0}},
                                   {"diff_trust_root": True}])
def test_bulyan_stands_alone(other):
    with pytest.raises(MeanAroundMedianUnavailableError):
        settings_of({BULYAN_KEY: {"byzantine": 1}, **other})


def test_bulyan_stage_one_keeps_n_minus_2f_of_at_least_4f_plus_3():
    class Eng:
        def krum_select(self, slots, f, keep):
            return slots[:keep]

    spec = settings_of({BULYAN_KEY: {"byzantine": 2}}).select
    assert select(Eng(), spec, list(range(11))) == list(range(7))
    with pytest.raises(MeanAroundMedianUnavailableError):
        select(Eng(), spec, list(range(10)))
