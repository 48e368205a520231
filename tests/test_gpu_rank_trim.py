"""GPU: the rank-trimmed mean (PGH_RANK_TRIMMED_MEAN, kernel K17), bit-exact against the numpy restatement of its
definition in tests/test_rank_trim_logic.py (NaNs by position).  The definition is in include/pgh_api.h."""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import serveropt_oracle as SO  # noqa: E402
import test_rank_trim_logic as RT  # noqa: E402
from trim_oracle import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
RANK_TRIM, STATE, UNSUPPORTED = 9, -3, -6
TIER_N = (3, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024)  # both sides of every tier's edge
TIER_P = 257  # four tiles and one column
KINDS = ("grid", "special")
CKPT = np.random.default_rng(17).standard_normal(TIER_P).astype(F)


def load(eng, rows, b, slots=None, cap=None):
    eng.set_layout([rows.shape[1]])
    eng.reserve(cap or len(rows))
    eng.set_rank_trim(b)
    for k, d in enumerate(rows):
        eng.ingest(k if slots is None else int(slots[k]), d)


def close(eng, rows, ckpt, b):
    return load(eng, rows, b) or eng.fedavg(RANK_TRIM, ckpt)


@pytest.fixture(scope="module")
def tier_closes(engine):
    """``{(kind, n, b): the close}``: one pass per kind of input over TIER_N, the slab growing from one N to the next."""
    got = {}
    for kind in KINDS:
        rows = RT.tall(kind, TIER_P)
        engine.set_layout([TIER_P])
        engine.reserve(1024)
        have = 0
        for n in TIER_N:
            for k in range(have, n):
                engine.ingest(k, rows[k])
            have = n
            for b in RT.trims(n):
                engine.set_rank_trim(b)
                got[kind, n, b] = engine.fedavg(RANK_TRIM, CKPT)
    return got


@pytest.mark.parametrize("n", TIER_N)
@pytest.mark.parametrize("kind", KINDS)
def test_tiers(tier_closes, kind, n):
    rows = RT.tall(kind, TIER_P)[:n]
    for b in RT.trims(n):
        assert same_bits(tier_closes[kind, n, b], RT.fedavg(CKPT, rows, b)), (kind, n, b)
        if kind == "grid":  # exact sums: the rational mean of the sorted middle (no quotient of integers this small lies
            # within an f64 ulp of an f32 midpoint, so rounding it to f64 first changes nothing)
            mid = np.sort(rows.astype(np.int64), axis=0)[b:n - b].sum(0)
            exact = np.array([float(Fraction(int(t), n - 2 * b)) for t in mid]).astype(F)
            assert np.array_equal(tier_closes[kind, n, b].view(np.uint32), (CKPT - exact).astype(F).view(np.uint32)), (n, b)


@pytest.mark.parametrize("n", [9, 65])
def test_rows_that_hold_the_padding_pattern(engine, n):
    """Column c holds 0x7fffffff -- what the kernel pads places past N with -- in its last min(c, n) rows, finite
    values elsewhere: #{u <= L} counts live places only."""
    rows = np.random.default_rng(n).standard_normal((n, n + 2)).astype(F).view(np.uint32)
    for c in range(n + 2):
        rows[n - min(c, n):, c] = 0x7FFFFFFF
    rows, ckpt = rows.view(F), np.zeros(n + 2, F)
    assert same_bits(close(engine, rows, ckpt, 1), RT.fedavg(ckpt, rows, 1))


@pytest.mark.parametrize("n", [65, 600])  # within a RowTab; a longer list, which takes the device table
def test_scattered_slots_give_the_bits_of_the_contiguous_close(engine, n):
    rows, b = RT.tall("special", TIER_P)[:n], n // 10
    want = close(engine, rows, CKPT, b)
    assert same_bits(want, RT.fedavg(CKPT, rows, b))
    slots = np.random.default_rng(n).permutation(n + 3)[:n]  # fold position k sits in slot slots[k]
    load(engine, rows, b, slots, cap=n + 3)
    engine.ckpt_upload(CKPT)
    engine.fold_slots_finish_resident(RANK_TRIM, slots)
    assert same_bits(engine.ckpt_download(), want)


@pytest.mark.parametrize("what, status", [("setting_off", STATE), ("n_2b", STATE), ("n_1025", UNSUPPORTED), ("fold_slots", UNSUPPORTED)])
def test_refusals_leave_the_context_usable(engine, what, status):
    from pygrid_amd.exceptions import AggregationError

    n = 1025 if what == "n_1025" else 8
    rows, ckpt = np.random.default_rng(8).standard_normal((n, 67)).astype(F), np.zeros(67, F)
    load(engine, rows, {"setting_off": 0, "n_2b": 4}.get(what, 2))
    assert engine.effective_variant(RANK_TRIM) == 70
    with pytest.raises(AggregationError) as e:
        engine.fold_slots(RANK_TRIM, [0, 1]) if what == "fold_slots" else engine.fedavg(RANK_TRIM, ckpt)
    assert e.value.status == status, e.value
    assert same_bits(close(engine, rows[:8], ckpt, 3), RT.fedavg(ckpt, rows[:8], 3))


def test_behind_fedadam(engine):
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    rows = (RT.tall("grid", TIER_P)[:17] * F(1e-2)).astype(F)
    close(engine, rows, CKPT, 4)
    try:
        engine.set_server_opt(SO.ADAM, *hp.values())  # (behind the layout, which clears it)
        want = SO.step(SO.ADAM, CKPT, RT.rank_trim(rows, 4)[0], *SO.init_state(TIER_P, hp["tau"]), **hp)[0]
        assert SO.same_bits(engine.fedavg(RANK_TRIM, CKPT), want)
    finally:
        engine.set_server_opt(SO.NONE)


@pytest.mark.parametrize("incremental", [False, True])
def test_fraction_from_server_config(engine, incremental):
    """``{"fraction": 0.2}`` resolves at the close: b = 4 of 17 diffs, 3 of the 11 that a Multi-Krum stage keeps."""
    import krum_oracle as KO
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.exceptions import RankTrimUnavailableError
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.settings import settings_of
    from pygrid_amd.state_schema import build_state_fast, parse_state

    diffs = (RT.tall("grid", 1003)[:17] * F(1e-2)).astype(F)
    ckpt = np.random.default_rng(3).standard_normal(1003).astype(F)

    def run(cfg, n):
        if not incremental:
            return CycleAggregator(engine).average_params(cfg, [ckpt], [[d] for d in diffs[:n]])[0]
        inc = IncrementalCycle(engine, [1003], slots=18, checkpoint=build_state_fast([ckpt]), settings=settings_of(cfg))
        for w in range(n):
            inc.assigned(w)
            inc.reported(w, build_state_fast([diffs[w]]))
        return parse_state(inc.close(build_state_fast([ckpt])))[0]

    cfg = {"diff_trimmed_mean": {"fraction": 0.2}}
    assert same_bits(run(cfg, 17), RT.fedavg(ckpt, diffs, 4))
    picked = KO.krum(diffs, 3, 11)["picked"]
    assert same_bits(run({**cfg, "diff_krum": {"byzantine": 3, "keep": 11}}, 17), RT.fedavg(ckpt, diffs[picked], 3))
    with pytest.raises(RankTrimUnavailableError):  # N < 2b + 1: the close fails closed
        run({"diff_trimmed_mean": {"count": 2}}, 4)
