"""GPU: the mean around the median (PGH_MEAN_AROUND_MEDIAN, kernel K15) and Bulyan, bit-exact against
tests/mam_oracle.py (NaNs by position).  The definition is in include/pgh_api.h and DESIGN.md section 5."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import krum_oracle as KO  # noqa: E402
import mam_oracle as MM  # noqa: E402
import serveropt_oracle as SO  # noqa: E402
from gen_trim_golden import special_rows  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MAM, STATE, UNSUPPORTED = 8, -3, -6
# K15's tiers end at 8, 16, 32 and 64 rows (one lane holds the column) and at 128, 256, 512 and 1,024
TIER_N = (2, 3, 8, 9, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024)
TIER_P = 257  # four tiles and one column


@functools.lru_cache(maxsize=None)
def tall(kind, p=TIER_P):
    """1,024 rows and a checkpoint: specials in every fifth place of every row, or a grid of integers in [-3, 3]."""
    rng = np.random.default_rng(p + len(kind))
    rows = special_rows(1024, p, 15000 + p, every=5, rows=1024) if kind == "special" else rng.integers(-3, 4, (1024, p)).astype(F)
    return rows, rng.standard_normal(p).astype(F)


def load(eng, rows, drop, slots=None, cap=None):
    eng.set_layout([rows.shape[1]])
    eng.reserve(cap or len(rows))
    eng.set_median_drop(drop)
    for k, d in enumerate(rows):
        eng.ingest(k if slots is None else int(slots[k]), d)


def close(eng, rows, ckpt, drop):
    load(eng, rows, drop)
    return eng.fedavg(MAM, ckpt)


@pytest.mark.parametrize("n", TIER_N)
def test_tiers(engine, n):
    for kind in ("special", "grid"):
        rows, ckpt = tall(kind)
        for drop in sorted({1, n // 2, n - 1}):
            _, at_e, kept_at_e, where = MM.mean_around_median(rows[:n], drop)
            cut = at_e > kept_at_e  # columns whose ties at E are only partly kept: the quota walk
            if kind == "grid" and n >= 8:
                assert cut.any(), (n, drop)
                if n > 64:  # ... and in one of them the tied rows lie in more than one block of 64
                    assert any(len(set(np.flatnonzero(where[:, c]) // 64)) > 1 for c in np.flatnonzero(cut)), (n, drop)
            assert MM.same_bits(close(engine, rows[:n], ckpt, drop), MM.fedavg(ckpt, rows[:n], drop)), (kind, n, drop)
    assert engine.effective_variant(MAM) == 60


@pytest.mark.parametrize("p", [1, 5, 4097, 2 * 65536 + 5])
def test_shapes(engine, p):
    rows, ckpt = special_rows(37, p, 5000 + p), np.random.default_rng(p).standard_normal(p).astype(F)
    assert MM.same_bits(close(engine, rows, ckpt, 5), MM.fedavg(ckpt, rows, 5))


@pytest.mark.parametrize("n", [37, 513])  # within a RowTab; a longer list, which takes the device table
def test_sources_give_the_bits_of_the_contiguous_close(engine, n):
    import torch

    rows, ckpt = tall("grid", 1000)
    rows, drop = rows[:n], n // 4
    want = close(engine, rows, ckpt, drop)
    assert MM.same_bits(want, MM.fedavg(ckpt, rows, drop))
    ck, out = torch.from_numpy(ckpt).cuda(), torch.zeros(1000, device="cuda")
    for off, ln in ((0, 260), (260, 740)):
        engine.fedavg_device_range(MAM, off, ln, ck.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    slots = np.random.default_rng(n).permutation(n + 3)[:n]  # fold position k sits in slot slots[k]
    load(engine, rows, drop, slots, cap=n + 3)
    engine.ckpt_upload(ckpt)
    engine.fold_slots_finish_resident(MAM, slots)
    assert np.array_equal(engine.ckpt_download().view(np.uint32), want.view(np.uint32))


def test_behind_fedadam(engine):
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    rows, ckpt = tall("grid")
    rows = (rows[:70] * F(1e-2)).astype(F)
    close(engine, rows, ckpt, 9)
    try:
        engine.set_server_opt(SO.ADAM, *hp.values())  # (behind the layout, which clears it)
        got = engine.fedavg(MAM, ckpt)
        want = SO.step(SO.ADAM, ckpt, MM.mean_around_median(rows, 9)[0], *SO.init_state(TIER_P, hp["tau"]), **hp)[0]
        assert SO.same_bits(got, want)
    finally:
        engine.set_server_opt(SO.NONE)


@pytest.mark.parametrize("incremental", [False, True])
def test_bulyan_end_to_end(engine, incremental):
    """7 diffs, f = 1: one hostile in a few coordinates only, one all NaN (excluded by stage 1, it counts against f)."""
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.exceptions import MeanAroundMedianUnavailableError
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.state_schema import build_state_fast, parse_state

    p, cfg = 1003, {"diff_bulyan": {"byzantine": 1}}
    rng = np.random.default_rng(7)
    diffs, ckpt = (rng.standard_normal((7, p)) * 1e-2).astype(F), rng.standard_normal(p).astype(F)
    diffs[2] = diffs[[0, 1, 3, 5, 6]].mean(0)  # central in norm ...
    diffs[2, ::600] = F(0.15)                  # ... and far off in two coordinates
    diffs[4] = np.nan
    picked = KO.krum(diffs, 1, 5)["picked"]
    want = MM.fedavg(ckpt, diffs[picked], 2)
    assert len(picked) == 5 and 2 in picked  # stage 1 keeps the hostile diff; stage 2 drops its two coordinates
    assert np.abs(ckpt - want)[::600].max() < 0.02 < np.abs(diffs[picked].mean(0))[::600].min()

    def run(n):
        if not incremental:
            return CycleAggregator(engine).average_params(cfg, [ckpt], [[d] for d in diffs[:n]])[0], None
        from pygrid_amd.settings import settings_of
        inc = IncrementalCycle(engine, [p], slots=8, checkpoint=build_state_fast([ckpt]), settings=settings_of(cfg))
        for w in range(n):
            inc.assigned(w)
            inc.reported(w, build_state_fast([diffs[w]]))
        return parse_state(inc.close(build_state_fast([ckpt])))[0], inc.last_close

    got, last = run(7)
    assert MM.same_bits(got, want)
    assert last is None or (last["mean_around_median"] == {"drop": 2, "byzantine": 1} and last["krum"]["picked"] == 5)
    with pytest.raises(MeanAroundMedianUnavailableError):
        run(6)  # n < 4 f + 3: the close fails closed


@pytest.mark.parametrize("what, status", [("n_1025", UNSUPPORTED), ("n_le_c", STATE), ("setting_off", STATE),
                                          ("stream_begin", UNSUPPORTED), ("fold_slots", UNSUPPORTED), ("dp_noise", STATE)])
def test_refusals_leave_the_context_usable(engine, what, status):
    from pygrid_amd.exceptions import AggregationError

    n = 1025 if what == "n_1025" else 9
    rows, ckpt = special_rows(n, 67, 67, rows=n), np.zeros(67, F)
    load(engine, rows, {"n_1025": 1, "n_le_c": 9, "setting_off": 0}.get(what, 2))
    try:
        if what == "dp_noise":
            engine.set_clip_norm(1.0)
            engine.set_dp_noise(1.0, 1, 1)
        with pytest.raises(AggregationError) as e:
            {"stream_begin": lambda: engine.stream_begin(MAM), "fold_slots": lambda: engine.fold_slots(MAM, [0, 1])}.get(
                what, lambda: engine.fedavg(MAM, ckpt))()
        assert e.value.status == status, e.value
    finally:
        engine.set_dp_noise(0.0)
        engine.set_clip_norm(0.0)
    assert MM.same_bits(close(engine, rows[:9], ckpt, 2), MM.fedavg(ckpt, rows[:9], 2))
