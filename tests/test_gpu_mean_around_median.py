"""GPU: the mean around the median (PGH_MEAN_AROUND_MEDIAN, kernel K15) and Bulyan, bit-exact against
tests/mam_oracle.py and the golden file tests/golden/mam_cases.npz (NaNs by position).  The definition is in
include/pgh_api.h and DESIGN.md section 5; tests/test_mean_around_median_logic.py proves without a GPU that the inputs
of ``gen_mam_golden.columns`` tell wrong variants of the definition apart at every N and drop used here."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_mam_golden as GM  # noqa: E402
import krum_oracle as KO  # noqa: E402
import mam_oracle as MM  # noqa: E402
import serveropt_oracle as SO  # noqa: E402
from gen_trim_golden import special_rows  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MEAN, MAM, STATE, UNSUPPORTED = 0, 8, -3, -6
# K15's tiers end at 8, 16, 32 and 64 rows (one lane holds the column) and at 128, 256, 512 and 1,024 (2, 4, 8
# and 16 waves share it).  The tuple holds each tier's last row count and the two beside it from 8 on (so every
# tier, <1, 32> included, runs at its smallest and its largest N), and 2, 3 and 7 rows below the first edge.
TIER_N = GM.TIER_N
TIER_P = 257  # four tiles and one column
TIER_KINDS = ("special", "grid", "columns")
assert TIER_N == (2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GM.GOLDEN)


def make_engine(**env):
    """A context of its own: PGH_BLOCK_BYTES is read when a context is made."""
    from pygrid_amd import Engine

    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return Engine(int(os.environ.get("PGH_DEVICE", "0")))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@functools.lru_cache(maxsize=None)
def tall(kind, p=TIER_P):
    """1,024 rows and a checkpoint: specials in every fifth place of every row, a grid of integers in [-3, 3], or
    the built columns of tests/gen_mam_golden.py."""
    if kind == "columns":
        assert p == GM.P
        return GM.columns(1024)
    rng = np.random.default_rng(p + len(kind))
    rows = special_rows(1024, p, 15000 + p, every=5, rows=1024) if kind == "special" else rng.integers(-3, 4, (1024, p)).astype(F)
    return rows, rng.standard_normal(p).astype(F)


@functools.lru_cache(maxsize=None)
def wide(n, p):
    """``columns(n)`` side by side up to p columns, its checkpoint and, by drop, the expected close: the rule is
    column-wise, so the oracle runs on 257 columns.  257 is odd: every kind of column meets every lane and block edge."""
    assert n in GM.OTHER_N  # the row counts at which the CPU test proves the columns at drop = N // 2, which the callers use
    rows, ckpt = GM.columns(n)
    reps = -(-p // GM.P)
    rows, ckpt = np.ascontiguousarray(np.tile(rows, (1, reps))[:, :p]), np.tile(ckpt, reps)[:p].copy()

    @functools.lru_cache(maxsize=None)
    def want(drop):
        return np.tile(MM.fedavg(*GM.columns(n)[::-1], drop), reps)[:p].copy()

    return rows, ckpt, want


def load(eng, rows, drop, slots=None, cap=None):
    eng.set_layout([rows.shape[1]])
    eng.reserve(cap or len(rows))
    eng.set_median_drop(drop)
    for k, d in enumerate(rows):
        eng.ingest(k if slots is None else int(slots[k]), d)


def close(eng, rows, ckpt, drop):
    load(eng, rows, drop)
    return eng.fedavg(MAM, ckpt)


@pytest.fixture(scope="module")
def tier_closes(engine):
    """``{(kind, n, drop): (the close, the variant reported)}``: one pass per kind of input over TIER_N, the slab
    growing from one N to the next (not 1,024 fresh ingests per N)."""
    got = {}
    for kind in TIER_KINDS:
        rows, ckpt = tall(kind)
        engine.set_layout([TIER_P])
        engine.reserve(1024)
        have = 0
        for n in TIER_N:
            for k in range(have, n):
                engine.ingest(k, rows[k])
            have = n
            for drop in sorted({1, n // 2, n - 1}):
                engine.set_median_drop(drop)
                got[kind, n, drop] = engine.fedavg(MAM, ckpt), engine.effective_variant(MAM)
    return got


@pytest.mark.parametrize("n", TIER_N)
def test_tiers(tier_closes, n):
    for kind in TIER_KINDS:
        rows, ckpt = tall(kind)
        for drop in sorted({1, n // 2, n - 1}):
            _, at_e, kept_at_e, where = MM.mean_around_median(rows[:n], drop)
            cut = at_e > kept_at_e  # columns whose ties at E are only partly kept: the quota walk
            if kind == "grid" and n >= 8:
                assert cut.any(), (n, drop)
                if n > 64:  # ... and in one of them the tied rows lie in more than one block of 64
                    assert any(len(set(np.flatnonzero(where[:, c]) // 64)) > 1 for c in np.flatnonzero(cut)), (n, drop)
            got, variant = tier_closes[kind, n, drop]
            assert variant == 60
            assert MM.same_bits(got, MM.fedavg(ckpt, rows[:n], drop)), (kind, n, drop)


def test_golden_cases(engine, G):
    """The pinned cases from a contiguous slab: non-finite medians, the sum's order, subnormal distances."""
    for n, c in GM.CASES:
        ckpt, rows, want = G[f"ckpt_{n}"], G[f"diffs_{n}"], G[f"out_{n}"]
        assert MM.same_bits(MM.fedavg(ckpt, rows, c), want)
        assert MM.same_bits(close(engine, rows, ckpt, c), want), (n, c)


@pytest.mark.parametrize("n", [8, 9, 16, 32, 64, 128, 256, 512, 1024])  # each of the eight tiers; 9 is the pinned case
def test_nan_payloads(engine, G, n):
    """A +NaN median among NaN rows of three payloads: whether the finite rows are kept hangs on the payload that
    the difference of two NaNs carries (tests/gen_mam_golden.py: x_k's, quieted: a finite result; m's: NaN).  Each
    tier is code of its own, and the 16-wave one subtracts at every read."""
    rows, ckpt, c = GM.nan_payload_case(n)
    want = MM.fedavg(ckpt, rows, c)
    assert MM.same_bits(want, GM.nan_payload_out("x", n)) and np.isnan(GM.nan_payload_out("m", n)).all() and np.isfinite(want).all()
    if n == 9:
        assert np.array_equal(u32(G["diffs_nan"]), u32(rows)) and MM.same_bits(G["out_nan"], want)
    got = close(engine, rows, ckpt, c)
    print("nan payload case, n =", n, ": finite outputs", int(np.isfinite(got).sum()), "of", got.size)
    assert MM.same_bits(got, want)


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


@pytest.mark.parametrize("n", [37, 513])
def test_permuted_fold_order(engine, n):
    """Ties go to the earlier fold position and the sum follows fold order: the slot list's order is the fold
    order, wherever the rows lie.  One more slot holds a stale all-NaN diff that is not listed."""
    rows, ckpt = GM.columns(n)
    rng = np.random.default_rng(n)
    assert n in GM.OTHER_N  # (drop = N // 2: a drop that the built columns serve, as the CPU test proves)
    drop, order, slot_of = n // 2, rng.permutation(n), rng.permutation(n + 4)[:n + 1]
    want = MM.fedavg(ckpt, rows[order], drop)
    assert not MM.same_bits(want, MM.fedavg(ckpt, rows, drop))
    load(engine, np.concatenate([rows, np.full((1, GM.P), np.nan, F)]), drop, slot_of, cap=n + 4)
    engine.ckpt_upload(ckpt)
    engine.fold_slots_finish_resident(MAM, slot_of[order])
    assert MM.same_bits(engine.ckpt_download(), want)


@pytest.mark.parametrize("block_bytes", ["4096", "0"])
def test_narrow_blocks_and_one_block(block_bytes):
    """PGH_BLOCK_BYTES=4096 (blocks of 1,024 columns) and =0 (plain row-major rows), a context each; 37 rows in
    one wave, 130 in a four-wave tile that crosses block edges; contiguous and scattered slots."""
    p = 2 * 65536 + 5
    with make_engine(PGH_BLOCK_BYTES=block_bytes) as e:
        for n in (37, 130):
            rows, ckpt, want = wide(n, p)
            drop = n // 2
            load(e, rows, drop)
            ld, pitch = e.slab()[1:]
            assert (ld == 1024 and pitch > 0) if block_bytes == "4096" else (ld >= p and pitch == 0)
            assert e.effective_variant(MAM) == 60
            assert MM.same_bits(e.fedavg(MAM, ckpt), want(drop)), (block_bytes, n)
            slots = np.random.default_rng(n).permutation(n + 3)[:n]
            load(e, rows, drop, slots, cap=n + 3)
            e.ckpt_upload(ckpt)
            e.fold_slots_finish_resident(MAM, slots)
            assert MM.same_bits(e.ckpt_download(), want(drop)), (block_bytes, n, "scattered")


@pytest.mark.parametrize("n, drop_first", [(9, True), (130, False)])
def test_group_and_shard_match_one_context(engine, n, drop_first):
    """A shard and a two-child group give the single context's bits (nothing in the rule looks along a row).
    pgh_set_shard clears the drop count; a group's reserve, which lays its children out again, keeps it."""
    from pygrid_amd import Engine
    from pygrid_amd.exceptions import AggregationError

    p, drop = 70001, n // 2
    rows, ckpt, want = wide(n, p)
    try:
        one = close(engine, rows, ckpt, drop)
        assert MM.same_bits(one, want(drop))
        lo, hi = 35000, p
        engine.set_layout([p])
        engine.set_median_drop(drop)
        engine.set_shard(lo, hi)
        engine.reserve(n)
        for k, d in enumerate(rows):
            engine.ingest(k, d[lo:hi])
        with pytest.raises(AggregationError) as err:  # the setting went with the shard
            engine.fedavg(MAM, ckpt[lo:hi])
        assert err.value.status == STATE
        engine.set_median_drop(drop)
        assert np.array_equal(u32(engine.fedavg(MAM, ckpt[lo:hi])), u32(one[lo:hi]))
    finally:
        engine.set_layout([p])
    with Engine(devices=[0, 0]) as grp:
        grp.set_layout([p])
        if drop_first:
            grp.set_median_drop(drop)
        grp.reserve(n + 2)
        if not drop_first:
            grp.set_median_drop(drop)
        for k, d in enumerate(rows):
            grp.ingest(k, d)
        assert grp.effective_variant(MAM) == 60
        assert np.array_equal(u32(grp.fedavg(MAM, ckpt)), u32(one))
        grp.ckpt_upload(ckpt)
        grp.fedavg_resident(MAM)
        assert np.array_equal(u32(grp.ckpt_download()), u32(one))
        grp.ckpt_upload(ckpt)
        grp.fold_slots_finish_resident(MAM, list(range(n)))
        assert np.array_equal(u32(grp.ckpt_download()), u32(one))


@pytest.mark.parametrize("n", [9, 130])
def test_accounted_bytes_and_repeated_closes(engine, n):
    """K15 reads the slab once: one timed launch of 4 N P + 8 P bytes.  A second close gives the same bits, and
    pgh_set_variant reaches neither the variant nor the bits."""
    p, drop = 4097, n // 2
    rows, ckpt, want = wide(n, p)
    load(engine, rows, drop)
    engine.reset_stats()
    first = engine.fedavg(MAM, ckpt)
    st = engine.stats()
    assert st["kernel_launches"] == 1 and st["kernel_bytes_last"] == st["kernel_bytes_total"] == 4 * n * p + 8 * p
    assert MM.same_bits(first, want(drop))
    assert np.array_equal(u32(engine.fedavg(MAM, ckpt)), u32(first))
    try:
        engine.set_variant(13)
        assert engine.effective_variant(MAM) == 60
        assert np.array_equal(u32(engine.fedavg(MAM, ckpt)), u32(first))
    finally:
        engine.set_variant(-1)


def test_robust_where_the_mean_is_not(engine):
    """5 hostile rows of 11, c = 5: the six kept values are the honest ones, so the result is finite and inside
    the honest rows' range in every column; the plain mean of the same slab is not finite."""
    n, bad, p = 11, 5, 1001
    rng = np.random.default_rng(11)
    diffs = rng.standard_normal((n, p)).astype(F)
    hostile = rng.permutation(n)[:bad]
    diffs[hostile] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F), size=(bad, p))
    good = np.delete(diffs, hostile, axis=0)
    ckpt = rng.standard_normal(p).astype(F)
    got = close(engine, diffs, ckpt, bad)
    mean = MM.mean_around_median(diffs, bad)[0]
    assert MM.same_bits(got, MM.fedavg(ckpt, diffs, bad)) and np.isfinite(got).all()
    assert np.all(mean >= good.min(0)) and np.all(mean <= good.max(0)) and np.array_equal(u32(got), u32(ckpt - mean))
    assert not np.isfinite(engine.fedavg(MEAN, ckpt)).all()


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
