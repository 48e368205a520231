"""GPU: kernel K20 (k_row_gram_bf16) against numpy f64 within the bound of include/pgh_api.h ("Split-bf16 Gram"), the
exact cases, the split, hostile magnitudes, its invariances as bits, the selection and the mixing through it, the refusals."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from pygrid_amd.engine import GRAM_BF16_RUN

pytestmark = pytest.mark.gpu
F = np.float32
RB, TILE = 128, 4096  # GRAM_RB; K7's tile = the chunk of a small model
CHILD = """import sys, numpy as np; sys.path.insert(0, sys.argv[1]); from pygrid_amd import Engine; rows = np.load(sys.argv[2] + '/rows.npy')
with Engine(int(sys.argv[3])) as e:
    e.set_layout([rows.shape[1]]); e.reserve(len(rows)); [e.ingest(k, d) for k, d in enumerate(rows)]
    np.save(sys.argv[2] + '/gram.npy', e.row_gram(list(range(len(rows))), kind='bf16'))"""


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def load(eng, rows, slots=None, cap=None):
    eng.set_layout([rows.shape[1]])
    eng.reserve(cap or len(rows))
    for k, d in enumerate(rows):
        eng.ingest(k if slots is None else int(slots[k]), d)


def gram(eng, rows):
    load(eng, rows)
    return eng.row_gram(list(range(len(rows))), kind="bf16")


def bound(rows):  # ((6 R + 2) 2^-24 + P 2^-53) sum |a_i| |b_i|, in f64
    X = np.abs(rows.astype(np.float64))
    return ((6 * GRAM_BF16_RUN + 2) * 2.0 ** -24 + rows.shape[1] * 2.0 ** -53) * (X @ X.T)


def within_bound(got, rows):
    X = rows.astype(np.float64)
    err, b = np.abs(got - X @ X.T), bound(rows)
    print("largest error / bound:", float((err / np.maximum(b, 1e-300)).max()))
    return bool(np.isfinite(got).all() and (err <= b).all())


def spread_rows(n, p, seed=20):  # normal rows whose scales spread over 2^-40 .. 2^40
    rng = np.random.default_rng(seed + 1000 * n + p)
    return np.ldexp(rng.standard_normal((n, p)), rng.integers(-40, 41, (n, 1))).astype(F)


# the MFMA's k slice, K7's tile and the chunk (one tile here) in P; the tile, the wave's sub-block and the block in n
@pytest.mark.parametrize("p", [1, 31, 33, TILE - 1, TILE + 1, 2 * TILE + 5])
@pytest.mark.parametrize("n", [1, 2, RB - 1, RB + 1, 2 * RB + 1])
def test_row_gram_bf16_within_the_bound(engine, n, p):
    got = gram(engine, rows := spread_rows(n, p))
    assert within_bound(got, rows) and np.array_equal(u64(got), u64(got.T))


@pytest.mark.parametrize("n, p", [(RB + 1, 33), (2 * RB + 1, TILE), (65, TILE - 3)])
def test_small_integers_are_exact(engine, n, p):
    """All bits in h and every f32 sum exact: indexing, tiling, the masked tail and the diagonal pairs, as equality."""
    rows = np.random.default_rng(n + p).integers(-7, 8, (n, p)).astype(F)
    X = rows.astype(np.float64)
    assert np.array_equal(gram(engine, rows), X @ X.T)


@pytest.mark.parametrize("q, p", [(0, 1), (17, TILE), (TILE - 1, TILE), (TILE, TILE + 3), (2 * TILE + 2, 2 * TILE + 3)])
def test_one_product_is_six_terms(engine, q, p):
    """Rows that are zero but at param q: G[a][b] = v_a v_b from hh, hm, mh, mm, hl, lh; losing m or l misses by 2^4."""
    rng = np.random.default_rng(q)
    rows = np.zeros((33, p), F)
    rows[:, q] = np.ldexp(rng.uniform(1, 2, 33), rng.integers(-20, 21, 33)).astype(F) * rng.choice([-1, 1], 33)
    want = np.outer(rows[:, q].astype(np.float64), rows[:, q].astype(np.float64))
    err = np.abs(gram(engine, rows) - want) / np.abs(want)
    print("largest relative error * 2^24:", float(err.max() * 2 ** 24))
    assert (err <= 8 * 2.0 ** -24).all()


def test_hostile_magnitudes_stay_finite_and_unpicked(engine):
    rows = np.random.default_rng(4).standard_normal((12, TILE + 1)).astype(F)
    rows[3], rows[5] = F(1e30), np.finfo(F).max
    assert within_bound(gram(engine, rows), rows)
    every = list(range(12))
    assert not {3, 5} & set(engine.krum_select(every, 3, distances="gram_bf16"))
    engine.ingest(7, np.where(np.arange(TILE + 1) == 9, np.nan, rows[7]).astype(F))
    assert not {3, 5, 7} & set(engine.krum_select(every, 3, distances="gram_bf16")) and engine.krum_stats()["excluded"] == 1


def test_bits_do_not_depend_on_slots_batching_or_the_call(engine, tmp_path):
    n, p = RB + 1, TILE + 1  # three block pairs, two chunks
    want = gram(engine, rows := spread_rows(n, p, seed=7))
    assert np.array_equal(u64(engine.row_gram(list(range(n)), kind="bf16")), u64(want))  # a repeated call
    slot_of = np.random.default_rng(3).permutation(n + 9)[:n]
    load(engine, rows, slot_of, cap=n + 9)
    assert np.array_equal(u64(engine.row_gram(slot_of, kind="bf16")), u64(want))  # the device row table
    # a budget of one block pair's partials: three batches, in a fresh process (the budget is read at pgh_create)
    np.save(tmp_path / "rows.npy", rows)
    out = subprocess.run([sys.executable, "-c", CHILD, str(Path(__file__).resolve().parent.parent), str(tmp_path), os.environ.get("PGH_DEVICE", "0")],
                         env=dict(os.environ, PGH_PAIRDIST_BUDGET=str(8 * RB * RB * 2)), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and np.array_equal(u64(np.load(tmp_path / "gram.npy")), u64(want)), out.stdout + out.stderr


@pytest.mark.parametrize("stage", [{"diff_krum": {"byzantine": 4}}, {"diff_nnm": {"byzantine": 4}, "diff_median": True}])
def test_a_close_picks_and_mixes_as_the_exact_kind(engine, stage):
    """33 rows on a line, 29 at t = 0 .. 28 and four far ones: every cut between neighbours lies far above the bound."""
    from pygrid_amd.cycle import CycleAggregator

    rng, f = np.random.default_rng(33), 4
    t = np.concatenate([np.arange(29.0), 1000.0 + 10.0 * np.arange(4)])
    rows = (np.outer(t, rng.standard_normal(257)) + 0.01 * rng.standard_normal((33, 257))).astype(F)
    X = rows.astype(np.float64)
    D = ((X[:, None] - X[None]) ** 2).sum(axis=2)
    order = np.argsort(D, axis=1)
    D, B = np.take_along_axis(D, order, 1), np.take_along_axis(bound(rows), order, 1)  # (D = s_a + s_b - 2 G: twice G's bound)
    assert (D[:, 33 - f] - D[:, 33 - f - 1] > 100 * 2 * (B[:, 33 - f] + B[:, 33 - f - 1])).all()  # the mixing's cut, row by row
    ckpt = rng.standard_normal(257).astype(F)
    key = next(iter(stage))
    a, b = (CycleAggregator(engine).average_params({**stage, key: {**stage[key], **kind}}, [ckpt], [[d] for d in rows])[0]
            for kind in ({"distances": "gram_bf16"}, {}))
    assert np.isfinite(a).all() and np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


@pytest.mark.parametrize("case", ["group", "rows", "shard"])
def test_refusals_are_k16s(engine, case):
    from pygrid_amd import Engine
    from pygrid_amd.exceptions import AggregationError

    eng, n = (Engine(devices=[0, 0]) if case == "group" else engine), (1025 if case == "rows" else 9)
    try:  # a group; more rows than PGH_KRUM_MAX_ROWS; a shard narrower than the model
        eng.set_layout([64])
        if case == "shard":
            eng.set_shard(32, 64)
        eng.reserve(n)
        if case != "shard":
            eng.synth_fill(5, n)
        for fn in (lambda s: eng.row_gram(s, kind="bf16"), lambda s: eng.krum_select(s, 1, distances="gram_bf16")):
            with pytest.raises(AggregationError) as e:
                fn(list(range(n)))
            assert e.value.status == -6, e.value  # PGH_E_UNSUPPORTED
    finally:
        eng.close() if case == "group" else engine.set_layout([64])
    assert case == "group" or within_bound(gram(engine, rows := spread_rows(9, 64)), rows)  # the context stays usable
