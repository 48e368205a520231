"""GPU: kernel K19 (k_mix_rows, "Row mixing" in include/pgh_api.h) against the float64 numpy product -- bits where every
partial sum is exact, the derived bound elsewhere -- its invariances, the refusals, a ``diff_nnm`` close on both paths."""
import contextlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import median_oracle as MO  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def load(eng, rows, slots=None, cap=None):
    eng.set_layout([rows.shape[1]])
    eng.reserve(cap or 2 * len(rows))
    for k, d in enumerate(rows):
        eng.ingest(k if slots is None else int(slots[k]), d)


def read(eng, slot):  # the diff a slot holds: its plain mean against a zero checkpoint is 0 - x (this frees the slot)
    eng.ckpt_upload(np.zeros(eng.P, F))
    eng.fold_slots_finish_resident(0, [int(slot)])  # PGH_MEAN
    return -eng.ckpt_download()


def mixed(eng, X, W, src=None, dst=None, cap=None):  # X into src (0 .. n-1), mixed by W into dst (n .. n+m-1), read back
    n, m = len(X), len(W)
    src = list(range(n)) if src is None else list(src)
    dst = list(range(n, n + m)) if dst is None else list(dst)
    load(eng, X, src, cap or n + m)
    eng.mix_rows(src, dst, W)
    return np.stack([read(eng, s) for s in dst])


def exact_case(m, n, p):  # integers in [-3, 3], weights in {0, 1/8, 1/4, 1}: every product and partial sum is exact in f64
    rng = np.random.default_rng([m, n, p])
    return rng.integers(-3, 4, (n, p)).astype(F), rng.choice([0.0, 0.125, 0.25, 1.0], (m, n))


def convex_case(m, n, p):
    rng = np.random.default_rng([19, m, n, p])
    W = rng.random((m, n))
    return rng.standard_normal((n, p)).astype(F), W / W.sum(axis=1, keepdims=True)


def within_bound(got, X, W):  # 2^-24 |ref|: the one f32 rounding; 2 n 2^-52 sum |w| |x|: twice the kernel's and numpy's f64 bounds
    X64 = X.astype(np.float64)
    ref = W @ X64
    bound = 2.0 ** -24 * np.abs(ref) + 2 * X.shape[0] * 2.0 ** -52 * (np.abs(W) @ np.abs(X64))
    err = np.abs(got.astype(np.float64) - ref)
    print("largest error / bound:", float((err / bound).max()))
    return bool((err <= bound).all())


# the MFMA tile (16), the wave's sub-block (64) and the workgroup's block (128) in m, n and P; the k step (16) in n
SHAPES = [(m, n, p) for m, n in ((1, 1), (3, 5), (16, 16), (17, 15), (65, 63), (129, 130)) for p in (1, 63, 65, 257, 4099)]


@pytest.mark.parametrize("m, n, p", SHAPES + [(1024, 1024, 257)])
def test_mix_is_the_exact_product(engine, m, n, p):
    X, W = exact_case(m, n, p)
    got = mixed(engine, X, W)
    assert got.dtype == F and (got == (W @ X.astype(np.float64)).astype(F)).all()


@pytest.mark.parametrize("m, n", [(65, 63), (129, 130)])
def test_mix_within_the_bound(engine, m, n):
    X, W = convex_case(m, n, 4099)
    assert within_bound(mixed(engine, X, W), X, W)


def test_an_element_depends_on_n_and_k_alone(engine, monkeypatch):
    from pygrid_amd import Engine

    X, W = convex_case(129, 130, 4099)
    want = mixed(engine, X, W)[77]
    assert np.array_equal(mixed(engine, X, W[77:78])[0].view(np.uint32), want.view(np.uint32))  # m = 1
    monkeypatch.setenv("PGH_BLOCK_BYTES", "4096")  # a column-blocked slab; read when a context is made
    with Engine(engine.device) as e:
        got = mixed(e, X, W)[77]
        assert e.slab()[1] < 4099 and e.slab()[2] > 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the sources listed backwards, the weights' columns with them: another order of the same sum
    assert within_bound(mixed(engine, X[::-1].copy(), W[:, ::-1]), X, W)


def test_slots_anywhere_sources_untouched_and_no_nan_hidden(engine):
    X, W = exact_case(17, 15, 257)
    slot_of = np.random.default_rng(5).permutation(40)
    src, dst = slot_of[:15], slot_of[15:32]  # neither a run nor in order
    assert (mixed(engine, X, W, src, dst, cap=40) == (W @ X.astype(np.float64)).astype(F)).all()
    assert all((read(engine, s) == x).all() for s, x in zip(src, X))
    X[4], W[:, 4] = np.nan, 0.0  # IEEE: a zero weight does not hide a NaN in a listed source
    assert np.isnan(mixed(engine, X, W)).all()


@pytest.mark.parametrize("case, status", [("overlap", -1), ("duplicate", -1), ("unreserved", -1), ("rows", -6), ("group", -6)])
def test_refusals(engine, case, status):
    from pygrid_amd import Engine
    from pygrid_amd.exceptions import AggregationError

    X = exact_case(3, 5, 65)[0]
    src, dst = {"overlap": (range(5), [5, 4, 6]), "duplicate": (range(5), [5, 6, 5]), "unreserved": (range(5), [5, 6, 10]),
                "rows": (range(1025), range(1025, 1028)), "group": (range(5), [5, 6, 7])}[case]
    with Engine(devices=[engine.device, engine.device]) if case == "group" else contextlib.nullcontext(engine) as e:
        load(e, X, cap=10)
        with pytest.raises(AggregationError) as err:
            e.mix_rows(list(src), list(dst), np.zeros((3, len(src))))
        assert err.value.status == status, err.value


def nnm_reference(ckpt, rows, f):  # distances, the n - f nearest (ties: the earlier row), the mix in f64, the median
    X = rows.astype(np.float64)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    W = np.zeros_like(D)
    for i, near in enumerate(np.argsort(D, axis=1, kind="stable")[:, :len(rows) - f]):
        W[i, near] = 1.0 / (len(rows) - f)
    return MO.fedavg_median(ckpt, (W @ X).astype(F))


def test_a_close_mixes_then_takes_the_median(engine):
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.state_schema import build_state_fast, parse_state

    rng = np.random.default_rng(9)
    rows, f, cfg = rng.standard_normal((9, 257)).astype(F), 2, {"diff_nnm": {"byzantine": 2}, "diff_median": True}
    rows[3], rows[6] = rows[3] + F(40.0), rows[6] - F(25.0)  # two far outliers
    ckpt = rng.standard_normal(257).astype(F)
    want = nnm_reference(ckpt, rows, f).view(np.uint32)
    got = CycleAggregator(engine).average_params(cfg, [ckpt], [[d] for d in rows])[0]
    assert np.array_equal(np.asarray(got, F).view(np.uint32), want)
    ck_pb = build_state_fast([ckpt])
    inc = IncrementalCycle(engine, [257], slots=18, checkpoint=ck_pb, nnm=cfg["diff_nnm"], median=True)
    for w, d in enumerate(rows):
        inc.assigned(w, key=w)
        inc.reported(w, build_state_fast([d]))
    new = parse_state(inc.close(ck_pb))[0]
    assert np.array_equal(np.asarray(new, F).view(np.uint32), want)
    assert inc.last_close["nnm"] == {"byzantine": 2, "neighbours": 7, "excluded": 0}
