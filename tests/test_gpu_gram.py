"""GPU: kernel K16 (k_row_gram) against longdouble dot products within the derived bound of include/pgh_api.h ("Gram
distances"), its invariances as bits, the selection through it against krum_oracle.py and the exact kind, the refusals."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import krum_oracle as KO  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
RB, TILE, LD = 128, 4096, 65536  # GRAM_RB; K7's tile = the K-chunk of a small model; the widest one-block slab row
CHILD = """import sys, numpy as np; sys.path.insert(0, sys.argv[1]); from pygrid_amd import Engine; rows = np.load(sys.argv[2] + '/rows.npy')
with Engine(int(sys.argv[3])) as e:
    e.set_layout([rows.shape[1]]); e.reserve(len(rows)); [e.ingest(k, d) for k, d in enumerate(rows)]
    np.save(sys.argv[2] + '/gram.npy', e.row_gram(list(range(len(rows)))))"""


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def load(eng, rows, slots=None, cap=None):
    eng.set_layout([rows.shape[1]])
    eng.reserve(cap or len(rows))
    for k, d in enumerate(rows):
        eng.ingest(k if slots is None else int(slots[k]), d)


def make_rows(n, p, seed=16):
    """Random normal rows; the last one 1e18, the one before it subnormal (where n leaves room)."""
    rows = np.random.default_rng(seed + 1000 * n + p).standard_normal((n, p)).astype(F)
    if n >= 2:
        rows[-1] = F(1e18) * np.sign(rows[-1])
    if n >= 3:
        rows[-2] = (rows[-2] * 1e-40).astype(F)
    return rows


def within_bound(got, rows):
    """|G - the longdouble Gram matrix| <= P 2^-53 sum |a_i| |b_i|, the right-hand side in longdouble."""
    X = rows.astype(np.longdouble)
    bound = np.longdouble(rows.shape[1]) * np.longdouble(2.0) ** -53 * (np.abs(X) @ np.abs(X).T)
    err = np.abs(got.astype(np.longdouble) - X @ X.T)
    print("largest error / bound:", float((err / bound).max()))
    return bool((err <= bound).all())


# every boundary once: the MFMA tile and the block in n; K7's tile, the chunk (one tile here) and the slab's blocks in P
@pytest.mark.parametrize("n, p", [
    pytest.param(1, 1, id="n=1,P=1"), pytest.param(2, LD + 3, id="n=2,P=ld+3"),
    pytest.param(15, TILE - 1, id="n=16-1,P=tile-1"), pytest.param(17, TILE + 1, id="n=16+1,P=tile+1"),
    pytest.param(RB - 1, TILE + 5, id="n=RB-1,P=chunk+5"), pytest.param(RB + 1, 37, id="n=RB+1,P=37")])
def test_row_gram_within_the_bound(engine, n, p):
    load(engine, rows := make_rows(n, p))
    assert p <= LD or (engine.slab()[1] < p and engine.slab()[2] > 0)  # past LD the slab is column-blocked
    got = engine.row_gram(list(range(n)))
    assert within_bound(got, rows) and np.array_equal(u64(got), u64(got.T))
    assert np.array_equal(u64(got), u64(engine.row_gram(list(range(n)))))  # a repeated call: identical bits


def test_row_gram_bits_do_not_depend_on_slots_or_batching(engine, tmp_path):
    n, p = RB + 1, TILE + 5  # three block pairs, two chunks: 256 KiB of partial blocks a block pair
    load(engine, rows := make_rows(n, p, seed=7))
    want = engine.row_gram(list(range(n)))
    slot_of = np.random.default_rng(3).permutation(n + 9)[:n]
    load(engine, rows, slot_of, cap=n + 9)
    assert np.array_equal(u64(engine.row_gram(slot_of)), u64(want))  # the device row table
    assert np.array_equal(u64(engine.row_gram(slot_of[[0, 5, 0]])), u64(want[np.ix_([0, 5, 0], [0, 5, 0])]))  # a repeated slot
    # a budget of one block pair's partials: three batches, in a fresh process (the budget is read at pgh_create)
    np.save(tmp_path / "rows.npy", rows)
    out = subprocess.run([sys.executable, "-c", CHILD, str(Path(__file__).resolve().parent.parent), str(tmp_path), os.environ.get("PGH_DEVICE", "0")],
                         env=dict(os.environ, PGH_PAIRDIST_BUDGET=str(8 * RB * RB * 2)), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and np.array_equal(u64(np.load(tmp_path / "gram.npy")), u64(want)), out.stdout + out.stderr


@pytest.mark.parametrize("m", [0, 1])
def test_krum_select_gram_is_the_reference_pick(engine, m):
    """23 independent normal rows, three far outliers, a NaN row and one holding an infinity; a close under each kind."""
    from pygrid_amd.cycle import CycleAggregator

    rows, f = np.random.default_rng(23).standard_normal((23, TILE + 5)).astype(F), 3
    for k, far in ((2, 40.0), (11, -25.0), (19, 60.0)):
        rows[k] += F(far)
    rows[7, 100], rows[15, 4000] = np.nan, np.inf
    ref = KO.krum(rows, f, m)
    sc, cut = sorted(ref["scores"]), len(ref["picked"])
    assert sc[cut] - sc[cut - 1] > 1e-6 * sc[cut]  # the condition: the kinds cannot disagree on this cut
    load(engine, rows)
    every = list(range(len(rows)))
    got = engine.krum_select(every, f, m, distances="gram")
    st = engine.krum_stats()
    assert got == ref["picked"] == engine.krum_select(every, f, m)
    assert not {7, 15, 2, 11, 19} & set(got) and (st["rows"], st["excluded"], st["picked"]) == (23, 2, cut)
    # the scores it reports are the host steps over K16's matrix and K7's sums, bit for bit
    inc = ref["included"]
    pos, scores = engine.krum_select_host(engine.gram_distances_host(engine.row_gram(inc), engine.row_sumsq(inc)), f, m)
    dropped = [scores[k] for k in range(len(inc)) if k not in pos]
    assert np.array_equal(u64([st["max_picked_score"], st["min_dropped_score"]]), u64([max(scores[pos]), min(dropped)]))
    # the picked set is equal and the fold behind it is the unchanged one: the closes are one result
    ckpt = np.random.default_rng(1).standard_normal(rows.shape[1]).astype(F)
    a, b = (CycleAggregator(engine).average_params({"diff_krum": {"byzantine": f, "keep": m or None, **kind}}, [ckpt],
                                                   [[d] for d in rows])[0] for kind in ({"distances": "gram"}, {}))
    assert np.isfinite(a).all() and np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def test_refusals_leave_the_context_usable(engine):
    from pygrid_amd import Engine
    from pygrid_amd.engine import I64
    from pygrid_amd.exceptions import AggregationError

    def refused(eng, slots):
        for fn in (eng.row_gram, lambda s: eng.krum_select(s, 1, distances="gram")):
            with pytest.raises(AggregationError) as e:
                fn(slots)
            assert e.value.status == -6, e.value  # PGH_E_UNSUPPORTED

    with Engine(devices=[0, 0]) as grp:  # a group
        load(grp, rows := make_rows(9, 200))
        refused(grp, list(range(9)))
    for setup, slots in ((lambda: (engine.set_layout([64]), engine.reserve(1025), engine.synth_fill(5, 1025)), list(range(1025))),
                         (lambda: (engine.set_layout([200]), engine.set_shard(100, 200), engine.reserve(9)), list(range(9))),
                         (lambda: (engine.set_layout([200]), engine.reserve(4, I64, 2)), [0, 1, 2])):
        try:  # more rows than PGH_KRUM_MAX_ROWS; a shard narrower than the model; an int64 slab
            setup()
            refused(engine, slots)
        finally:
            engine.set_layout([200])
        load(engine, rows)
        assert within_bound(engine.row_gram(list(range(9))), rows)
