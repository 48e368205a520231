"""CPU: conditions on the inputs of tests/test_gpu_row_sums_wide.py.  The engine folds a row's tile partials in
chunks of ``clip_oracle.FOLD_CHUNK``; the GPU tests compare its sums with the oracle's as u64 bits, which proves
the chunking only if every way of getting the chunking wrong moves those bits for the rows used.  So here each
wrong fold below is computed from the oracle's own tile partials, for every row of ``wide_rows`` at every width,
and must differ from ``clip_oracle.row_sumsq`` in bits (the seeds in gen_clip_golden.py were chosen so that the
oracle alone says so).  No GPU, no product code."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import gen_clip_golden as GG  # noqa: E402
import gen_row_sums_wide_golden as GW  # noqa: E402

CH = CO.FOLD_CHUNK


def bits(x) -> int:
    return int(np.array([x], np.float64).view(np.uint64)[0])


def chunks_of(parts):
    return [parts[c0:c0 + CH] for c0 in range(0, len(parts), CH)]


def wrong_folds(parts) -> dict:
    """name -> the sum a mistaken chunk loop would give, for those mistakes the tile count lets happen: with one
    chunk only (f) is a different computation, and (c) needs two partials to add ahead of their turn."""
    fold, nt, chunks = GW.left_fold, len(parts), chunks_of(parts)
    out = {"f: the last partial is dropped": fold(parts[:-1])}
    if nt > CH:
        out["a: the last chunk is dropped"] = fold(parts[:CH * ((nt - 1) // CH)])
        out["b: only the first chunk is folded"] = fold(parts[:CH])
        out["d: acc restarts at each chunk"] = fold(chunks[-1])
        out["e: the first partial of every later chunk is skipped"] = fold(
            np.concatenate([chunks[0]] + [c[1:] for c in chunks[1:]]))
        if len(chunks[-1]) >= 2:
            out["c: a subtotal per chunk, the subtotals folded"] = fold([fold(c) for c in chunks])
    return out


def test_the_widths_are_what_the_fold_chunk_makes_them():
    assert [GG.n_tiles(p) for p in GG.WIDE_P] == [CH, CH + 2, 2 * CH + 6]
    assert GG.P_B % 4 == 1 and GG.P_B % CO.TILE == 1 and GG.P_C % CO.TILE == 3
    assert GG.WIDE_N == 5


@pytest.mark.parametrize("p", GG.WIDE_P)
def test_every_wrong_chunking_moves_the_bits(p):
    rows, sums = GG.wide_rows(p), GW.wide_sums(p)
    assert rows.shape == (GG.WIDE_N, p) and rows.dtype == np.float32
    for r in range(GG.WIDE_N):
        parts = GW.wide_partials(p)[r]
        assert parts.size == GG.n_tiles(p)
        right = bits(CO.row_sumsq(rows[r]))
        assert right == bits(sums[r])  # the cached fold of the cached partials is the oracle's
        wrong = wrong_folds(parts)
        assert len(wrong) == (1 if p == GG.P_A else 6), (p, sorted(wrong))
        for name, s in wrong.items():
            if name[0] == "c" and max(np.count_nonzero(c) for c in chunks_of(parts)) <= 1:
                # the sparse row where each chunk holds one value (P_C): a chunk's subtotal IS that value, the
                # two folds are the same additions and no input could tell them apart; rows 0..3 do there
                assert r == GG.SENTINEL and p == GG.P_C and bits(s) == right
                continue
            assert bits(s) != right, (p, r, name, float(s))
        # every chunk holds both large and small partials (rows 0..3): a k = -3 tile beside a k = 3 tile is 12
        # orders of magnitude, less 4,096 x where the large one is P_B's one-param tile and a draw's own spread
        if r != GG.SENTINEL:
            for c in chunks_of(parts):
                assert c.min() > 0 and c.max() / c.min() >= 1e6, (p, r)


@pytest.mark.parametrize("p", GG.WIDE_P)
def test_the_sparse_row(p):
    row = GG.wide_rows(p)[GG.SENTINEL]
    at = GG.sentinel_at(p)
    assert np.count_nonzero(row) == len(at) == (2 if p == GG.P_A else 3)
    tiles = sorted(i // CO.TILE for i in at)
    assert tiles == ([0, CH - 1] if p == GG.P_A else [0, CH, GG.n_tiles(p) - 1])
    s = GW.wide_sums(p)[GG.SENTINEL]
    assert s == GG.sentinel_sumsq(p) == 2.0 ** 54 + (4 if p == GG.P_A else 8)
    assert bits(s) == bits(CO.row_sumsq(row))


def test_golden_file_is_what_the_generator_writes():
    """Byte for byte; and the bits in it are the oracle's of today."""
    assert GW.GOLDEN.read_bytes() == GW.npz_bytes(GW.build())
    G = np.load(GW.GOLDEN)
    assert tuple(G["wide_p"]) == GG.WIDE_P
    for p in GG.WIDE_P:
        assert G[f"sumsq_bits_{p}"].dtype == np.uint64 and G[f"sumsq_bits_{p}"].shape == (GG.WIDE_N,)
        assert np.array_equal(G[f"sumsq_bits_{p}"], GG.bits64([CO.row_sumsq(r) for r in GG.wide_rows(p)]))
        assert bits(CO.row_sumsq(GG.wide_other(p))) == int(G[f"other_bits_{p}"][0])
        assert len(set(G[f"sumsq_bits_{p}"].tolist()) | {int(G[f"other_bits_{p}"][0])}) == GG.WIDE_N + 1
