"""Writes tests/golden/clip_cases.npz: inputs, sums of squares (as u64 bit patterns), scales and
outputs of the small clipped-FedAvg cases, as tests/clip_oracle.py computed them when the definition
 was written.  Both test files load the file, so a later edit of the oracle
cannot move the definition unnoticed.  Run from the repository root:

    python tests/gen_clip_golden.py

Only when the definition itself changes (the oracle and this file together)."""
from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import clip_oracle as CO  # noqa: E402

F = np.float32
GOLDEN = ROOT / "tests" / "golden" / "clip_cases.npz"

SUMSQ_P = (1, 3, 63, 64, 65, 4095, 4096, 4097, 8197, 70001)
STORED_P_MAX = 8197  # the rows of larger cases are regenerated (mixed_rows), only their sums are stored
FOLD_P, FOLD_C = 8197, 10.0
FOLD_M = (0.01, 0.02, 5, 0.01, 40, 0.03, 0.5)


def mixed_rows(p: int, n: int = 3) -> np.ndarray:
    """n rows of p floats of mixed magnitude (1e-3 .. 1e3 per element)."""
    rng = np.random.default_rng(7000 + p)
    return (rng.standard_normal((n, p)) * 10.0 ** rng.integers(-3, 4, (n, p))).astype(F)


# The widths at which a row's tile partials fill more than one chunk of the engine's fold (clip_oracle's
# docstring says why these three); tests/gen_row_sums_wide_golden.py pins their sums, not this file's main().
CH = CO.FOLD_CHUNK
P_A = CH * CO.TILE
P_B = (CH + 2) * CO.TILE - (CO.TILE - 1)
P_C = 2 * CH * CO.TILE + 5 * CO.TILE + 3
WIDE_P = (P_A, P_B, P_C)
assert WIDE_P == (4_194_304, 4_198_401, 8_409_091)
WIDE_N = 5  # one K7 row group of 4 and a remainder of 1; one K12 row chunk
WIDE_GAIN = (1.0, 0.01, 3.0, 0.001)  # per random row, so that one bound clips some rows and not others
# chosen so that tests/test_row_sums_wide.py holds: the oracle alone tells every wrong chunking from the right one
WIDE_SEED = {P_A: 91000, P_B: 91025, P_C: 91009}
SENTINEL = WIDE_N - 1  # the sparse row
SENTINEL_BIG, SENTINEL_SMALL = 2.0 ** 27, 1.5  # squares 2**54 (one ulp is 4 there) and 2.25


def n_tiles(p: int) -> int:
    return -(-p // CO.TILE)


def sentinel_at(p: int) -> dict:
    """index -> value of the sparse row: 2**27 in tile 0, 1.5 in tile 1,024 (the first tile of the fold's second
    chunk, where the width has one) and 1.5 in the row's last param."""
    at = {5: SENTINEL_BIG, p - 1: SENTINEL_SMALL}
    if n_tiles(p) > CH:
        at[CH * CO.TILE + 777] = SENTINEL_SMALL
    return at


def sentinel_sumsq(p: int) -> float:
    """The sparse row's sum in the definition's order, by hand: 2**54 + 2.25 rounds up to 2**54 + 4 and that
    + 2.25 to 2**54 + 8.  (Not the real sum, 2**54 + 4.5: folding 2.25 + 2.25 first gives 2**54 + 4, folding
    without either 2.25 gives 2**54 + 4 or 2**54.)"""
    return 2.0 ** 54 + 4.0 * (len(sentinel_at(p)) - 1)


@functools.lru_cache(maxsize=None)
def wide_rows(p: int) -> np.ndarray:
    """WIDE_N rows of p floats (cached, read-only).  Rows 0..3: standard normals scaled per tile by 10**k, k drawn
    from -3..3, times the row's WIDE_GAIN; every fold chunk of two or more tiles opens with a k = -3 tile followed
    by a k = 3 tile, so each chunk holds large and small partials.  Row 4: sentinel_at(p), zero elsewhere."""
    rng = np.random.default_rng(WIDE_SEED[p])
    nt = n_tiles(p)
    rows = np.zeros((WIDE_N, p), F)
    for r, gain in enumerate(WIDE_GAIN):
        k = rng.integers(-3, 4, nt)
        for c0 in range(0, nt - 1, CH):
            k[c0], k[c0 + 1] = -3, 3
        rows[r] = (rng.standard_normal(p) * np.repeat(gain * 10.0 ** k, CO.TILE)[:p]).astype(F)
    for i, x in sentinel_at(p).items():
        rows[SENTINEL, i] = x
    rows.setflags(write=False)
    return rows


def wide_other(p: int) -> np.ndarray:
    """Another row of that width, for a second ingest into a slot."""
    return (wide_rows(p)[0][::-1] * F(3)).astype(F)


def fold_inputs():
    rng = np.random.default_rng(8197)
    ckpt = rng.standard_normal(FOLD_P).astype(F)
    diffs = np.stack([(rng.standard_normal(FOLD_P) * m).astype(F) for m in FOLD_M])
    return ckpt, diffs


def boundary_inputs():
    """Row 0 is exactly [3, 4, 0, ...]: sumsq == 25.0, norm == 5.0."""
    rng = np.random.default_rng(5)
    diffs = np.zeros((3, 8), F)
    diffs[0, :2] = (3.0, 4.0)
    diffs[1] = rng.standard_normal(8).astype(F) * F(0.1)
    diffs[2] = rng.standard_normal(8).astype(F) * F(100.0)
    return rng.standard_normal(8).astype(F), diffs


def nonfinite_inputs():
    rng = np.random.default_rng(6)
    diffs = (rng.standard_normal((4, 12)) * 3.0).astype(F)
    diffs[1, 5] = np.inf
    diffs[2, 7] = np.nan
    return rng.standard_normal(12).astype(F), diffs


def bits64(x) -> np.ndarray:
    return np.asarray(x, np.float64).view(np.uint64)


def build() -> dict:
    out = {"sumsq_p": np.array(SUMSQ_P, np.int64)}
    for p in SUMSQ_P:
        rows = mixed_rows(p)
        if p <= STORED_P_MAX:
            out[f"rows_{p}"] = rows
        out[f"sumsq_bits_{p}"] = bits64([CO.row_sumsq(r) for r in rows])
    ckpt, diffs = fold_inputs()
    s = CO.scales(diffs, FOLD_C)
    out.update(fold_ckpt=ckpt, fold_diffs=diffs, fold_c=np.float32(FOLD_C),
               fold_sumsq_bits=bits64([CO.row_sumsq(d) for d in diffs]), fold_scales=s,
               fold_out=CO.fold(diffs, s, ckpt))
    ckpt, diffs = boundary_inputs()
    below = np.nextafter(F(5.0), F(0.0))
    out.update(bnd_ckpt=ckpt, bnd_diffs=diffs, bnd_c=np.array([5.0, below], F),
               bnd_sumsq_bits=bits64([CO.row_sumsq(d) for d in diffs]),
               bnd_scales=np.stack([CO.scales(diffs, 5.0), CO.scales(diffs, below)]),
               bnd_out=np.stack([CO.fedavg_clipped(ckpt, diffs, 5.0), CO.fedavg_clipped(ckpt, diffs, below)]))
    ckpt, diffs = nonfinite_inputs()
    out.update(nf_ckpt=ckpt, nf_diffs=diffs, nf_c=np.float32(4.0), nf_scales=CO.scales(diffs, 4.0),
               nf_out=CO.fedavg_clipped(ckpt, diffs, 4.0))
    return out


def main():
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLDEN, **build())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
