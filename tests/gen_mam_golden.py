"""Writes tests/golden/mam_cases.npz: inputs and expected outputs of the small cases of the mean around the
median, as tests/mam_oracle.py computed them when the definition (include/pgh_api.h) was
written.  The CPU test and the GPU test both load the file, so a later edit of the oracle cannot move the
definition unnoticed.  Run from the repository root:

    python tests/gen_mam_golden.py

Only when the definition itself changes (pgh_api.h, DESIGN.md, the oracle and this file together).

``columns(n)`` is the one seeded input builder of the K15 tests: the first n of 1,024 fixed rows over P = 257
columns.  Its columns are built so that a kernel that is wrong in one step of the definition gives other bits in
some column at every N and drop the GPU tests use (tests/test_mean_around_median_logic.py proves that without a
GPU, with a table of wrong variants).  The columns, by ``COLS``:

* ``nonfinite``: 4 specials (+NaN 0x7fc00000, -NaN 0xffc00000, +inf, -inf) x 4 phases j.  Row 0 and the rows
  k = j (mod 4) hold finite values, every other row the special, so the special is the column's median from
  N = 4 on, and with j = (N - 1) mod 4 finite rows stand before and after the special ones: every distance is
  NaN (or inf for the finite rows around an infinite median) and step 3 alone decides which rows are kept.
* ``inf_middles``: -inf and +inf in turn; an even N has a -inf and a +inf middle, m = 0.5 a + 0.5 b is NaN.  (No
  finite rows here: every finite value sorts between the infinities, so one of them would be a middle.)
* ``order``: 2^62 at position 62 and -2^62 at position 64 (two blocks of 64) among small odd integers.  Column
  0 of the pair has one farther value, 2^100 at position 1, which drop = 1 removes; column 1 has +-2^100 at every
  odd position, which drop = N // 2 removes.  Both large values are kept; the block sum -2^62 + (odd integers)
  loses the integers of block 1, which a plain left fold or a fold by blocks of 128 adds after 2^62 - 2^62 = 0.
* ``huge``: values in [3e38, 3.3e38]: two of them overflow an f32 sum and an f32 quotient's dividend.
* ``subnormal``: integer multiples of 2^-149, 60 .. 140 in six columns and 2^20 .. 2^22 in six (apart enough
  to show in the mean of 1,023 of them): every distance is subnormal; flushed, all would tie.
* ``middles``: 10, -10, then -1 and 1.5 in turn: the middles of an even N are -1 and 1.5, m = 0.25 makes -10
  the farthest value, the lower middle alone would make it 10.
* ``grid``: integers in [-3, 3]: ties at the threshold distance, in more than one block of 64.
* ``normal``: standard normals: even-N middles that differ, sums that an f32 accumulator rounds differently.

The checkpoint is 0 under the built columns (out = -mean keeps every bit of the mean) and normal elsewhere."""
from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import mam_oracle as MM  # noqa: E402

F, U32 = np.float32, np.uint32
GOLDEN = ROOT / "tests" / "golden" / "mam_cases.npz"

CASES = ((4, 1), (9, 3), (17, 8), (33, 16), (70, 9), (129, 64))  # (N, c)
P, ROWS = 257, 1024
# the row counts of the GPU tier test: K15's tiers end at 8, 16, 32 and 64 rows (one lane holds the column) and at
# 128, 256, 512 and 1,024 (2, 4, 8 and 16 waves share it): each tier's last row count and the ones beside it
# (so every tier runs at its largest and its smallest N), and the smallest closes, 2 and 3 rows
TIER_N = (2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
OTHER_N = (9, 37, 130, 513)  # the other GPU tests that take ``columns``: these row counts, drop = N // 2


def drops_used(n: int):
    """Every drop count a test runs ``columns(n)`` with: 1, N // 2 and N - 1 by the tiers, N // 2 by the other GPU
    tests, c by the golden cases."""
    return sorted({1, n // 2, n - 1} | {c for m, c in CASES if m == n})


N_USED = tuple(sorted(set(TIER_N) | set(OTHER_N) | {m for m, _ in CASES}))
PNAN, NNAN, PINF, NINF = 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000
SPECIALS = (PNAN, NNAN, PINF, NINF)
COLS = {"nonfinite": range(0, 16), "inf_middles": range(16, 17), "order": range(17, 19), "huge": range(19, 23),
        "subnormal": range(23, 35), "middles": range(35, 36), "grid": range(36, 161), "normal": range(161, 257)}
BIG_AT = (62, 64)  # the positions of 2^62 and -2^62 in the order columns


@functools.lru_cache(maxsize=1)
def _table():
    rng = np.random.default_rng(15)
    k = np.arange(ROWS)
    d = np.zeros((ROWS, P), F)
    u = d.view(U32)
    ckpt = rng.standard_normal(P).astype(F)
    ckpt[:COLS["grid"][0]] = F(0.0)
    d[:, COLS["grid"]] = rng.integers(-3, 4, (ROWS, len(COLS["grid"])))
    d[:, COLS["normal"]] = rng.standard_normal((ROWS, len(COLS["normal"])))
    for s, bits in enumerate(SPECIALS):
        for j in range(4):
            col = COLS["nonfinite"][4 * s + j]
            d[:, col] = rng.standard_normal(ROWS)
            u[(k != 0) & (k % 4 != j), col] = bits
    u[:, COLS["inf_middles"][0]] = np.where(k % 2 == 0, NINF, PINF)
    one, half = COLS["order"]
    d[:, one] = d[:, half] = 2 * rng.integers(0, 8, ROWS) + 1
    d[1, one] = F(2.0 ** 100)
    d[k % 4 == 1, half], d[k % 4 == 3, half] = F(2.0 ** 100), F(-2.0 ** 100)
    d[BIG_AT[0], [one, half]], d[BIG_AT[1], [one, half]] = F(2.0 ** 62), F(-2.0 ** 62)
    d[:, COLS["huge"]] = F(3e38) * (1 + 0.1 * rng.random((ROWS, len(COLS["huge"])))).astype(F)
    u[:, COLS["subnormal"][:6]] = rng.integers(60, 141, (ROWS, 6))
    u[:, COLS["subnormal"][6:]] = rng.integers(1 << 20, 1 << 22, (ROWS, 6))
    d[:, COLS["middles"][0]] = np.where(k % 2 == 0, F(-1.0), F(1.5))
    d[:2, COLS["middles"][0]] = F(10.0), F(-10.0)
    d.setflags(write=False)
    ckpt.setflags(write=False)
    return d, ckpt


def columns(n: int):
    """``(rows [n, P], ckpt [P])``: the first n rows of the table (read-only views)."""
    d, ckpt = _table()
    return d[:n], ckpt


def nan_payload_case(n: int = 9):
    """``(rows [n, 70], ckpt, c)``, n >= 8: NaNs of three payloads in every column.  Sorted by key the rows are four
    finite values, 0x7fc00000 n - 6 times, 0x7fc00001 and 0x7fe00000, so m = +NaN 0x7fc00000.  In fold order a finite
    row, 0x7fe00000, 0x7fc00001, two finite rows, 0x7fc00000 n - 6 times, a finite row; c = n - 3 keeps three.
    n = 8 (the tier of up to 8 rows) has one finite row in the middle, not two, 0x7fc00000 three times (both
    middles), and c = 6 keeps two."""
    rng = np.random.default_rng(9)
    ckpt, d = rng.standard_normal(70).astype(F), rng.standard_normal((n, 70)).astype(F)
    keep = 3 if n >= 9 else 2
    d.view(U32)[2 + keep:n - 1] = PNAN
    d.view(U32)[1], d.view(U32)[2] = 0x7FE00000, 0x7FC00001
    return d, ckpt, n - keep


def nan_payload_out(carries: str, n: int = 9) -> np.ndarray:
    """What the case above gives if the difference of two NaNs carries x_k's payload (``"x"``: the finite rows tie
    with the 0x7fc00000 rows at the smallest distance and win by position: rows 0, 3 and 4 (n = 8: 0 and 3), a
    finite mean) or m's (``"m"``: every distance ties, rows 0, 1 and 2 (0 and 1) are kept, the mean is NaN).
    x - m of a finite x is m's NaN."""
    d, ckpt, c = nan_payload_case(n)
    e = np.where(np.isnan(d) & (carries == "x"), d.view(U32), U32(PNAN)) & U32(0x7FFFFFFF)
    v = np.take_along_axis(d, np.sort(np.argsort(e, axis=0, kind="stable")[:n - c], axis=0), axis=0).astype(np.float64)
    with np.errstate(all="ignore"):
        s = v[0]
        for x in v[1:]:
            s = s + x
        return (ckpt - (s / np.float64(n - c)).astype(F)).astype(F)


def build() -> dict:
    out = {"cases": np.array(CASES, np.int64)}
    d, ckpt, c = nan_payload_case()
    out["ckpt_nan"], out["diffs_nan"], out["out_nan"] = ckpt, d, MM.fedavg(ckpt, d, c)
    for n, c in CASES:
        d, ckpt = columns(n)
        out[f"ckpt_{n}"] = ckpt
        out[f"diffs_{n}"] = d
        out[f"out_{n}"] = MM.fedavg(ckpt, d, c)
        out[f"kept_{n}"] = MM.mean_around_median(d, c)[2].astype(np.int32)
    return out


def main():
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLDEN, **build())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
