"""Writes tests/golden/median_cases.npz: inputs and expected outputs of the small median cases, as
tests/median_oracle.py computed them when the definition was written.  Both
test files load the file, so a later edit of the oracle cannot move the definition unnoticed.  Run
from the repository root:

    python tests/gen_median_golden.py

Only when the definition itself changes (the oracle and this file together)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import median_oracle as MO  # noqa: E402

F = np.float32
GOLDEN = ROOT / "tests" / "golden" / "median_cases.npz"

CASES = (1, 2, 3, 4, 9, 16)  # N
CASE_P = 40
SUB = F(1e-45)  # the smallest subnormal (bits 1): 0.5 x it rounds to even, i.e. to 0


def f32(bits: int) -> np.float32:
    return np.array([bits], np.uint32).view(F)[0]


def plant(d: np.ndarray, col: int, mids, low=F(-7.0), high=F(7.0)):
    """Column ``col``: the middle one (N odd) or two (N even) values of the sort are ``mids``, the
    other rows split evenly below and above, scattered over the rows."""
    n = d.shape[0]
    k = 1 if n & 1 else 2
    side = (n - k) // 2
    vals = [low] * side + list(mids[:k]) + [high] * side
    perm = np.random.default_rng(1000 * n + col).permutation(n)
    d[perm, col] = np.array(vals, F)


def case_inputs(n: int):
    rng = np.random.default_rng(4200 + n)
    d = rng.standard_normal((n, CASE_P)).astype(F)
    ckpt = rng.standard_normal(CASE_P).astype(F)
    plant(d, 0, [F(-0.0), F(0.0)])                 # +-0 middles: -0, +0 -> +0 (N odd: -0)
    plant(d, 1, [F(0.0), F(0.0)])
    plant(d, 2, [SUB, f32(2)])                     # subnormal middles: 0.5 x an odd subnormal rounds
    plant(d, 3, [f32(3), f32(3)])
    plant(d, 4, [-SUB, f32(0x80000003)])
    d[:, 5] = F(0.25)                              # an all-equal column
    d[:, 6] = np.where(np.arange(n) % 2 == 0, F(1.5), F(-2.0))  # ties across the middle
    d[:, 7] = np.where(np.arange(n) < (n + 1) // 2, F(1.5), F(-2.0))
    plant(d, 8, [F(3e38), F(3e38)], high=F(3.2e38))  # both middles 3e38: a finite result
    plant(d, 9, [F(-3e38), F(-3e38)], low=F(-3.2e38))
    plant(d, 10, [-np.inf, np.inf], low=-np.inf, high=np.inf)  # middles -inf and +inf: NaN (N even)
    plant(d, 11, [np.inf, np.inf], high=np.inf)
    h = (n + 1) // 2 - 1                           # ceil(N / 2) - 1 NaNs of each sign: a finite result
    for col, vals in ((12, [np.nan] * h), (13, [-np.nan] * h), (14, [np.nan] * (h // 2) + [-np.nan] * (h - h // 2))):
        rows = np.random.default_rng(77 * n + col).permutation(n)[:h]
        d[rows, col] = np.array(vals, F) if h else d[rows, col]
    maj = n // 2 + 1                               # a NaN majority of one sign: a NaN result
    d[np.random.default_rng(5 * n).permutation(n)[:maj], 15] = np.nan
    d[np.random.default_rng(6 * n).permutation(n)[:maj], 16] = -np.nan
    d[0, 17], d[n - 1, 18] = F(1e30), F(-1e30)     # one huge value
    return ckpt, d


def build() -> dict:
    out = {"cases": np.array(CASES, np.int64)}
    for n in CASES:
        ckpt, d = case_inputs(n)
        out[f"ckpt_{n}"] = ckpt
        out[f"diffs_{n}"] = d
        out[f"median_{n}"] = MO.median_of_rows(d)
        out[f"out_{n}"] = MO.fedavg_median(ckpt, d)
    return out


def main():
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLDEN, **build())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
