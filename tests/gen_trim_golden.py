"""Writes tests/golden/trim_cases.npz: inputs and outputs (with the final lo / hi keys) of the small
trimmed-mean cases, as tests/trim_oracle.py computed them when the definition
was written.  Both test files load the file, so a later edit of the oracle cannot move the definition
unnoticed.  Run from the repository root:

    python tests/gen_trim_golden.py

Only when the definition itself changes (the oracle and this file together)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import trim_oracle as TO  # noqa: E402

F = np.float32
GOLDEN = ROOT / "tests" / "golden" / "trim_cases.npz"

CASES = ((3, 1), (5, 2), (9, 1), (17, 8), (40, 4))  # (N, b)
CASE_P = 257
SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e38, -1e38, 1e-45, -1e-45, 1e-39], F)


def special_rows(n: int, p: int, seed: int, every: int = 7, rows: int = 3) -> np.ndarray:
    """n rows of p normal floats; every `every`-th param of the first `rows` rows is a special value
    (NaNs of both signs, infinities, zeros of both signs, +-1e38, subnormals)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, p)).astype(F)
    for r in range(min(rows, n)):
        m = d[r, r::every].size
        d[r, r::every] = rng.choice(SPECIALS, size=m)
    return d


def case_inputs(n: int, b: int):
    d = special_rows(n, CASE_P, 9000 + 16 * n + b)
    if n >= 3:
        d[1, 5], d[2, 5] = np.nan, -np.nan  # one column with a NaN of each sign
    d[:, 11] = F(0.25)                      # an all-equal column
    d[:, 12] = np.where(np.arange(n) % 2 == 0, F(1.5), F(-2.0))  # ties across the trim boundary
    ckpt = np.random.default_rng(77 + n).standard_normal(CASE_P).astype(F)
    return ckpt, d


def build() -> dict:
    out = {"cases": np.array(CASES, np.int64)}
    for n, b in CASES:
        ckpt, d = case_inputs(n, b)
        st = TO.TrimState(CASE_P, b)
        for row in d:
            st.step(row)
        out[f"ckpt_{n}_{b}"] = ckpt
        out[f"diffs_{n}_{b}"] = d
        out[f"lo_{n}_{b}"] = st.lo
        out[f"hi_{n}_{b}"] = st.hi
        out[f"out_{n}_{b}"] = st.close(ckpt)
    return out


def main():
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLDEN, **build())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
