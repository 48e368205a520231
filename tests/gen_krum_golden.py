"""Writes tests/golden/krum_cases.npz: inputs, distance matrices (u64 bit patterns), scores (u64) and picked
lists of small Multi-Krum cases, as tests/krum_oracle.py computed them when the definition (include/pgh_api.h,
DESIGN.md section 5) was written.  The tests load the file, so a later edit of the oracle cannot move the
definition unnoticed.  Run from the repository root:

    python tests/gen_krum_golden.py

Only when the definition itself changes (the header, DESIGN.md, the oracle and this file together)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import krum_oracle as KO  # noqa: E402

F = np.float32
GOLDEN = ROOT / "tests" / "golden" / "krum_cases.npz"

HOSTILE_P = 4097  # one full tile and one param of the next
HOSTILE_F = 4
HOSTILE_GOOD = (0, 1, 3, 5, 6, 8, 10)  # where the seven good rows stand
HOST_CASES = 6     # random matrices for the host step alone: (n, f, m) below
HOST_SHAPES = ((5, 1, 0), (9, 3, 0), (9, 2, 1), (12, 4, 8), (16, 0, 0), (33, 10, 23))


def hostile_inputs():
    """12 rows: 7 at centre + 0.05 N(0,1); a row of 1e30; -10 x centre; a row of 3e38 and one of -3e38; a good
    row holding a NaN.  Returns (ckpt, diffs, centre)."""
    rng = np.random.default_rng(4097)
    centre = rng.standard_normal(HOSTILE_P).astype(F)
    good = [(centre + rng.standard_normal(HOSTILE_P) * 0.05).astype(F) for _ in range(8)]
    nan = good[7].copy()
    nan[4096] = np.nan  # in the ragged tile
    rows = {2: np.full(HOSTILE_P, 1e30, F), 4: (centre * F(-10)).astype(F), 7: np.full(HOSTILE_P, 3e38, F),
            9: np.full(HOSTILE_P, -3e38, F), 11: nan}
    for k, g in zip(HOSTILE_GOOD, good):
        rows[k] = g
    diffs = np.stack([rows[k] for k in range(12)])
    return rng.standard_normal(HOSTILE_P).astype(F), diffs, centre


def host_matrix(k: int) -> np.ndarray:
    """A symmetric matrix with exact ties (values drawn from a few), +inf entries and a +0.0 diagonal."""
    n = HOST_SHAPES[k][0]
    rng = np.random.default_rng(100 + k)
    pool = np.concatenate([rng.random(4) * 10, [0.0, 1.0, 1.0, np.inf, 1e300]])
    D = np.zeros((n, n), np.float64)
    for a in range(n):
        for b in range(a + 1, n):
            D[a, b] = D[b, a] = pool[rng.integers(pool.size)] if rng.random() < 0.6 else rng.random() * 5
    if k == 4:  # every row alike: every score ties, the earliest rows win
        D[:] = 2.5
        np.fill_diagonal(D, 0.0)
    return D


def bits64(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def cases() -> dict:
    out = {}
    ckpt, diffs, _ = hostile_inputs()
    g = KO.krum(diffs, HOSTILE_F)
    assert g["picked"] == list(HOSTILE_GOOD) and g["excluded"] == 1 and len(g["included"]) == 2 * HOSTILE_F + 3
    assert np.isinf(g["D"]).any()
    inc = g["included"]
    assert g["scores"][inc.index(7)] == g["scores"][inc.index(9)]  # the two 3e38 rows tie
    out["hostile_ckpt"], out["hostile_diffs"] = ckpt, diffs
    out["hostile_included"] = np.array(inc, np.int32)
    out["hostile_D_bits"] = bits64(g["D"])
    out["hostile_score_bits"] = bits64(g["scores"])
    out["hostile_picked"] = np.array(g["picked"], np.int32)
    out["hostile_stats_bits"] = bits64([g["max_picked_score"], g["min_dropped_score"]])
    for m in (1, 3):
        out[f"hostile_picked_m{m}"] = np.array(KO.krum(diffs, HOSTILE_F, m)["picked"], np.int32)
    for k, (n, f, m) in enumerate(HOST_SHAPES):
        D = host_matrix(k)
        pos, sc = KO.select(D, f, m)
        out[f"host_D_bits_{k}"] = bits64(D)
        out[f"host_picked_{k}"] = np.array(pos, np.int32)
        out[f"host_score_bits_{k}"] = bits64(sc)
    return out


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **cases())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")
