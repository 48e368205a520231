"""Writes tests/golden/geomed_cases.npz: inputs, weights (u32 bit patterns), objectives (u64) and outputs of
small geometric-median cases, as tests/geomed_oracle.py computed them when the definition (include/pgh_api.h,
DESIGN.md section 5) was written.  The tests load the file, so a later edit of the oracle cannot move the
definition unnoticed.  Run from the repository root:

    python tests/gen_geomed_golden.py

Only when the definition itself changes (the header, DESIGN.md, the oracle and this file together)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import geomed_oracle as GO  # noqa: E402

F = np.float32
GOLDEN = ROOT / "tests" / "golden" / "geomed_cases.npz"

FOLD_P = 4099  # one full tile and a ragged one
FOLD_M = (0.01, 0.02, 5, 0.01, 40)
FOLD_ITERS = (1, 2, 3, 16)
HOSTILE_P = 301


def fold_inputs():
    rng = np.random.default_rng(4099)
    ckpt = rng.standard_normal(FOLD_P).astype(F)
    diffs = np.stack([(rng.standard_normal(FOLD_P) * m).astype(F) for m in FOLD_M])
    return ckpt, diffs


def hostile_inputs():
    """7 rows near a common mean, then an all-1e30 row, a row holding a NaN, a row holding +inf."""
    rng = np.random.default_rng(301)
    mean = rng.standard_normal(HOSTILE_P).astype(F)
    good = np.stack([(mean + rng.standard_normal(HOSTILE_P) * 0.05).astype(F) for _ in range(7)])
    big = np.full(HOSTILE_P, 1e30, F)
    nan = good[1].copy()
    nan[17] = np.nan
    inf = good[2].copy()
    inf[200] = np.inf
    diffs = np.concatenate([good[:3], big[None], good[3:5], nan[None], good[5:], inf[None]])
    return rng.standard_normal(HOSTILE_P).astype(F), diffs, mean


def step_inputs():
    """Squared distances for the host step alone: mixed magnitudes, a zero (the smoothing takes over), an
    infinity and a NaN (weight 0), a value whose square root is below the smoothing."""
    return np.array([4.0, 1e-20, 0.0, 2.25e10, np.inf, 9.0, np.nan, 1e-3, 7.5], np.float64), F(1e-6)


def bits64(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def bits32(x) -> np.ndarray:
    return np.ascontiguousarray(x, F).view(np.uint32)


def cases() -> dict:
    out = {}
    ckpt, diffs = fold_inputs()
    out["fold_ckpt"], out["fold_diffs"] = ckpt, diffs
    for it in FOLD_ITERS:
        g = GO.geomed(diffs, it, GO.DEFAULT_NU)
        out[f"fold_w_bits_{it}"] = bits32(g["weights"])
        out[f"fold_obj_bits_{it}"] = bits64(g["objectives"])
        out[f"fold_out_bits_{it}"] = bits32(GO.fedavg_geomed(ckpt, diffs, it, GO.DEFAULT_NU))
    point = diffs[1]
    out["distsq_bits"] = bits64([GO.row_distsq(d, point) for d in diffs])
    hck, hd, _ = hostile_inputs()
    out["hostile_ckpt"], out["hostile_diffs"] = hck, hd
    out["hostile_out_bits"] = bits32(GO.fedavg_geomed(hck, hd, 3, GO.DEFAULT_NU))
    D, nu = step_inputs()
    w, W, obj, B = GO.step(D, nu)
    out["step_D"], out["step_nu"] = D, np.array([nu], F)
    out["step_w_bits"], out["step_W_bits"] = bits32(w), bits32([W])
    out["step_obj_bits"], out["step_B_bits"] = bits64([obj]), bits64([B])
    return out


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **cases())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")
