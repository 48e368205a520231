"""Writes tests/golden/trust_cases.npz: inputs, sums and dots (u64 bit patterns), weights (u32) and outputs of
small trust-bootstrapped cases, as tests/trust_oracle.py computed them when the definition (include/pgh_api.h,
DESIGN.md section 5) was written.  The tests load the file, so a later edit of the oracle cannot move the
definition unnoticed.  Run from the repository root:

    python tests/gen_trust_golden.py

Only when the definition itself changes (the header, DESIGN.md, the oracle and this file together)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import clip_oracle as CO  # noqa: E402
import trust_oracle as TO  # noqa: E402

F = np.float32
GOLDEN = ROOT / "tests" / "golden" / "trust_cases.npz"

FOLD_P = 4099  # one full tile and a ragged one
FOLD_M = (0.01, 0.02, 5, 0.01, 40)
HOSTILE_P = 301
HOSTILE_N, HONEST = 10, (1, 4, 8)  # 7 of 10 rows point away from the root


def fold_inputs():
    """Five rows of mixed magnitude around a common direction, the root along it."""
    rng = np.random.default_rng(14099)
    ckpt = rng.standard_normal(FOLD_P).astype(F)
    root = (rng.standard_normal(FOLD_P) * 0.1).astype(F)
    diffs = np.stack([((root + rng.standard_normal(FOLD_P) * 0.08) * m).astype(F) for m in FOLD_M])
    diffs[3] = -diffs[3]  # one row pointing away: trust 0, it stays in the fold
    return ckpt, diffs, root


def hostile_inputs():
    """A hostile majority: the rows of HONEST near the root, every other row pointing away from it with a
    magnitude of up to 1e30 (finite sums of squares: the rows stay included)."""
    rng = np.random.default_rng(14301)
    root = (rng.standard_normal(HOSTILE_P) * 0.05).astype(F)
    mags = 10.0 ** rng.uniform(0, 30, HOSTILE_N)
    diffs = np.stack([(root * 0.7 + rng.standard_normal(HOSTILE_P) * 0.01).astype(F) if k in HONEST
                      else ((-root + rng.standard_normal(HOSTILE_P) * 0.005) * min(mags[k], 1e30)).astype(F)
                      for k in range(HOSTILE_N)])
    return rng.standard_normal(HOSTILE_P).astype(F), diffs, root


def weights_inputs():
    """The host step alone: s0 and per row (sumsq, dot) -- an ordinary row, a row pointing away, an all-zero row,
    a NaN and an infinite sum (excluded, their dots NaN), a row of subnormal norm along the root (its rescale is
    clamped), an orthogonal row, a long row."""
    s0 = np.float64(2.5)
    sumsq = np.array([1.0, 4.0, 0.0, np.nan, np.inf, 1e-90, 9.0, 1e20], np.float64)
    dot = np.array([0.75, -3.0, 0.0, np.nan, np.nan, 1.2e-45, 0.0, 1e10], np.float64)
    return s0, sumsq, dot


def bits64(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def bits32(x) -> np.ndarray:
    return np.ascontiguousarray(x, F).view(np.uint32)


def cases() -> dict:
    out = {}
    ckpt, diffs, root = fold_inputs()
    t = TO.trust(diffs, root)
    out["fold_ckpt"], out["fold_diffs"], out["fold_root"] = ckpt, diffs, root
    out["fold_s0_bits"] = bits64([t["s0"]])
    out["fold_sumsq_bits"], out["fold_dot_bits"] = bits64(t["sumsq"]), bits64(t["dot"])
    out["fold_w_bits"], out["fold_T_bits"] = bits32(t["weights"]), bits64([t["T"]])
    out["fold_out_bits"] = bits32(TO.fedavg_trust(ckpt, diffs, root))
    hck, hd, hroot = hostile_inputs()
    out["hostile_ckpt"], out["hostile_diffs"], out["hostile_root"] = hck, hd, hroot
    out["hostile_out_bits"] = bits32(TO.fedavg_trust(hck, hd, hroot))
    s0, ss, dt = weights_inputs()
    w = TO.trust_weights(s0, ss, dt)
    out["w_s0"], out["w_sumsq"], out["w_dot"] = np.array([s0]), ss, dt
    out["w_included"] = np.array(w["included"], np.int32)
    out["w_bits"], out["w_T_bits"] = bits32(w["weights"]), bits64([w["T"]])
    return out


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **cases())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")
