"""Writes tests/golden/clip_cases.npz: inputs, sums of squares (as u64 bit patterns), scales and
outputs of the small clipped-FedAvg cases, as tests/clip_oracle.py computed them when the definition
 was written.  Both test files load the file, so a later edit of the oracle
cannot move the definition unnoticed.  Run from the repository root:

    python tests/gen_clip_golden.py

Only when the definition itself changes (the oracle and this file together)."""
from __future__ import annotations

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
