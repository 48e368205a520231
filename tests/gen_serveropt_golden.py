"""Writes tests/golden/serveropt_cases.npz: per optimizer one step over special and random values
(inputs ckpt, g, m, v; expected out, m', v' from tests/serveropt_oracle.py).  A GPU test replays the
cases with one diff under PGH_MEAN (g = d / 1.0f = d) and the state uploaded.

    python tests/gen_serveropt_golden.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import serveropt_oracle as SO  # noqa: E402

F = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden" / "serveropt_cases.npz"
HP = {"lr": 0.3, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
SPECIAL_BITS = (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0xBF800000,
                0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x33800000, 0x5F000000)


def inputs():
    """Every special value of g against a handful of (ckpt, m, v) settings, then random values."""
    sp = np.array(SPECIAL_BITS, np.uint32).view(F)
    rng = np.random.default_rng(20260)
    settings = [(F(0.25), F(0.0), F(1e-6)), (F(-3.0), F(0.5), F(2.0)), (F(0.0), F(-0.0), F(0.0)),
                (F(1e30), F(1e20), F(3e38)), (F(-0.0), F(1e-40), F(1e-44))]
    ck, g, m, v = [], [], [], []
    for c0, m0, v0 in settings:
        ck += [c0] * sp.size
        g += list(sp)
        m += [m0] * sp.size
        v += [v0] * sp.size
    n = 173  # the whole case stays ragged (len % 4 == 1)
    ck += list((rng.standard_normal(n) * 0.1).astype(F))
    g += list((rng.standard_normal(n) * 1e-2).astype(F))
    m += list((rng.standard_normal(n) * 1e-2).astype(F))
    v += list((rng.random(n) * 1e-4).astype(F))
    return tuple(np.array(a, F) for a in (ck, g, m, v))


def build() -> dict:
    ck, g, m, v = inputs()
    out = {"ckpt": ck, "g": g, "m": m, "v": v, "hp": np.array([HP["lr"], HP["beta1"], HP["beta2"], HP["tau"]], F)}
    for kind in SO.KINDS:
        o, m2, v2 = SO.step(kind, ck, g, m, v, **HP)
        out[f"out_{kind}"], out[f"m_{kind}"], out[f"v_{kind}"] = o, m2, v2
    return out


def main():
    GOLDEN.parent.mkdir(exist_ok=True)
    np.savez_compressed(GOLDEN, **build())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
