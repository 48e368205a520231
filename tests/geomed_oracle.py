"""Test infrastructure: the geometric-median close (PGH_GEOMETRIC_MEDIAN, kernel K12) restated in numpy,
operation by operation, from the definition in include/pgh_api.h ("geometric-median FedAvg") and DESIGN.md
section 5.  The order of the sums is K7's: ``clip_oracle.tile_partials`` / ``row_sumsq``.  Never a product
path: the product's Engine has no CPU fallback."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402

F32 = np.float32
F64 = np.float64
MAX_ITERS = 16
DEFAULT_ITERS, DEFAULT_NU = 3, 1e-6
same_bits = CO.same_bits


def row_distsq(d, v) -> np.float64:
    """K12: K7's sum over ``x_i = d[i] - v[i]``, one f32 subtraction per param."""
    with np.errstate(all="ignore"):
        x = (np.asarray(d, F32).reshape(-1) - np.asarray(v, F32).reshape(-1)).astype(F32)
    return CO.row_sumsq(x)


def step(D, nu):
    """The host step: squared distances (f64, fold order) -> ``(w [f32], W f32, objective f64, B f64)``; B == 0
    (every D non-finite) gives ``w = W = None``."""
    nu = F64(F32(nu))
    D = np.asarray(D, F64).reshape(-1)
    beta = np.zeros(D.size, F64)
    B = obj = None
    with np.errstate(all="ignore"):
        for k, Dk in enumerate(D):
            dist = np.sqrt(Dk)
            beta[k] = F64(1.0) / max(nu, dist) if np.isfinite(Dk) else F64(0.0)
            B = beta[k] if k == 0 else F64(B + beta[k])
            obj = dist if k == 0 else F64(obj + dist)
        if not B != 0.0:
            return None, None, obj, B
        w = np.array([F32(b / B) for b in beta], F32)
        W = w[0]
        for x in w[1:]:
            W = F32(W + x)
    return w, W, obj, B


def weighted_mean(rows, w, W) -> np.ndarray:
    """``acc = d_0 * w_0; acc = acc + d_c * w_c`` (product rounded to f32, then added); ``acc / W``."""
    with np.errstate(all="ignore"):
        acc = (np.asarray(rows[0], F32).reshape(-1) * F32(w[0])).astype(F32)
        for d, wc in zip(rows[1:], w[1:]):
            acc = (acc + (np.asarray(d, F32).reshape(-1) * F32(wc)).astype(F32)).astype(F32)
        return (acc / F32(W)).astype(F32)


class NoFiniteRow(ValueError):
    """No row included, or no finite distance in an iteration: the engine's PGH_E_STATE."""


def geomed(diffs, iters=DEFAULT_ITERS, nu=DEFAULT_NU) -> dict:
    """Rows in fold order -> ``v`` (= v^(iters), f32 [P]), ``included`` (row indices), ``weights`` / ``W`` of
    the last iteration, ``objectives`` (one per iteration), ``max_weight``, ``excluded`` (a count)."""
    assert 1 <= iters <= MAX_ITERS
    rows = [np.asarray(d, F32).reshape(-1) for d in diffs]
    s = [CO.row_sumsq(d) for d in rows]
    inc = [k for k, x in enumerate(s) if np.isfinite(x)]
    if not inc:
        raise NoFiniteRow("no row is finite")
    kept = [rows[k] for k in inc]
    D = [s[k] for k in inc]
    objectives = []
    for t in range(iters):
        w, W, obj, _ = step(D, nu)
        if w is None:
            raise NoFiniteRow(f"no finite distance in iteration {t}")
        objectives.append(obj)
        v = weighted_mean(kept, w, W)
        if t < iters - 1:
            D = [row_distsq(d, v) for d in kept]
    return {"v": v, "included": inc, "weights": w, "W": W, "objectives": objectives, "objective": objectives[-1],
            "max_weight": F32(max(w)), "excluded": len(rows) - len(inc)}


def fedavg_geomed(ckpt, diffs, iters=DEFAULT_ITERS, nu=DEFAULT_NU) -> np.ndarray:
    """Flat arrays: ``ckpt`` [P], ``diffs`` N x [P]; the new checkpoint ``ckpt - v`` [P]."""
    with np.errstate(all="ignore"):
        return (np.asarray(ckpt, F32).reshape(-1) - geomed(diffs, iters, nu)["v"]).astype(F32)


def objective_at(diffs, point) -> np.float64:
    """The plain sum of distances of the finite rows to ``point`` (f64 numpy; properties, not bits)."""
    p = np.asarray(point, F64).reshape(-1)
    return F64(sum(np.sqrt(np.sum((np.asarray(d, F64).reshape(-1) - p) ** 2)) for d in diffs))
