"""Test infrastructure: the Multi-Krum selection (pgh_krum_select, kernel K13) restated in numpy and python
floats, step by step, from the definition in include/pgh_api.h ("Multi-Krum selection") and DESIGN.md section 5.
The distances are ``geomed_oracle.row_distsq`` (K7's order over one f32 subtraction); the scores are python-float
left folds.  Never a product path: the product's Engine has no CPU fallback."""
from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import geomed_oracle as GO  # noqa: E402

F32 = np.float32
F64 = np.float64
MAX_ROWS = 1024


class BadDistance(ValueError):
    """A NaN or negative off-diagonal distance: the engine's PGH_E_ARG."""


class TooFewRows(ValueError):
    """n' < 2f + 3 or m > n' - f: the engine's PGH_E_STATE."""


def included(diffs):
    """Step 1: the indices of the rows whose K7 sum of squares is finite, in order."""
    return [k for k, d in enumerate(diffs) if np.isfinite(CO.row_sumsq(np.asarray(d, F32).reshape(-1)))]


def pairdist(rows) -> np.ndarray:
    """Step 2: D[a][b] = K12's sum of row a against the point row b; the diagonal is +0.0."""
    n = len(rows)
    D = np.zeros((n, n), F64)
    for a in range(n):
        for b in range(a + 1, n):
            D[a, b] = D[b, a] = GO.row_distsq(rows[a], rows[b])
    return D


def scores(D, f: int):
    """Step 3: per row the left fold, in ascending order, of the n - f - 2 smallest distances to the others."""
    D = np.asarray(D, F64)
    n = D.shape[0]
    for a in range(n):
        for b in range(n):
            if a != b and not float(D[a, b]) >= 0.0:
                raise BadDistance(f"D[{a}][{b}] = {D[a, b]}")
    if n < 2 * f + 3:
        raise TooFewRows(f"{n} rows, f = {f}")
    k = n - f - 2
    out = []
    for a in range(n):
        vals = sorted(float(D[a, b]) for b in range(n) if b != a)[:k]
        s = vals[0]
        for v in vals[1:]:
            s = s + v
        out.append(s)
    return out


def select(D, f: int, m: int = 0):
    """Steps 3 and 4: ``(picked positions in list order, scores)``."""
    sc = scores(D, f)
    n = len(sc)
    keep = n - f if m == 0 else m
    if keep > n - f:
        raise TooFewRows(f"m = {m} > n - f = {n - f}")
    order = sorted(range(n), key=lambda a: (sc[a], a))
    return sorted(order[:keep]), sc


def krum(diffs, f: int, m: int = 0) -> dict:
    """Steps 1 to 4 over rows in list order: ``picked`` (row indices, list order), ``included``, ``excluded`` (a
    count), ``D`` (over the included rows), ``scores`` (of the included rows)."""
    rows = [np.asarray(d, F32).reshape(-1) for d in diffs]
    inc = included(rows)
    if len(inc) < 2 * f + 3 or m > len(inc) - f:
        raise TooFewRows(f"{len(inc)} finite rows, f = {f}, m = {m}")
    D = pairdist([rows[k] for k in inc])
    pos, sc = select(D, f, m)
    dropped = [sc[k] for k in range(len(inc)) if k not in pos]
    return {"picked": [inc[k] for k in pos], "included": inc, "excluded": len(rows) - len(inc), "D": D, "scores": sc,
            "max_picked_score": max(sc[k] for k in pos), "min_dropped_score": min(dropped) if dropped else math.inf}
