"""Test infrastructure: trust-bootstrapped FedAvg (PGH_TRUSTED_MEAN, FLTrust, kernel K14) restated in numpy,
operation by operation, from the definition in include/pgh_api.h ("trust-bootstrapped FedAvg") and DESIGN.md
section 5.  The order of the sums is K7's: ``clip_oracle.tile_partials`` / ``row_sumsq``, here over products.
Never a product path: the product's Engine has no CPU fallback."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402

F32 = np.float32
F64 = np.float64
TILE = CO.TILE
FLT_MAX = F64(np.finfo(F32).max)
same_bits = CO.same_bits


def dot_tile_partials(d, g) -> np.ndarray:
    """K14's tile partials: ``clip_oracle.tile_partials`` over ``(double)d[i] * (double)g[i]`` (exact in f64);
    params at or past P contribute +0.0 whatever either operand would hold there."""
    d = np.ascontiguousarray(d, dtype=F32).reshape(-1)
    g = np.ascontiguousarray(g, dtype=F32).reshape(-1)
    assert d.size == g.size
    n_tiles = max(1, -(-d.size // TILE))
    pr = np.zeros(n_tiles * TILE, dtype=F64)
    with np.errstate(all="ignore"):
        pr[:d.size] = d.astype(F64) * g.astype(F64)
        pr = pr.reshape(n_tiles, 4, 256, 4)           # [t][j][l][e]: param 4096 t + 4 (l + 256 j) + e
        a = np.zeros((n_tiles, 256), dtype=F64)
        for j in range(4):
            for e in range(4):
                a = a + pr[:, j, :, e]
        v = a.reshape(n_tiles, 4, 64).copy()          # [t][wave][lane]
        for h in (32, 16, 8, 4, 2, 1):
            v[:, :, :h] = v[:, :, :h] + v[:, :, h:2 * h]
        w = v[:, :, 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def row_dot(d, g) -> np.float64:
    """K14: K7's sum, in K7's order, over the products of ``d`` and ``g``."""
    parts = dot_tile_partials(d, g)
    acc = F64(parts[0])
    with np.errstate(all="ignore"):
        for p in parts[1:]:
            acc = F64(acc + p)
    return acc


class BadRoot(ValueError):
    """s0 is not finite and > 0: the engine's PGH_E_ARG."""


class NoTrustedRow(ValueError):
    """No row included, or T == 0: the engine's PGH_E_STATE."""


def trust_weights(s0, sumsq, dot) -> dict:
    """Steps 2 and 4: ``included`` (positions), ``weights`` (f32, of the included rows), ``T``, ``ts`` (f64, of
    the included rows) and ``trusted`` (how many have ts > 0)."""
    s0 = F64(s0)
    if not (np.isfinite(s0) and s0 > 0):
        raise BadRoot(f"s0 = {s0}")
    sumsq = np.asarray(sumsq, F64).reshape(-1)
    dot = np.asarray(dot, F64).reshape(-1)
    inc, ts, a = [], [], []
    T = None
    with np.errstate(all="ignore"):
        n0 = np.sqrt(s0)
        for k, sc in enumerate(sumsq):
            if not np.isfinite(sc):
                continue
            if sc > 0:
                nc = np.sqrt(sc)
                cos = F64(dot[k] / F64(n0 * nc))
                t = cos if cos > 0 else F64(0.0)
                ac = F64(t * F64(n0 / nc))
            else:
                t = ac = F64(0.0)
            inc.append(k)
            ts.append(t)
            a.append(ac)
            T = t if T is None else F64(T + t)
        if not inc:
            raise NoTrustedRow("no row is finite")
        if not T != 0.0:
            raise NoTrustedRow("T == 0: no row is trusted")
        w = np.array([F32(min(F64(ac / T), FLT_MAX)) for ac in a], F32)
    return {"included": inc, "weights": w, "T": T, "ts": np.array(ts, F64), "trusted": int(sum(t > 0 for t in ts))}


def weighted_sum(rows, w) -> np.ndarray:
    """``acc = d_0 * w_0; acc = acc + d_c * w_c`` (product rounded to f32, then added), ``acc / 1.0f``."""
    with np.errstate(all="ignore"):
        acc = (np.asarray(rows[0], F32).reshape(-1) * F32(w[0])).astype(F32)
        for d, wc in zip(rows[1:], w[1:]):
            acc = (acc + (np.asarray(d, F32).reshape(-1) * F32(wc)).astype(F32)).astype(F32)
        return (acc / F32(1.0)).astype(F32)


def trust(diffs, root) -> dict:
    """Rows in fold order and the root -> ``acc`` (f32 [P]) and everything ``trust_weights`` returns, plus ``s0``,
    ``sumsq``, ``dot`` (NaN where the row is excluded), ``excluded``, ``max_weight`` and ``root_norm``."""
    rows = [np.asarray(d, F32).reshape(-1) for d in diffs]
    g0 = np.asarray(root, F32).reshape(-1)
    s0 = CO.row_sumsq(g0)
    if not (np.isfinite(s0) and s0 > 0):
        raise BadRoot(f"s0 = {s0}")
    s = np.array([CO.row_sumsq(d) for d in rows], F64)
    p = np.array([row_dot(d, g0) if np.isfinite(sc) else np.nan for d, sc in zip(rows, s)], F64)
    r = trust_weights(s0, s, p)
    r.update(s0=s0, sumsq=s, dot=p, excluded=len(rows) - len(r["included"]), max_weight=F32(max(r["weights"])),
             root_norm=np.sqrt(s0), acc=weighted_sum([rows[k] for k in r["included"]], r["weights"]))
    return r


def fedavg_trust(ckpt, diffs, root) -> np.ndarray:
    """Flat arrays: ``ckpt`` [P], ``diffs`` N x [P], ``root`` [P]; the new checkpoint ``ckpt - acc`` [P]."""
    with np.errstate(all="ignore"):
        return (np.asarray(ckpt, F32).reshape(-1) - trust(diffs, root)["acc"]).astype(F32)
