"""Numpy restatement of the mean around the median (PGH_MEAN_AROUND_MEDIAN; include/pgh_api.h, DESIGN.md
section 5).  Test infrastructure only: the product has no CPU path."""
from __future__ import annotations

import numpy as np

from median_oracle import median_of_rows
from trim_oracle import key, same_bits  # noqa: F401  (key orders the median; same_bits: re-exported)

F32, F64, U32 = np.float32, np.float64, np.uint32


def mean_around_median(diffs, drop: int):
    """``diffs`` N x [P] in fold order: ``(mean [P], rows at the threshold distance E [P], how many of those are
    kept [P])``: the N - drop smallest by (e, k) -- a stable argsort on e -- added in f64, a block of 64 fold
    positions at a time from +0.0, the block sums left to right."""
    d = np.stack([np.asarray(r, F32).reshape(-1) for r in diffs])
    n, beta = d.shape[0], d.shape[0] - int(drop)
    with np.errstate(all="ignore"):
        e = (d - median_of_rows(d)[None, :]).astype(F32).view(U32) & U32(0x7FFFFFFF)
    order = np.argsort(e, axis=0, kind="stable")
    kept = np.zeros(d.shape, bool)
    np.put_along_axis(kept, order[:beta], True, axis=0)
    at_e = e == np.take_along_axis(e, order[beta - 1:beta], axis=0)
    S = None
    with np.errstate(all="ignore"):
        for g in range(0, n, 64):
            s = np.zeros(d.shape[1], F64)
            for k in range(g, min(n, g + 64)):
                s = np.where(kept[k], s + d[k].astype(F64), s)
            S = s if S is None else S + s
        return (S / F64(beta)).astype(F32), at_e.sum(0), (at_e & kept).sum(0), at_e


def _bits(x) -> int:
    return int(np.float32(x).view(U32))


def _key(b: int) -> int:
    """The median's signed key of a bit pattern, as a Python int."""
    b ^= 0x7FFFFFFF if b >> 31 else 0
    return b - (1 << 32) if b >> 31 else b


def column_scalar(col, drop: int):
    """One column, one value at a time, a second restatement that shares no array expression with the one above:
    ``(mean, how many rows at the threshold distance E are kept)``.  f32 steps are numpy f32 scalars, the sum
    is Python floats (f64)."""
    x = [np.float32(v) for v in col]
    n, beta = len(x), len(x) - int(drop)
    with np.errstate(all="ignore"):
        s = sorted(x, key=lambda v: _key(_bits(v)))
        m = s[(n - 1) // 2] if n & 1 else np.float32(0.5) * s[n // 2 - 1] + np.float32(0.5) * s[n // 2]
        ek = sorted((_bits(x[k] - m) & 0x7FFFFFFF, k) for k in range(n))[:beta]
        kept = {k for _, k in ek}
        total = None
        for g in range(0, n, 64):
            block = 0.0
            for k in range(g, min(n, g + 64)):
                if k in kept:
                    block += float(x[k])
            total = block if total is None else total + block
        return np.float32(total / float(beta)), sum(1 for e, _ in ek if e == ek[-1][0])


def mean_around_median_scalar(diffs, drop: int):
    """``column_scalar`` over every column of ``diffs`` N x [P]: ``(mean [P], kept at E [P])``."""
    d = np.stack([np.asarray(r, F32).reshape(-1) for r in diffs])
    res = [column_scalar(d[:, c], drop) for c in range(d.shape[1])]
    return np.array([r[0] for r in res], F32), np.array([r[1] for r in res], np.int64)


def fedavg(ckpt, diffs, drop: int) -> np.ndarray:
    """Flat arrays: the new checkpoint ``ckpt - mean``, one f32 subtraction."""
    with np.errstate(all="ignore"):
        return (np.asarray(ckpt, F32).reshape(-1) - mean_around_median(diffs, drop)[0]).astype(F32)
