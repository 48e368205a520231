"""Numpy restatement of the coordinate-wise trimmed mean (PGH_TRIMMED_MEAN; DESIGN.md section 5,
include/pgh_api.h).  Test infrastructure only: the product has no CPU path.
tests/golden/trim_cases.npz (tests/gen_trim_golden.py) pins what this file computed when the
definition was written, so an edit here cannot silently move the definition.

The definition is a streaming one.  Values are ordered by the int32 key
``bits(x) ^ ((bits(x) >> 31) & 0x7fffffff)`` (arithmetic shift, signed compare), a total order on
bit patterns: ``-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN``; ``unkey`` is the same expression.
Per parameter the state is ``lo[0..b) = INT32_MAX``, ``hi[0..b) = INT32_MIN`` and an f32 ``acc``;
client k = 0, 1, ... in fold order:

1. ``e = key(x_k)``
2. ``for j < b: t = max(lo[j], e); lo[j] = min(lo[j], e); e = t``; stop if ``k < b``
3. ``for j < b: t = min(hi[j], e); hi[j] = max(hi[j], e); e = t``; stop if ``k < 2b``
4. ``v = unkey(e)``; ``acc = v`` if ``k == 2b`` else ``acc + v`` (f32)

and ``out = ckpt - acc / float(N - 2b)``.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
I32 = np.int32
INT_MAX = np.iinfo(np.int32).max
INT_MIN = np.iinfo(np.int32).min


def key(x) -> np.ndarray:
    b = np.ascontiguousarray(x, dtype=F32).view(I32)
    return b ^ ((b >> 31) & I32(0x7FFFFFFF))


def unkey(k) -> np.ndarray:
    k = np.ascontiguousarray(k, dtype=I32)
    return (k ^ ((k >> 31) & I32(0x7FFFFFFF))).view(F32)


class TrimState:
    """The selection state of P parameters; ``step`` folds one client's row."""

    def __init__(self, p: int, b: int):
        if not 1 <= b <= 8:
            raise ValueError(f"trim count {b} outside 1..8")
        self.b, self.k = b, 0
        self.lo = np.full((b, p), INT_MAX, I32)
        self.hi = np.full((b, p), INT_MIN, I32)
        self.acc = np.zeros(p, F32)
        self.kept = []  # the evicted rows, in order (for the independent check)

    def step(self, row):
        b, k = self.b, self.k
        self.k += 1
        e = key(np.asarray(row, F32).reshape(-1)).copy()
        for j in range(b):
            t = np.maximum(self.lo[j], e)
            self.lo[j] = np.minimum(self.lo[j], e)
            e = t
        if k < b:
            return
        for j in range(b):
            t = np.minimum(self.hi[j], e)
            self.hi[j] = np.maximum(self.hi[j], e)
            e = t
        if k < 2 * b:
            return
        v = unkey(e)
        self.kept.append(v.copy())
        with np.errstate(all="ignore"):
            self.acc = v.copy() if k == 2 * b else (self.acc + v).astype(F32)

    def close(self, ckpt) -> np.ndarray:
        n, b = self.k, self.b
        if n < 2 * b + 1:
            raise ValueError(f"trimmed mean with b = {b} needs at least {2 * b + 1} diffs, have {n}")
        with np.errstate(all="ignore"):
            avg = (self.acc / F32(n - 2 * b)).astype(F32)
            return (np.asarray(ckpt, F32).reshape(-1) - avg).astype(F32)


def fedavg_trimmed(ckpt, diffs, b) -> np.ndarray:
    """Flat arrays: ``ckpt`` [P], ``diffs`` N x [P] in fold order; the new checkpoint [P]."""
    st = TrimState(int(np.size(ckpt)), int(b))
    for d in diffs:
        st.step(d)
    return st.close(ckpt)


def flat(tensors) -> np.ndarray:
    return np.concatenate([np.asarray(t, F32).reshape(-1) for t in tensors])


def fedavg_trimmed_tensors(model_params, diffs, b):
    """Tensor lists in and out, like ``oracle.fedavg_mean``."""
    out = fedavg_trimmed(flat(model_params), [flat(d) for d in diffs], b)
    res, off = [], 0
    for p in model_params:
        n = int(np.size(p))
        res.append(out[off:off + n].reshape(np.shape(p)))
        off += n
    return res


def same_bits(a, b) -> bool:
    """Bit-equal f32 arrays, except that NaNs only have to sit at the same positions."""
    a = np.ascontiguousarray(a, F32).reshape(-1)
    b = np.ascontiguousarray(b, F32).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
