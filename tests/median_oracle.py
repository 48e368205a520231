"""Numpy restatement of the coordinate-wise median (PGH_MEDIAN; DESIGN.md section 5,
include/pgh_api.h).  Test infrastructure only: the product has no CPU path.
tests/golden/median_cases.npz (tests/gen_median_golden.py) pins what this file computed when the
definition was written, so an edit here cannot silently move the definition.

Values are ordered by the trimmed mean's int32 key (``trim_oracle.key``: a total order on bit
patterns, ``-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN``; ``unkey`` is the same expression;
equal keys are identical bits, so ties need no rule).  Per parameter, ``s = sort(keys of the N
reported values)``:

* N odd: ``m = unkey(s[(N - 1) / 2])``;
* N even: ``a = unkey(s[N / 2 - 1])``, ``b = unkey(s[N / 2])``, ``m = 0.5f * a + 0.5f * b`` -- two
  f32 products, each rounded, then one f32 addition (not ``(a + b) / 2``: two middles of 3e38 give
  3e38; a ``-inf`` and a ``+inf`` middle give NaN);

and ``out = ckpt - m``, one f32 subtraction.  Nothing depends on the order of the rows.
"""
from __future__ import annotations

import numpy as np

from trim_oracle import flat, key, same_bits, unkey  # noqa: F401  (same_bits: re-exported)

F32 = np.float32


def median_of_rows(diffs) -> np.ndarray:
    """``m`` per parameter: ``diffs`` N x [P] (any order)."""
    d = np.stack([np.asarray(r, F32).reshape(-1) for r in diffs])
    n = d.shape[0]
    s = np.sort(key(d).reshape(d.shape), axis=0)
    if n & 1:
        return unkey(s[(n - 1) // 2])
    a, b = unkey(s[n // 2 - 1]), unkey(s[n // 2])
    with np.errstate(all="ignore"):
        return ((F32(0.5) * a).astype(F32) + (F32(0.5) * b).astype(F32)).astype(F32)


def fedavg_median(ckpt, diffs) -> np.ndarray:
    """Flat arrays: ``ckpt`` [P], ``diffs`` N x [P]; the new checkpoint [P]."""
    with np.errstate(all="ignore"):
        return (np.asarray(ckpt, F32).reshape(-1) - median_of_rows(diffs)).astype(F32)


def fedavg_median_tensors(model_params, diffs):
    """Tensor lists in and out, like ``oracle.fedavg_mean``."""
    out = fedavg_median(flat(model_params), [flat(d) for d in diffs])
    res, off = [], 0
    for p in model_params:
        n = int(np.size(p))
        res.append(out[off:off + n].reshape(np.shape(p)))
        off += n
    return res
