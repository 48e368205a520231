"""Numpy restatement of clipped FedAvg (include/pgh_api.h): the per-row sum of
squares in its one fixed order, the scale, and the clipped fold.  Test infrastructure only: the
product has no CPU path.  tests/golden/clip_cases.npz (tests/gen_clip_golden.py) pins what this file
computed when the definition was written, so an edit here cannot silently move the definition.

The order of the sum (f64 throughout; a square of an f32 is exact in f64):

* tile t covers shard params [4096 t, 4096 (t + 1)); params at or past P count as +0.0;
* lane l of 256: ``a = +0.0; for j in 0..3: for e in 0..3: a += sq(4096 t + 4 (l + 256 j) + e)``;
* per wave of 64 consecutive lanes: ``for h in 32, 16, 8, 4, 2, 1: v[l] += v[l + h]`` for l < h;
* tile partial ``((w0 + w1) + w2) + w3``; row sum = left fold of the tile partials, ascending.

The engine's fold kernel brings a row's partials into LDS ``FOLD_CHUNK`` = 1,024 at a time (``SUMSQ_FOLD_CHUNK``
in pgh_kernels.hip) and one lane carries the sum across the chunks; the definition above knows no chunks.  Three
widths in tests/gen_clip_golden.py (``WIDE_P``) are cut to that number and move with it:

* ``P_A`` = 1024 x 4096 = 4,194,304: exactly one full chunk, the loop ends on ``c0 == ntiles``;
* ``P_B`` = 1026 x 4096 - 4095 = 4,198,401: 1,026 tiles, a second chunk of two, one param in the last tile
  (``p % 4 == 1``: the clamp to the last column and the +0.0 mask);
* ``P_C`` = 2 x 1024 x 4096 + 5 x 4096 + 3 = 8,409,091: 2,054 tiles, two full chunks and one of six, a ragged
  last tile.

tests/test_row_sums_wide.py (CPU: the inputs tell a wrong chunking from the right one) and
tests/test_gpu_row_sums_wide.py (K7, K12 and the closes on them) use no other widths.
"""
from __future__ import annotations

import numpy as np

TILE = 4096
FOLD_CHUNK = 1024  # the engine's SUMSQ_FOLD_CHUNK: not part of the definition, only of where the tests look
F32 = np.float32
F64 = np.float64


def tile_partials(d) -> np.ndarray:
    d = np.ascontiguousarray(d, dtype=F32).reshape(-1)
    n_tiles = max(1, -(-d.size // TILE))
    x = np.zeros(n_tiles * TILE, dtype=F64)
    x[:d.size] = d.astype(F64)
    with np.errstate(all="ignore"):
        sq = (x * x).reshape(n_tiles, 4, 256, 4)      # [t][j][l][e]: param 4096 t + 4 (l + 256 j) + e
        a = np.zeros((n_tiles, 256), dtype=F64)
        for j in range(4):
            for e in range(4):
                a = a + sq[:, j, :, e]
        v = a.reshape(n_tiles, 4, 64).copy()          # [t][wave][lane]
        for h in (32, 16, 8, 4, 2, 1):
            v[:, :, :h] = v[:, :, :h] + v[:, :, h:2 * h]
        w = v[:, :, 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def row_sumsq(d) -> np.float64:
    parts = tile_partials(d)
    acc = F64(parts[0])
    with np.errstate(all="ignore"):
        for p in parts[1:]:
            acc = F64(acc + p)
    return acc


def scale(sumsq, c) -> np.float32:
    """``norm <= (double)C ? 1.0f : (float)((double)C / norm)``, ``norm = sqrt(sumsq)`` in f64."""
    c = F64(F32(c))
    with np.errstate(all="ignore"):
        norm = np.sqrt(F64(sumsq))
        if norm <= c:
            return F32(1.0)
        return F32(c / norm)


def scales(diffs, c) -> np.ndarray:
    return np.array([scale(row_sumsq(d), c) for d in diffs], dtype=F32)


def fold(diffs, s, ckpt) -> np.ndarray:
    """``acc = d_0 * s_0; acc = acc + d_c * s_c`` (product rounded to f32, then added);
    ``out = ckpt - acc / float(N)``."""
    n = len(diffs)
    with np.errstate(all="ignore"):
        acc = (np.asarray(diffs[0], F32).reshape(-1) * F32(s[0])).astype(F32)
        for d, sc in zip(diffs[1:], s[1:]):
            acc = (acc + (np.asarray(d, F32).reshape(-1) * F32(sc)).astype(F32)).astype(F32)
        avg = (acc / F32(n)).astype(F32)
        return (np.asarray(ckpt, F32).reshape(-1) - avg).astype(F32)


def fedavg_clipped(ckpt, diffs, c) -> np.ndarray:
    """Flat arrays: ``ckpt`` [P], ``diffs`` N x [P]; the new checkpoint [P]."""
    return fold(diffs, scales(diffs, c), ckpt)


def flat(tensors) -> np.ndarray:
    return np.concatenate([np.asarray(t, F32).reshape(-1) for t in tensors])


def fedavg_clipped_tensors(model_params, diffs, c):
    """Tensor lists in and out, like ``oracle.fedavg_mean``: the norm is over the whole model."""
    out = fedavg_clipped(flat(model_params), [flat(d) for d in diffs], c)
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
