"""Oracle of the DP noise of the clipped close (include/pgh_api.h "Gaussian noise on the clipped close",
kernel K11): Philox4x32-10 in uint64 arrays, the Marsaglia polar method as a masked attempt loop, and the
fdlibm-form logarithm ``plog`` -- every operation one IEEE f64 (or, at the close, f32) operation, no libm.
A scalar pure-Python restatement (``normals_scalar``) shares no code with the array one.  Test
infrastructure only: the product has no CPU path.  tests/golden/dp_cases.npz (tests/gen_dp_golden.py) pins
what this file computed when the definition was written.
"""
from __future__ import annotations

import math
import struct

import numpy as np

F32 = np.float32
F64 = np.float64
U32 = np.uint32
U64 = np.uint64
I64 = np.int64

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
ATTEMPTS = 32

LN2 = float.fromhex("0x1.62e42fefa39efp-1")
LG = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
      1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)  # Lg1 .. Lg7
SQRT2_MANT = 0x6A09E667F3BCD
TWO_M52 = 2.0 ** -52


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------

def philox(c0, c1, c2, c3, k0, k1):
    """Counter words and key words (arrays or ints, each < 2**32) -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3, k0, k1 = (np.atleast_1d(np.asarray(x, dtype=U64)) for x in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    m32, s32 = U64(MASK32), U64(32)
    for r in range(10):
        p0 = U64(M0) * c0          # < 2**64: exact
        p1 = U64(M1) * c2
        h0, l0 = p0 >> s32, p0 & m32
        h1, l1 = p1 >> s32, p1 & m32
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0 = (k0 + U64(W0)) & m32
        k1 = (k1 + U64(W1)) & m32
    return c0, c1, c2, c3


# ---- plog -------------------------------------------------------------------------------------------------

def plog(s) -> np.ndarray:
    """The definition's logarithm of normal f64 values in (0, 1)."""
    s = np.ascontiguousarray(s, dtype=F64)
    b = s.view(U64)
    e = ((b >> U64(52)) & U64(0x7FF)).astype(I64) - I64(1023)
    mb = b & U64(0xFFFFFFFFFFFFF)
    big = mb >= U64(SQRT2_MANT)
    e = e + big.astype(I64)
    m = (mb | np.where(big, U64(0x3FE0000000000000), U64(0x3FF0000000000000))).view(F64)
    f = m - F64(1.0)
    t = f / (F64(2.0) + f)
    w = t * t
    R = np.full(s.shape, LG[6], dtype=F64)
    for c in LG[5::-1]:
        R = R * w
        R = R + F64(c)
    R = R * w
    return e.astype(F64) * F64(LN2) + (f - t * (f - R))


# ---- standard normals -------------------------------------------------------------------------------------

def _uniform(lo, hi) -> np.ndarray:
    q = (((hi << U64(32)) | lo).view(I64)) >> I64(11)  # arithmetic
    return (q.astype(F64) + F64(0.5)) * F64(TWO_M52)


def pair_normals(key: int, rnd: int, pairs, want_attempts: bool = False):
    """``(Z0, Z1)`` of the listed pair indices (f64 arrays); with want_attempts also the accepted attempt
    (0-based; ATTEMPTS where every one was rejected)."""
    p = np.ascontiguousarray(pairs, dtype=U64).reshape(-1)
    k0, k1 = int(key) & MASK32, (int(key) >> 32) & MASK32
    z0 = np.zeros(p.size, F64)
    z1 = np.zeros(p.size, F64)
    took = np.full(p.size, ATTEMPTS, np.int32)
    todo = np.arange(p.size)
    for a in range(ATTEMPTS):
        if todo.size == 0:
            break
        pp = p[todo]
        x0, x1, x2, x3 = philox(pp & U64(MASK32), pp >> U64(32), int(rnd) & MASK32, a, k0, k1)
        v1 = _uniform(x0, x1)
        v2 = _uniform(x2, x3)
        s = v1 * v1 + v2 * v2
        ok = s < F64(1.0)
        so, v1o, v2o = s[ok], v1[ok], v2[ok]
        L = plog(so)
        f = np.sqrt((F64(-2.0) * L) / so)
        z0[todo[ok]] = v1o * f
        z1[todo[ok]] = v2o * f
        took[todo[ok]] = a
        todo = todo[~ok]
    return (z0, z1, took) if want_attempts else (z0, z1)


def normals(key: int, rnd: int, i0: int, n: int) -> np.ndarray:
    """``Z_i`` for the flat model indices [i0, i0 + n): pair i >> 1, even i takes Z0, odd i Z1."""
    if n <= 0:
        return np.zeros(0, F64)
    p_lo, p_hi = i0 >> 1, (i0 + n - 1) >> 1
    z0, z1 = pair_normals(key, rnd, np.arange(p_lo, p_hi + 1, dtype=np.uint64))
    z = np.empty(2 * z0.size, F64)
    z[0::2] = z0
    z[1::2] = z1
    start = i0 - 2 * p_lo
    return np.ascontiguousarray(z[start:start + n])


# ---- the close ----------------------------------------------------------------------------------------------

def sigma_of(z, c, n: int) -> float:
    """``((double)z * (double)C) / (double)N`` with z and C float32."""
    return float((F64(F32(z)) * F64(F32(c))) / F64(n))


def noise(key: int, rnd: int, z, c, n: int, p: int, i0: int = 0) -> np.ndarray:
    """``n_i = (float)(sigma * Z_i)`` for the model indices [i0, i0 + p)."""
    return (F64(sigma_of(z, c, n)) * normals(key, rnd, i0, p)).astype(F32)


def noised_avg(g, key: int, rnd: int, z, c, n: int) -> np.ndarray:
    """``g' = g + n`` in f32 (g: the clipped average of the whole model, flat)."""
    g = np.ascontiguousarray(g, F32).reshape(-1)
    with np.errstate(all="ignore"):
        return (g + noise(key, rnd, z, c, n, g.size)).astype(F32)


def close(ckpt, g, key: int, rnd: int, z, c, n: int) -> np.ndarray:
    """Without a server optimizer: ``out = ckpt - g'``."""
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(ckpt, F32).reshape(-1) - noised_avg(g, key, rnd, z, c, n)).astype(F32)


# ---- the scalar restatement: Python ints and floats (binary64), shares nothing with the above ----------------

def philox_scalar(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0 = M0 * c0
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0 = (k0 + W0) & MASK32
        k1 = (k1 + W1) & MASK32
    return c0, c1, c2, c3


def plog_scalar(s: float) -> float:
    b = struct.unpack("<Q", struct.pack("<d", s))[0]
    e = ((b >> 52) & 0x7FF) - 1023
    mb = b & 0xFFFFFFFFFFFFF
    if mb >= SQRT2_MANT:
        e += 1
        mb |= 0x3FE0000000000000
    else:
        mb |= 0x3FF0000000000000
    m = struct.unpack("<d", struct.pack("<Q", mb))[0]
    f = m - 1.0
    t = f / (2.0 + f)
    w = t * t
    R = LG[6]
    for c in (LG[5], LG[4], LG[3], LG[2], LG[1], LG[0]):
        R = R * w + c      # two operations, each rounded (Python has no FMA in `*` and `+`)
    R = R * w
    return float(e) * LN2 + (f - t * (f - R))


def _uniform_scalar(lo: int, hi: int) -> float:
    q = (hi << 32) | lo
    if q >= 1 << 63:
        q -= 1 << 64
    q >>= 11  # Python's >> on a negative int is arithmetic
    return (float(q) + 0.5) * TWO_M52


def pair_normals_scalar(key: int, rnd: int, p: int):
    kw = (key & MASK32, (key >> 32) & MASK32)
    for a in range(ATTEMPTS):
        x0, x1, x2, x3 = philox_scalar((p & MASK32, (p >> 32) & MASK32, rnd & MASK32, a), kw)
        v1 = _uniform_scalar(x0, x1)
        v2 = _uniform_scalar(x2, x3)
        s = v1 * v1 + v2 * v2
        if s < 1.0:
            f = math.sqrt((-2.0 * plog_scalar(s)) / s)  # (correctly rounded)
            return v1 * f, v2 * f
    return 0.0, 0.0


def bits64(a) -> np.ndarray:
    return np.ascontiguousarray(a, F64).view(U64)


def bits32(a) -> np.ndarray:
    return np.ascontiguousarray(a, F32).view(U32)
