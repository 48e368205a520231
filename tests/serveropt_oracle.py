"""Oracle of the server optimizers (include/pgh_api.h "server optimizers", kernel K10): a numpy float32
restatement with one ufunc per rounding, and a scalar one through ``struct`` that shares no code with it.

``g`` is the cycle's average as its mode defines it.  The averaging oracles of the project return
``ckpt - g``; ``avg_from(close)`` takes ``g`` out of them the way the library does: the close against a
checkpoint of -0.0f gives (-0) - g = -g bit for bit for every non-NaN g, and the sign bit is flipped.
"""
from __future__ import annotations

import math
import struct

import numpy as np

F32 = np.float32
U32 = np.uint32
NONE, MOMENTUM, ADAGRAD, ADAM, YOGI = 0, 1, 2, 3, 4
KINDS = (MOMENTUM, ADAGRAD, ADAM, YOGI)
KIND_NAMES = {MOMENTUM: "fedavgm", ADAGRAD: "fedadagrad", ADAM: "fedadam", YOGI: "fedyogi"}


def flip(x) -> np.ndarray:
    """x with its sign bit flipped (exact negation, NaNs included)."""
    return (np.ascontiguousarray(x, F32).view(U32) ^ U32(0x80000000)).view(F32)


def avg_from(close, p: int) -> np.ndarray:
    """``close(ckpt) -> ckpt - g`` (flat float32 [p]) -> g."""
    return flip(close(np.full(p, -0.0, F32)))


def init_state(p: int, tau) -> tuple:
    tau = F32(tau)
    return np.zeros(p, F32), np.full(p, tau * tau, F32)


def step(kind: int, ckpt, g, m, v, lr, beta1, beta2, tau):
    """One close: ``(out, m', v')``; every line is one rounded float32 operation per element."""
    ckpt, g, m, v = (np.ascontiguousarray(a, F32) for a in (ckpt, g, m, v))
    lr, beta1, beta2, tau = F32(lr), F32(beta1), F32(beta2), F32(tau)
    c1 = F32(1.0) - beta1
    c2 = F32(1.0) - beta2
    with np.errstate(all="ignore"):
        if kind == MOMENTUM:
            t = beta1 * m
            m2 = t + g
            u = lr * m2
            return ckpt - u, m2, v
        t = beta1 * m
        w = c1 * g
        m2 = t + w
        q = g * g
        if kind == ADAGRAD:
            v2 = v + q
        elif kind == ADAM:
            a = beta2 * v
            b = c2 * q
            v2 = a + b
        elif kind == YOGI:
            s = np.where(v > q, F32(1.0), np.where(v < q, F32(-1.0), F32(0.0))).astype(F32)
            b = c2 * q
            e = b * s
            v2 = v - e
        else:
            raise ValueError(kind)
        num = lr * m2
        r = np.sqrt(v2)
        den = r + tau
        quo = num / den
        out = ckpt - quo
    for a in (out, m2, v2):
        assert a.dtype == F32
    return out, m2, v2


# ---- the scalar restatement: Python floats (binary64), each result rounded to binary32 by struct ----
# A binary64 +, -, *, / or sqrt of two binary32 values, rounded to binary32, is the correctly rounded
# binary32 operation (53 >= 2 * 24 + 2: double rounding is innocuous for these five).

def r32(x: float) -> float:
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def _sqrt(x: float) -> float:
    if x != x or x < 0:
        return math.nan
    return math.sqrt(x) if x != math.inf else math.inf


def _div(a: float, b: float) -> float:
    if b == 0:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    if abs(a) == math.inf and abs(b) == math.inf:
        return math.nan
    return a / b


def _mul(a: float, b: float) -> float:
    if (a == 0 and abs(b) == math.inf) or (b == 0 and abs(a) == math.inf):
        return math.nan
    return a * b


def step_scalar(kind: int, ckpt: float, g: float, m: float, v: float, lr, beta1, beta2, tau):
    lr, beta1, beta2, tau = (r32(float(x)) for x in (lr, beta1, beta2, tau))
    c1 = r32(1.0 - beta1)
    c2 = r32(1.0 - beta2)
    if kind == MOMENTUM:
        m2 = r32(r32(_mul(beta1, m)) + g)
        return r32(ckpt - r32(_mul(lr, m2))), m2, v
    m2 = r32(r32(_mul(beta1, m)) + r32(_mul(c1, g)))
    q = r32(_mul(g, g))
    if kind == ADAGRAD:
        v2 = r32(v + q)
    elif kind == ADAM:
        v2 = r32(r32(_mul(beta2, v)) + r32(_mul(c2, q)))
    else:
        s = 1.0 if v > q else -1.0 if v < q else 0.0
        v2 = r32(v - r32(_mul(r32(_mul(c2, q)), s)))
    den = r32(r32(_sqrt(v2)) + tau)
    return r32(ckpt - r32(_div(r32(_mul(lr, m2)), den))), m2, v2


def same_bits(a, b) -> bool:
    """Bit-identical, any NaN equal to any NaN."""
    a = np.ascontiguousarray(a, F32).reshape(-1)
    b = np.ascontiguousarray(b, F32).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(U32)[~na], b.view(U32)[~nb]))


def run_cycles(kind, ckpt, gs, hp, m=None, v=None):
    """Consecutive committed cycles with the state carried: ``gs`` one average per cycle.  Returns the
    list of ``(out, m, v)`` after each cycle; each cycle's ``out`` is the next one's checkpoint."""
    p = np.size(ckpt)
    if m is None:
        m, v = init_state(p, hp["tau"])
    res = []
    ck = np.ascontiguousarray(ckpt, F32)
    for g in gs:
        ck, m, v = step(kind, ck, g, m, v, hp["lr"], hp["beta1"], hp["beta2"], hp["tau"])
        res.append((ck, m, v))
    return res
