"""Gaussian noise on the clipped close: DP-FedAvg (clip every diff to C, add N(0, (z C)^2 I) to the sum,
divide by N; the arithmetic and the sampler are defined in ``include/pgh_api.h``).

``server_config["dp_noise"] = {"multiplier": z, "key": optional int}`` beside ``diff_clip_norm``, which it
requires: noise is a modifier of the clip rule, not a rule of its own (``robust.rule_of`` does not know it).
An absent key or ``None`` leaves the close un-noised.

The noise of a close is a function of ``(key, round, z, C, N, diffs)`` alone, so a retried close releases
the same noise, never a second draw.  ``key`` defaults to one ``secrets.randbits(64)`` per FL process, held
by this process (``DpKeys``, like ``ServerOptStates``; not persisted); ``round`` is the cycle's id mod 2^32.
Philox with a 64-bit key is a statistical generator, not a cryptographic one, and privacy accounting
(epsilon from z, the sampling rate and the number of rounds) is the operator's: the engine reports z, C
and N per close and no more.
"""
from __future__ import annotations

import dataclasses
import math
import secrets
import threading
from typing import Dict, Optional

import numpy as np

from .exceptions import AggregationError, DpNoiseUnavailableError
from .robust import CLIP_KEY, UNSET, Rule

DP_KEY = "dp_noise"


@dataclasses.dataclass(frozen=True)
class DpNoiseSpec:
    """A parsed ``dp_noise`` setting: the multiplier as the float32 the engine takes, the key if given."""
    multiplier: float
    key: Optional[int] = None


def dp_noise_of(server_config: dict, dp_noise=UNSET) -> Optional[DpNoiseSpec]:
    """The FL process's noise setting, or None.  ``dp_noise`` given overrides the ``server_config`` key
    (``None``: off).  Raises ``AggregationError`` on anything but a dict, an unknown key, a missing,
    mistyped (bools included), non-finite or non-positive ``multiplier`` (as a float32), or a ``key`` that
    is not an int in [0, 2^64): a mistyped setting must not quietly mean "no noise"."""
    cfg = server_config.get(DP_KEY, None) if dp_noise is UNSET else dp_noise
    if cfg is None:
        return None
    if isinstance(cfg, DpNoiseSpec):
        return cfg
    if not isinstance(cfg, dict):
        raise AggregationError(f"{DP_KEY} must be a dict or None, not {cfg!r}")
    unknown = sorted(set(cfg) - {"multiplier", "key"}, key=str)
    if unknown:
        raise AggregationError(f"{DP_KEY} has unknown keys {unknown}")
    if "multiplier" not in cfg:
        raise AggregationError(f"{DP_KEY}.multiplier is required")
    z = cfg["multiplier"]
    if isinstance(z, bool) or not isinstance(z, (int, float, np.integer, np.floating)):
        raise AggregationError(f"{DP_KEY}.multiplier must be a finite number > 0, not {z!r}")
    with np.errstate(over="ignore", under="ignore"):
        z32 = float(np.float32(z))
    if not math.isfinite(float(z)) or not math.isfinite(z32) or not z32 > 0:
        raise AggregationError(f"{DP_KEY}.multiplier must be a finite float32 > 0, not {z!r}")
    key = cfg.get("key", None)
    if key is not None:
        if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < 1 << 64:
            raise AggregationError(f"{DP_KEY}.key must be an integer in [0, 2**64), not {key!r}")
        key = int(key)
    return DpNoiseSpec(z32, key)


def check_rule(spec: Optional[DpNoiseSpec], rule: Optional[Rule]) -> None:
    """Noise needs the clip bound: without ``diff_clip_norm`` (or beside another rule) the close fails."""
    if spec is not None and (rule is None or rule.key != CLIP_KEY):
        raise DpNoiseUnavailableError(f"{DP_KEY} is set without {CLIP_KEY}: the noise is scaled by the clip bound "
                                      "(sensitivity C), so there is nothing to calibrate it to")


def round_of(cycle_id) -> int:
    """The close's ``round``: the cycle's id mod 2^32."""
    if isinstance(cycle_id, bool) or not isinstance(cycle_id, (int, np.integer)):
        raise AggregationError(f"{DP_KEY}: the round (the cycle's id) must be an integer, not {cycle_id!r}")
    return int(cycle_id) % (1 << 32)


class DpKeys:
    """The noise key of every FL process (``process``: its id) that closes noised cycles here: the
    setting's own ``key``, else one ``secrets.randbits(64)`` drawn at the process's first noised cycle and
    kept for this process's life, so that every retry of a close draws from the same stream."""

    def __init__(self):
        self._keys: Dict[object, int] = {}
        self._lock = threading.Lock()

    def key_for(self, process, spec: DpNoiseSpec) -> int:
        if spec.key is not None:
            return spec.key
        with self._lock:
            if process not in self._keys:
                self._keys[process] = secrets.randbits(64)
            return self._keys[process]


def set_on_engine(engine, spec: Optional[DpNoiseSpec], key: Optional[int] = None, rnd: Optional[int] = None) -> None:
    """Before a cycle's first ingest, after the clip bound is set: the noise set, or cleared -- an engine
    shared across FL processes never carries one over.  An engine without ``set_dp_noise`` that the cycle
    does not need is left alone; one that lacks it, or answers PGH_E_UNSUPPORTED, fails the cycle."""
    if spec is None:
        if hasattr(engine, "set_dp_noise"):
            engine.set_dp_noise(0.0)
        return
    if rnd is None:
        raise DpNoiseUnavailableError(f"{DP_KEY} is set but the close has no dp_round (the cycle's id): two cycles "
                                      "must never share a round")
    if key is None:
        raise DpNoiseUnavailableError(f"{DP_KEY} is set but the close has no key")
    try:
        engine.set_dp_noise(spec.multiplier, key, round_of(rnd))
    except AttributeError as e:
        raise DpNoiseUnavailableError(f"{DP_KEY} is set but the engine has no set_dp_noise") from e
    except AggregationError as e:
        if e.status != -6:  # PGH_E_UNSUPPORTED
            raise
        raise DpNoiseUnavailableError(f"{DP_KEY} is set but this engine cannot apply it: {e}") from e
