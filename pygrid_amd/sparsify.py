"""Top-k sparsification of the averaged update: SparseFed (Panda et al., AISTATS 2022).  After the diffs are
averaged (and, beside ``diff_clip_norm``, clipped) the close applies only the k coordinates of largest magnitude
and keeps the rest in a server-side error memory that is added back at the next close; the arithmetic is defined
in ``include/pgh_api.h`` (kernel K18).

``server_config["update_top_k"] = {"count": k}`` or ``{"fraction": phi}`` with ``0 < phi <= 1``, and optionally
``"error_feedback": bool`` (default ``True``).  It is a modifier behind the cycle's averaging, like the noise, not
a rule of its own (``robust.rule_of`` does not know it): it sits behind any mode, a ``diff_krum`` stage and a rule,
and ahead of a server optimizer, but not beside ``dp_noise``.  An absent key or ``None`` leaves the update dense.

The error memory lives on the engine, with the model's layout: an engine serves one FL process's sparsified cycles
at a time, and a node that restarts carries the memory over with ``Engine.topk_state`` / ``load_topk_state``.
The operator chooses k and the clip bound; the engine reports k, the threshold and the kept count per close.
"""
from __future__ import annotations

import dataclasses
import fractions
import math
from typing import Optional

import numpy as np

from .exceptions import AggregationError, TopKUnavailableError
from .robust import UNSET

TOPK_KEY = "update_top_k"
_FIELDS = {"count", "fraction", "error_feedback"}


@dataclasses.dataclass(frozen=True)
class TopKSpec:
    """A parsed ``update_top_k``: exactly one of ``count`` (k itself) and ``fraction`` (phi, 0 < phi <= 1)."""
    count: Optional[int] = None
    fraction: Optional[float] = None
    error_feedback: bool = True


def top_k_of(server_config: dict, top_k=UNSET) -> Optional[TopKSpec]:
    """The FL process's top-k setting, or None.  ``top_k`` given overrides the ``server_config`` key (``None``:
    off).  Raises ``AggregationError`` on anything but a dict, an unknown field, both of ``count`` and ``fraction``
    or neither, a ``count`` that is not an integer >= 1, a ``fraction`` that is not a float (or the int 1) in
    (0, 1], a bool where a number belongs or anything but a bool as ``error_feedback``: a mistyped setting must not
    quietly mean "the dense update"."""
    cfg = server_config.get(TOPK_KEY, None) if top_k is UNSET else top_k
    if cfg is None:
        return None
    if isinstance(cfg, TopKSpec):
        return cfg
    if not isinstance(cfg, dict):
        raise AggregationError(f"{TOPK_KEY} must be a dict or None, not {cfg!r}")
    unknown = sorted(set(cfg) - _FIELDS, key=str)
    if unknown:
        raise AggregationError(f"{TOPK_KEY} has unknown fields {unknown}")
    if ("count" in cfg) == ("fraction" in cfg):
        raise AggregationError(f"{TOPK_KEY} needs exactly one of 'count' and 'fraction', not {cfg!r}")
    fb = cfg.get("error_feedback", True)
    if not isinstance(fb, (bool, np.bool_)):
        raise AggregationError(f"{TOPK_KEY}['error_feedback'] must be True or False, not {fb!r}")
    if "count" in cfg:
        k = cfg["count"]
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or int(k) < 1:
            raise AggregationError(f"{TOPK_KEY}['count'] must be an integer >= 1, not {k!r}")
        return TopKSpec(count=int(k), error_feedback=bool(fb))
    phi = cfg["fraction"]
    if isinstance(phi, (bool, np.bool_)) or not isinstance(phi, (int, float, np.integer, np.floating)) \
            or not 0.0 < float(phi) <= 1.0:  # (a NaN compares false)
        raise AggregationError(f"{TOPK_KEY}['fraction'] must be a number with 0 < fraction <= 1, not {phi!r}")
    return TopKSpec(fraction=float(phi), error_feedback=bool(fb))


def resolve(spec: TopKSpec, n_params: int) -> int:
    """k for a model of ``n_params`` parameters.  A fraction resolves as ``ceil(P * phi)`` with phi the decimal the
    operator wrote (0.1 of 1,000 is 100, not the 101 that the nearest double of 0.1 would give), as
    ``diff_trimmed_mean`` resolves its own; a count larger than the model raises ``TopKUnavailableError``."""
    if spec.count is not None:
        if spec.count > n_params:
            raise TopKUnavailableError(f"{TOPK_KEY}['count'] = {spec.count} exceeds the model's {n_params} parameters")
        return spec.count
    return min(int(n_params), math.ceil(n_params * fractions.Fraction(str(spec.fraction))))


def refuse(why: str) -> TopKUnavailableError:
    return TopKUnavailableError(f"{TOPK_KEY} {why}")


def set_on_engine(engine, spec: Optional[TopKSpec]) -> None:
    """Before a cycle's first ingest, once the engine is laid out: the setting set, or cleared -- an engine shared
    across FL processes never carries one over.  The same k again keeps the engine's error memory.  An engine
    without ``set_topk`` that the cycle does not need is left alone; one that lacks it, or answers
    PGH_E_UNSUPPORTED (a group, a shard, a streaming context), fails the cycle."""
    if spec is None:
        if hasattr(engine, "set_topk"):
            engine.set_topk(0)
        return
    k = resolve(spec, int(sum(engine.numel)))
    try:
        engine.set_topk(k, spec.error_feedback)
    except AttributeError as e:
        raise refuse("is set but the engine has no set_topk") from e
    except AggregationError as e:
        if e.status != -6:  # PGH_E_UNSUPPORTED
            raise
        raise refuse(f"is set but this engine cannot apply it: {e}") from e


def close_stats(engine) -> dict:
    """The setting's entries of ``last_close``, read from the engine after the FINAL pass."""
    st = engine.topk_stats()
    return {"top_k": int(st["k"]), "top_k_kept": int(st["kept"]), "top_k_threshold": float(st["threshold"])}
