"""Multi-Krum selection of a cycle's diffs ahead of its average (Blanchard et al. 2017; the arithmetic is
defined in ``include/pgh_api.h``, the distances are kernel K13's).

``server_config["diff_krum"] = {"byzantine": f, "keep": optional m}``: every diff is scored by its distance
to its ``n' - f - 2`` nearest neighbours among the ``n'`` finite diffs, the ``m`` most central ones
(default ``n' - f``; 1 is Krum) are averaged and the others leave the cycle.  An absent key, ``None`` or
``False`` selects nothing.

A selection is a stage, not an averaging rule (``robust.rule_of`` does not know it): the cycle's mode --
the plain, iterative, weighted, clipped or trimmed mean, the median, the geometric median, with or without
a server optimizer -- runs over the picked diffs exactly as if they were the only reports.  It cannot stand
beside ``dp_noise``: the clip-and-noise sensitivity argument does not cover a data-dependent selection.
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import List, Optional, Sequence

import numpy as np

from .exceptions import AggregationError, KrumUnavailableError, PlanNotAcceleratedError
from .robust import UNSET

KRUM_KEY = "diff_krum"
_FIELDS = ("byzantine", "keep")


@dataclasses.dataclass(frozen=True)
class KrumSpec:
    """A parsed ``diff_krum`` setting: the assumed hostile count and the keep count (None: all but f)."""
    byzantine: int
    keep: Optional[int] = None


def _count(name: str, v, least: int) -> int:
    bad = AggregationError(f"{KRUM_KEY}[{name!r}] must be an integer >= {least}, not {v!r}")
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise bad
    if isinstance(v, (float, np.floating)) and not (np.isfinite(v) and float(v) == int(v)):
        raise bad
    if int(v) < least:
        raise bad
    return int(v)


def krum_of(server_config: dict, krum=UNSET) -> Optional[KrumSpec]:
    """The FL process's selection, or None.  ``krum`` given overrides the ``server_config`` key (``None``:
    off).  ``{"byzantine": f}`` (an int >= 0) is required, ``"keep"`` (an int >= 1, or None) optional.
    Anything else -- another type, an unknown key, a bool where a number belongs, a float with a fraction, a
    negative count -- raises ``AggregationError``: a mistyped setting must not quietly mean "every diff"."""
    cfg = server_config.get(KRUM_KEY, None) if krum is UNSET else krum
    if cfg is None or (isinstance(cfg, (bool, np.bool_)) and not cfg):
        return None
    if isinstance(cfg, KrumSpec):
        return cfg
    if not isinstance(cfg, dict):
        raise AggregationError(f"{KRUM_KEY} must be a dict of {_FIELDS}, None or False, not {cfg!r}")
    unknown = [k for k in cfg if k not in _FIELDS]
    if unknown:
        raise AggregationError(f"{KRUM_KEY} has unknown keys {unknown!r} (known: {_FIELDS})")
    if "byzantine" not in cfg:
        raise AggregationError(f"{KRUM_KEY}['byzantine'] is required")
    keep = cfg.get("keep", None)
    return KrumSpec(_count("byzantine", cfg["byzantine"], 0), None if keep is None else _count("keep", keep, 1))


def refuse(why: str) -> KrumUnavailableError:
    return KrumUnavailableError(f"{KRUM_KEY} {why}")


@contextlib.contextmanager
def failing_closed(spec: Optional[KrumSpec], what: str = "the engine does not average this cycle"):
    """Under a selection, a ``PlanNotAcceleratedError`` raised in the block becomes a ``KrumUnavailableError``:
    the caller must not fall back to the node's own averaging, which selects nothing."""
    try:
        yield
    except PlanNotAcceleratedError as e:
        if spec is None:
            raise
        raise refuse(f"is set but {what} ({e}); the node's own averaging selects nothing") from e


def select(engine, spec: KrumSpec, slots: Sequence[int]) -> List[int]:
    """The picked slots of ``slots`` (in their order).  An engine without ``krum_select``, one that answers
    PGH_E_UNSUPPORTED (a group, a sub-range shard, too many rows) or PGH_E_STATE (too few finite diffs for
    ``f``, ``keep`` too large) fails the cycle with ``KrumUnavailableError``."""
    fn = getattr(engine, "krum_select", None)
    if fn is None:
        raise refuse("is set but the engine has no krum_select")
    try:
        return [int(s) for s in fn(list(slots), spec.byzantine, spec.keep or 0)]
    except KrumUnavailableError:
        raise
    except AggregationError as e:
        if e.status not in (-6, -3):  # PGH_E_UNSUPPORTED, PGH_E_STATE
            raise
        raise refuse(f"is set but this engine cannot select among these diffs: {e}") from e


def close_stats(engine, spec: KrumSpec) -> dict:
    """The selection's entry of ``last_close``, read from the engine after the close."""
    ks = engine.krum_stats()
    return {"byzantine": spec.byzantine, "picked": int(ks["picked"]), "excluded": int(ks["excluded"]),
            "max_picked_score": float(ks["max_picked_score"])}
