"""Nearest-neighbour mixing of a cycle's diffs ahead of its average (Allouah et al., "Fixing by Mixing", AISTATS
2023; the arithmetic is defined in ``include/pgh_api.h``, "Row mixing", the mix is kernel K19's).

``server_config["diff_nnm"] = {"byzantine": f, "distances": optional kind}``: every finite diff is replaced by the
mean of its ``n' - f`` nearest diffs among the ``n'`` finite ones (itself included), and the cycle's rule then runs
over the mixed diffs exactly as if they were the only reports.  With non-iid clients the honest diffs are spread
out and the coordinate-wise rules lose their guarantees; the mixing restores them.  An absent key, ``None`` or
``False`` mixes nothing.  ``"distances"``: ``"exact"`` (the default: K13), ``"gram"`` (K16) or ``"gram_bf16"`` (K20), as under ``diff_krum``.

A mixing is a stage, not an averaging rule (``robust.rule_of`` does not know it).  The mixed diffs are new rows:
they go into slots of their own, so the stage DOUBLES the slab's slot count (n diffs take 2 n slots).  Behind it run
the plain mean, the trimmed means (by count and by rank), the median and the mean around the median, with or without
a server optimizer and ``update_top_k``; everything else -- a selection, Bulyan, the trust rule, clipping and noise,
the geometric median, weights, the iterative plan -- is refused before anything is ingested: the row-wise rules
would need per-row sums of the mixed rows.
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .engine import MEAN, MEAN_AROUND_MEDIAN, MEDIAN, RANK_TRIMMED_MEAN, TRIMMED_MEAN
from .exceptions import AggregationError, NnmUnavailableError, PlanNotAcceleratedError
from .krum import DISTANCES, distances_of
from .robust import UNSET

NNM_KEY = "diff_nnm"
_FIELDS = ("byzantine", "distances")
MODES = (MEAN, TRIMMED_MEAN, MEDIAN, MEAN_AROUND_MEDIAN, RANK_TRIMMED_MEAN)  # what runs over mixed diffs


@dataclasses.dataclass(frozen=True)
class NnmSpec:
    """A parsed ``diff_nnm`` setting: the assumed hostile count and the distance kind."""
    byzantine: int
    distances: str = "exact"


def nnm_of(server_config: dict, nnm=UNSET) -> Optional[NnmSpec]:
    """The FL process's mixing, or None.  ``nnm`` given overrides the ``server_config`` key (``None``: off).
    ``{"byzantine": f}`` (an int >= 0) is required, ``"distances"`` (one of ``krum.DISTANCES``) optional.  Anything
    else -- another type, an unknown key, a bool where a number belongs, a float with a fraction, a negative count --
    raises ``AggregationError``: a mistyped setting must not quietly mean "unmixed"."""
    cfg = server_config.get(NNM_KEY, None) if nnm is UNSET else nnm
    if cfg is None or (isinstance(cfg, (bool, np.bool_)) and not cfg):
        return None
    if isinstance(cfg, NnmSpec):
        return cfg
    if not isinstance(cfg, dict):
        raise AggregationError(f"{NNM_KEY} must be a dict of {_FIELDS}, None or False, not {cfg!r}")
    unknown = [k for k in cfg if k not in _FIELDS]
    if unknown:
        raise AggregationError(f"{NNM_KEY} has unknown keys {unknown!r} (known: {_FIELDS})")
    if "byzantine" not in cfg:
        raise AggregationError(f"{NNM_KEY}['byzantine'] is required")
    f = cfg["byzantine"]
    bad = AggregationError(f"{NNM_KEY}['byzantine'] must be an integer >= 0, not {f!r}")
    if isinstance(f, (bool, np.bool_)) or not isinstance(f, (int, float, np.integer, np.floating)):
        raise bad
    if isinstance(f, (float, np.floating)) and not (np.isfinite(f) and float(f) == int(f)):
        raise bad
    if int(f) < 0:
        raise bad
    return NnmSpec(int(f), distances_of(NNM_KEY, cfg.get("distances", DISTANCES[0])))


def refuse(why: str) -> NnmUnavailableError:
    return NnmUnavailableError(f"{NNM_KEY} {why}")


@contextlib.contextmanager
def failing_closed(spec: Optional[NnmSpec], what: str = "the engine does not average this cycle"):
    """Under a mixing, a ``PlanNotAcceleratedError`` raised in the block becomes an ``NnmUnavailableError``: the
    caller must not fall back to the node's own averaging, which mixes nothing."""
    try:
        yield
    except PlanNotAcceleratedError as e:
        if spec is None:
            raise
        raise refuse(f"is set but {what} ({e}); the node's own averaging mixes nothing") from e


def check_mode(mode: int, weights=None) -> None:
    """Before anything is ingested: the cycle's mode is one the stage can stand in front of."""
    if weights is not None:
        raise refuse("cannot be combined with aggregation weights")
    if mode not in MODES:
        raise refuse(f"cannot stand in front of averaging mode {mode}: the plain mean, the trimmed means, the median "
                     "and the mean around the median run over mixed diffs")


def check_engine(engine) -> None:
    """Before anything is ingested: the engine can mix (one GPU holding whole rows).  (A shard set under another
    layout is refused too, although laying the engine out anew would drop it: the caller who sharded it re-lays it.)"""
    if getattr(engine, "mix_rows", None) is None or getattr(engine, "nnm_weights", None) is None:
        raise refuse("is set but the engine has no mix_rows")
    if getattr(engine, "is_group", False):
        raise refuse("is set but the engine is a multi-GPU group: its shards each hold part of a row")
    if getattr(engine, "P", 0) and (getattr(engine, "lo", 0), getattr(engine, "hi", engine.P)) != (0, engine.P):
        raise refuse("is set but the engine holds a sub-range shard of the model")


def mix(engine, spec: NnmSpec, slots: Sequence[int], free: Sequence[int]) -> Tuple[List[int], dict]:
    """The slots of the mixed diffs, in the order of the finite ones of ``slots``, and the stage's entry of
    ``last_close`` (``byzantine``, ``neighbours``, ``excluded``), which the caller keeps: rows with a non-finite sum of
    squares are dropped, the distances among the ``n'`` left are taken (K13 or K16), each is replaced by the mean of
    its ``n' - f`` nearest (``n' > 2 f``, else ``NnmUnavailableError``) and written to the first ``n'`` slots of
    ``free``.  Fewer free slots than rows to mix, an engine that cannot (PGH_E_UNSUPPORTED, PGH_E_STATE): the cycle
    fails with ``NnmUnavailableError`` -- it never closes unmixed."""
    check_engine(engine)
    slots, f = [int(s) for s in slots], spec.byzantine
    try:
        sums = np.asarray(engine.row_sumsq(slots), np.float64)
        inc = [s for s, ss in zip(slots, sums) if np.isfinite(ss)]
        n = len(inc)
        if n <= 2 * f:
            raise refuse(f"with byzantine = {f} needs more than {2 * f} finite diffs, the close has {n} of {len(slots)}")
        if len(free) < n:
            raise refuse(f"is set and the slab has {len(free)} free slots for {n} mixed diffs: the stage doubles the "
                         "slot count")
        if spec.distances != "exact":  # K16's matrix, or K20's: the kind reaches the engine by keyword
            kind = {"kind": "bf16"} if spec.distances == "gram_bf16" else {}
            dist = engine.gram_distances_host(engine.row_gram(inc, **kind), sums[np.isfinite(sums)])
        else:
            dist = engine.row_pairdist(inc)
        dst = [int(s) for s in free[:n]]
        engine.mix_rows(inc, dst, engine.nnm_weights(dist, f))
    except NnmUnavailableError:
        raise
    except AggregationError as e:
        if getattr(e, "status", None) not in (-6, -3):  # PGH_E_UNSUPPORTED, PGH_E_STATE
            raise
        raise refuse(f"is set but this engine cannot mix these diffs: {e}") from e
    return dst, {"byzantine": f, "neighbours": n - f, "excluded": len(slots) - n}
