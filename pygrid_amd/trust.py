"""Trust-bootstrapped FedAvg (FLTrust: Cao, Fang, Liu, Gong, NDSS 2021; the arithmetic is defined in
``include/pgh_api.h``, the inner products are kernel K14's).

``server_config["diff_trust_root"] = True``: the server computes an update of its own from a small clean root
dataset and the cycle's checkpoint (the operator's provider does that, ``node.install(trust_root=fn)``), and
every reported diff is scored against it: a diff pointing away from the root gets trust 0, every other diff is
rescaled to the root's norm and weighted by its cosine to the root.  Unlike every rule of ``robust.KINDS`` it
holds against a hostile MAJORITY.  An absent key, ``None`` or ``False`` leaves the rule off.

It is not a row of ``robust.KINDS``: it needs a second input, the root, that no other rule has.  It is wired the
way ``krum.py`` is -- a field of ``settings.CloseSettings`` -- but it IS the cycle's averaging mode
(``TRUSTED_MEAN``, where the dispatch gives ``MEAN``), so it stands beside no rule, no weights, no iterative
plan and no ``dp_noise``; a ``diff_krum`` selection may run first, and a server optimizer may apply the result.
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import Optional

import numpy as np

from .exceptions import AggregationError, PlanNotAcceleratedError, TrustUnavailableError
from .robust import UNSET

TRUST_KEY = "diff_trust_root"


@dataclasses.dataclass(frozen=True)
class TrustSpec:
    """A parsed ``diff_trust_root`` setting: the rule is on (it has no parameter; the root comes per cycle)."""
    on: bool = True


def trust_of(server_config: dict, trust=UNSET) -> Optional[TrustSpec]:
    """The FL process's trust setting, or None.  ``trust`` given overrides the ``server_config`` key (``None``:
    off).  ``True`` turns the rule on; absent, ``None`` or ``False`` leaves it off; anything else raises
    ``AggregationError``: a mistyped setting must not quietly mean "trust every diff"."""
    cfg = server_config.get(TRUST_KEY, None) if trust is UNSET else trust
    if isinstance(cfg, TrustSpec):
        return cfg if cfg.on else None
    if cfg is None or (isinstance(cfg, (bool, np.bool_)) and not cfg):
        return None
    if isinstance(cfg, (bool, np.bool_)):
        return TrustSpec()
    raise AggregationError(f"{TRUST_KEY} must be True, False or None, not {cfg!r}")


def refuse(why: str) -> TrustUnavailableError:
    return TrustUnavailableError(f"{TRUST_KEY} {why}")


@contextlib.contextmanager
def failing_closed(spec: Optional[TrustSpec], what: str = "the engine does not average this cycle"):
    """Under the rule, a ``PlanNotAcceleratedError`` raised in the block becomes a ``TrustUnavailableError``:
    the caller must not fall back to the node's own averaging, which trusts every diff."""
    try:
        yield
    except PlanNotAcceleratedError as e:
        if spec is None:
            raise
        raise refuse(f"is set but {what} ({e}); the node's own averaging trusts every diff") from e


def set_on_engine(engine, spec: Optional[TrustSpec]) -> None:
    """Before a cycle's first ingest: the rule on or off.  An engine without ``set_trust``, or one that answers
    PGH_E_UNSUPPORTED (a group, a sub-range shard), fails the cycle under the rule and is left alone without it."""
    fn = getattr(engine, "set_trust", None)
    if spec is None:
        if fn is not None:
            with contextlib.suppress(AggregationError):  # (off is always accepted; a stand-in may not know it)
                fn(False)
        return
    if fn is None:
        raise refuse("is set but the engine has no set_trust")
    try:
        fn(True)
    except AggregationError as e:
        if e.status != -6:  # PGH_E_UNSUPPORTED
            raise
        raise refuse(f"is set but this engine cannot apply it: {e}") from e


def root_flat(root, numel) -> np.ndarray:
    """The server's root update as one float32 [P] array.  ``root`` may be State bytes shaped like a diff, a
    sequence of arrays (one per tensor of the model) or a flat array; ``numel``: the model's tensor sizes.  A
    layout that is not the model's raises ``TrustUnavailableError``."""
    numel = [int(n) for n in numel]
    P = sum(numel)
    if root is None:
        raise refuse("is set but the cycle has no root update")
    if isinstance(root, (bytes, bytearray, memoryview)):
        from . import state_schema

        try:
            tensors = state_schema.parse_state(bytes(root))
        except Exception as e:  # noqa: BLE001 -- whatever the parser raises: the root is unusable
            raise refuse(f"is set but the root's State bytes do not parse: {e}") from e
        root = tensors
    if isinstance(root, np.ndarray) and root.ndim == 1 and root.dtype != object:  # a flat array
        flat = np.ascontiguousarray(root, dtype=np.float32)
    else:  # one array per tensor of the model
        parts = [np.asarray(t, dtype=np.float32).reshape(-1) for t in root]
        if [p.size for p in parts] != numel:
            raise refuse(f"is set but the root has tensors of {[p.size for p in parts][:8]} values, the model of {numel[:8]}")
        flat = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    if flat.size != P:
        raise refuse(f"is set but the root has {flat.size} values, the model {P}")
    return flat


def set_root(engine, root, numel) -> None:
    """The cycle's root onto the engine (after ``set_on_engine``, after the engine was reset or reserved for the
    cycle): a root the engine refuses -- a NaN, an infinity, all zeros -- fails the cycle."""
    flat = root_flat(root, numel)
    try:
        engine.trust_root(flat)
    except TrustUnavailableError:
        raise
    except AggregationError as e:
        if e.status not in (-1, -3, -6):  # PGH_E_ARG (an unusable root), PGH_E_STATE, PGH_E_UNSUPPORTED
            raise
        raise refuse(f"is set but the engine refuses the root: {e}") from e


@contextlib.contextmanager
def closing(spec: Optional[TrustSpec]):
    """Around the FINAL fold under the rule: the engine's PGH_E_STATE (no finite diff, no trusted diff, no root)
    and PGH_E_UNSUPPORTED become ``TrustUnavailableError``."""
    try:
        yield
    except TrustUnavailableError:
        raise
    except AggregationError as e:
        if spec is None or e.status not in (-3, -6):
            raise
        raise refuse(f"is set but the engine cannot close this cycle under it: {e}") from e


def close_stats(engine) -> dict:
    """The rule's entry of ``last_close``, read from the engine after the close."""
    ts = engine.trust_stats()
    return {"trusted": int(ts["trusted"]), "excluded": int(ts["excluded"]), "total_trust": float(ts["total_trust"]),
            "max_weight": float(ts["max_weight"]), "root_norm": float(ts["root_norm"])}
