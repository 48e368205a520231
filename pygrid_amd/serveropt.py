"""Server optimizers at the cycle close: how the average is applied to the checkpoint.

``server_config["server_optimizer"] = {"name": "fedavgm" | "fedadagrad" | "fedadam" | "fedyogi",
"lr": ..., "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}`` (Hsu et al. 2019; Reddi et al. 2021,
Algorithm 2; the arithmetic is defined in ``include/pgh_api.h``).  An absent key or ``None`` leaves
the plain ``ckpt - avg``.

The moments (m, v) live in HBM beside the checkpoint and belong to one FL process.  ``ServerOptStates``
keeps a host copy per FL process for the time another process uses the engine, and commits a step
only once the close has produced its checkpoint bytes.  The state is not persisted: a restarted
node starts every process again from m = 0, v = tau^2.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, Optional

import numpy as np

from .engine import OPT_ADAGRAD, OPT_ADAM, OPT_MOMENTUM, OPT_NONE, OPT_YOGI
from .exceptions import AggregationError, ServerOptUnavailableError

OPT_KEY = "server_optimizer"
NAMES = {"fedavgm": OPT_MOMENTUM, "fedadagrad": OPT_ADAGRAD, "fedadam": OPT_ADAM, "fedyogi": OPT_YOGI}
DEFAULTS = {"beta1": 0.9, "beta2": 0.99, "tau": 1e-3}


@dataclasses.dataclass(frozen=True)
class ServerOptSpec:
    """A parsed ``server_optimizer`` setting; the values as the float32 the engine takes."""
    name: str
    kind: int
    lr: float
    beta1: float
    beta2: float
    tau: float

    def args(self):
        return self.kind, self.lr, self.beta1, self.beta2, self.tau


def _number(name: str, x) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise AggregationError(f"{OPT_KEY}.{name} must be a number, not {x!r}")
    with np.errstate(over="ignore"):
        f = float(np.float32(x))
    if not math.isfinite(f):
        raise AggregationError(f"{OPT_KEY}.{name} must be a finite float32, not {x!r}")
    return f


def server_opt_of(server_config: dict) -> Optional[ServerOptSpec]:
    """The FL process's server optimizer, or None.  Raises ``AggregationError`` on an unknown name or
    key, a bool, a non-finite or out-of-range value or a missing ``lr`` (``beta2`` and ``tau`` are
    range-checked for the optimizers that use them)."""
    cfg = server_config.get(OPT_KEY, None)
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise AggregationError(f"{OPT_KEY} must be a dict or None, not {cfg!r}")
    unknown = sorted(set(cfg) - {"name", "lr", *DEFAULTS}, key=str)
    if unknown:
        raise AggregationError(f"{OPT_KEY} has unknown keys {unknown}")
    name = cfg.get("name")
    if not isinstance(name, str) or name not in NAMES:
        raise AggregationError(f"{OPT_KEY}.name must be one of {sorted(NAMES)}, not {name!r}")
    if "lr" not in cfg:
        raise AggregationError(f"{OPT_KEY}.lr is required")
    kind = NAMES[name]
    val = {"lr": _number("lr", cfg["lr"]), **{k: _number(k, cfg.get(k, d)) for k, d in DEFAULTS.items()}}
    if not val["lr"] > 0:
        raise AggregationError(f"{OPT_KEY}.lr must be > 0, not {cfg['lr']!r}")
    if not 0 <= val["beta1"] < 1:
        raise AggregationError(f"{OPT_KEY}.beta1 must be in [0, 1) as a float32, not {cfg.get('beta1')!r}")
    if kind in (OPT_ADAM, OPT_YOGI) and not 0 <= val["beta2"] < 1:
        raise AggregationError(f"{OPT_KEY}.beta2 must be in [0, 1) as a float32, not {cfg.get('beta2')!r}")
    if kind != OPT_MOMENTUM and not val["tau"] > 0:
        raise AggregationError(f"{OPT_KEY}.tau must be > 0 as a float32, not {cfg.get('tau')!r}")
    # what the optimizer does not use is normalised away, so that equal behaviour compares equal
    beta2 = val["beta2"] if kind in (OPT_ADAM, OPT_YOGI) else 0.0
    tau = val["tau"] if kind != OPT_MOMENTUM else 0.0
    return ServerOptSpec(name, kind, val["lr"], val["beta1"], beta2, tau)


@dataclasses.dataclass
class _Held:
    spec: ServerOptSpec
    m: Optional[np.ndarray] = None  # host copy of the committed moments while another key is resident
    v: Optional[np.ndarray] = None
    steps: int = 0


def evict(engine) -> None:
    """Whoever's moments are resident on ``engine``: their committed state goes to that owner's host
    copy (a pending, uncommitted step is dropped) and the engine has no owner.  Call it before
    anything that drops the state in HBM (a new layout or shard)."""
    owner = getattr(engine, "opt_owner", None)
    if owner is None:
        return
    states, key = owner
    held = states._held.get(key)
    if held is not None:
        held.m, held.v = engine.server_opt_state()
    engine.opt_owner = None


class ServerOptStates:
    """The server-optimizer state of every FL process (``key``) that closes cycles on engines shared
    with others.  ``engine.opt_owner`` says whose moments are in HBM, like ``ckpt_owner``."""

    def __init__(self):
        self._held: Dict[object, _Held] = {}

    def steps(self, key) -> int:
        return self._held[key].steps if key in self._held else 0

    def state(self, engine, key):
        """``(m, v, steps)`` of ``key``: from HBM when resident on ``engine``, else the host copy."""
        held = self._held[key]
        if getattr(engine, "opt_owner", None) == (self, key):
            m, v = engine.server_opt_state()
            return m, v, held.steps
        return held.m, held.v, held.steps

    def bind(self, engine, key, spec: Optional[ServerOptSpec], numel: int) -> None:
        """Before the fold (and after the engine has its layout): the engine runs ``spec`` on
        ``key``'s moments.  ``spec`` None: no optimizer, so a shared engine never carries one over."""
        if spec is None:
            if hasattr(engine, "set_server_opt"):
                evict(engine)
                engine.set_server_opt(OPT_NONE)
            return
        if key is None:
            raise AggregationError(f"{OPT_KEY} is set but the close has no opt_key (the FL process id) to keep "
                                   "its state under")
        if not hasattr(engine, "set_server_opt"):
            raise ServerOptUnavailableError(f"{OPT_KEY} is set but the engine has no set_server_opt")
        held = self._held.get(key)
        if held is not None and (held.spec != spec or (held.m is not None and held.m.size != numel)):
            held = None  # a changed setting or model starts again from m = 0, v = tau^2
        try:
            if held is not None and getattr(engine, "opt_owner", None) == (self, key):
                engine.set_server_opt(*spec.args())  # the same again: the state stays
                return
            evict(engine)
            engine.set_server_opt(OPT_NONE)  # (the same spec left by another key must not keep that key's state)
            engine.set_server_opt(*spec.args())
            if held is None or held.m is None:  # (no host copy and not resident: the state was dropped)
                held = self._held[key] = _Held(spec)
            else:
                engine.load_server_opt_state(held.m, held.v)
        except AggregationError as e:
            if e.status != -6:  # PGH_E_UNSUPPORTED
                raise
            raise ServerOptUnavailableError(f"{OPT_KEY} is set but the engine cannot run it: {e}") from e
        held.m = held.v = None  # HBM holds the truth now
        engine.opt_owner = (self, key)

    def commit(self, engine) -> None:
        """The close has its checkpoint bytes: the step counts."""
        owner = getattr(engine, "opt_owner", None)
        if owner is None or owner[0] is not self:
            return
        engine.server_opt_commit()
        self._held[owner[1]].steps += 1

