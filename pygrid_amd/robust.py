"""The robust-aggregation rules an FL process can ask for in its ``server_config`` -- per-client L2
clipping, the coordinate-wise trimmed mean, the coordinate-wise median, the geometric median (none has a
reference counterpart) -- and what the host layer does with them, once:

* ``KINDS`` is the only place that ties a rule to its config key, the engine mode it turns ``MEAN``
  into, its error class and its engine setter.  A new defence is a new row (and a new class in
  ``exceptions.py`` only if callers must tell its failures apart);
* ``rule_of`` parses the settings and gives the single active ``Rule`` (or None).  At most one rule
  applies to a cycle: a combination is refused with the error of the rule earlier in ``KINDS``;
* ``failing_closed`` is the rule's fail-closed decision: where a rule is set, "the engine does not run
  this cycle" (``PlanNotAcceleratedError``, on which callers fall back to the node's own averaging)
  becomes the rule's error -- the node's averaging applies no rule, so the close fails instead;
* ``set_on_engine`` puts a rule onto an engine before a cycle's first ingest.

These two are the rule's part of ``settings.CloseSettings`` -- a cycle's rule, server optimizer and noise,
parsed once -- which is what the call sites hold.  Sits below it (imports only ``engine`` and ``exceptions``).
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import Optional

import numpy as np

from .engine import CLIPPED_MEAN, GEOMED_MAX_ITERS, GEOMETRIC_MEDIAN, MEDIAN, TRIMMED_MEAN, TRIM_MAX
from .exceptions import AggregationError, ClipUnavailableError, GeometricMedianUnavailableError, \
    MedianUnavailableError, PlanNotAcceleratedError, TrimUnavailableError

CLIP_KEY = "diff_clip_norm"  # optional server_config key: the per-client L2 bound (no reference counterpart)


def clip_norm_of(server_config: dict) -> Optional[float]:
    """The FL process's per-client L2 bound, ``server_config["diff_clip_norm"]``: a finite number
    > 0, or None when the key is absent or None (clipping off).  Anything else -- another type
    (bools included), NaN, an infinity, 0, a negative value -- raises ``AggregationError``: a
    mistyped bound must not quietly mean "no clipping"."""
    c = server_config.get(CLIP_KEY, None)
    if c is None:
        return None
    if isinstance(c, bool) or not isinstance(c, (int, float, np.integer, np.floating)):
        raise AggregationError(f"{CLIP_KEY} must be a finite number > 0, not {c!r}")
    c = float(c)
    with np.errstate(over="ignore", under="ignore"):
        c32 = np.float32(c)  # the engine takes the bound as a float32
    if not np.isfinite(c) or c <= 0 or not np.isfinite(c32) or c32 <= 0:
        raise AggregationError(f"{CLIP_KEY} must be a finite float32 > 0, not {c!r}")
    return c


TRIM_KEY = "diff_trim_count"  # optional server_config key: values dropped per side and parameter (no reference counterpart)


def trim_count_of(server_config: dict) -> Optional[int]:
    """The FL process's trim count, ``server_config["diff_trim_count"]``: an int in 1 .. 8, or None
    when the key is absent or None (no trimming).  Anything else -- a bool, a float with a fraction,
    0, a negative value, more than 8, another type -- raises ``AggregationError``: a mistyped count
    must not quietly mean "no trimming"."""
    b = server_config.get(TRIM_KEY, None)
    if b is None:
        return None
    if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)):
        raise AggregationError(f"{TRIM_KEY} must be an integer in 1..{TRIM_MAX}, not {b!r}")
    if isinstance(b, (float, np.floating)) and not (np.isfinite(b) and float(b) == int(b)):
        raise AggregationError(f"{TRIM_KEY} must be an integer in 1..{TRIM_MAX}, not {b!r}")
    if not 1 <= int(b) <= TRIM_MAX:
        raise AggregationError(f"{TRIM_KEY} must be an integer in 1..{TRIM_MAX}, not {b!r}")
    return int(b)


def check_trim_count(trim_count: int, n_diffs: int):
    """A trimmed close needs at least ``2 b + 1`` diffs (one value must be left per parameter)."""
    if n_diffs < 2 * trim_count + 1:
        raise TrimUnavailableError(f"{TRIM_KEY} = {trim_count} needs at least {2 * trim_count + 1} diffs, the cycle "
                                   f"has {n_diffs}")


MEDIAN_KEY = "diff_median"  # optional server_config key: True = the coordinate-wise median (no reference counterpart)


def median_of(server_config: dict) -> bool:
    """Whether the FL process asks for the coordinate-wise median, ``server_config["diff_median"]``:
    ``True`` turns it on; absent, ``None`` or ``False`` leaves it off.  Anything else -- an int, a
    string, a float -- raises ``AggregationError``: a mistyped switch must not quietly mean "the
    plain mean"."""
    m = server_config.get(MEDIAN_KEY, None)
    if m is None:
        return False
    if isinstance(m, (bool, np.bool_)):
        return bool(m)
    raise AggregationError(f"{MEDIAN_KEY} must be True or False, not {m!r}")


GEOMED_KEY = "diff_geometric_median"  # optional server_config key: the geometric median, RFA (no reference counterpart)
GEOMED_DEFAULTS = (3, 1e-6)  # (iterations, smoothing): the RFA paper's
_GEOMED_FIELDS = ("iterations", "smoothing")


def geomed_of(server_config: dict) -> Optional[tuple]:
    """The FL process's geometric-median setting, ``server_config["diff_geometric_median"]``, as
    ``(iterations, smoothing)``: ``True`` gives the defaults (3, 1e-6); a dict may set ``"iterations"``
    (an int in 1 .. 16) and ``"smoothing"`` (a finite float32 > 0), either optional.  Absent, ``None`` or
    ``False``: None (off).  Anything else -- another type, an unknown dict key, a bool where a number
    belongs, a float with a fraction for the iterations, a value out of range -- raises
    ``AggregationError``: a mistyped setting must not quietly mean "the plain mean"."""
    g = server_config.get(GEOMED_KEY, None)
    if g is None or (isinstance(g, (bool, np.bool_)) and not g):
        return None
    if isinstance(g, (bool, np.bool_)):
        return GEOMED_DEFAULTS
    if not isinstance(g, dict):
        raise AggregationError(f"{GEOMED_KEY} must be True, False or a dict of {_GEOMED_FIELDS}, not {g!r}")
    unknown = [k for k in g if k not in _GEOMED_FIELDS]
    if unknown:
        raise AggregationError(f"{GEOMED_KEY} has unknown keys {unknown!r} (known: {_GEOMED_FIELDS})")
    it, nu = g.get("iterations", GEOMED_DEFAULTS[0]), g.get("smoothing", GEOMED_DEFAULTS[1])
    bad_it = AggregationError(f"{GEOMED_KEY}['iterations'] must be an integer in 1..{GEOMED_MAX_ITERS}, not {it!r}")
    if isinstance(it, (bool, np.bool_)) or not isinstance(it, (int, float, np.integer, np.floating)):
        raise bad_it
    if isinstance(it, (float, np.floating)) and not (np.isfinite(it) and float(it) == int(it)):
        raise bad_it
    if not 1 <= int(it) <= GEOMED_MAX_ITERS:
        raise bad_it
    if isinstance(nu, (bool, np.bool_)) or not isinstance(nu, (int, float, np.integer, np.floating)):
        raise AggregationError(f"{GEOMED_KEY}['smoothing'] must be a finite float32 > 0, not {nu!r}")
    nu = float(nu)
    with np.errstate(over="ignore", under="ignore"):
        nu32 = np.float32(nu)  # the engine takes the smoothing as a float32
    if not np.isfinite(nu) or nu <= 0 or not np.isfinite(nu32) or nu32 <= 0:
        raise AggregationError(f"{GEOMED_KEY}['smoothing'] must be a finite float32 > 0, not {nu!r}")
    return (int(it), nu)


@dataclasses.dataclass(frozen=True)
class Rule:
    """One kind of robust aggregation (a row of ``KINDS``) or, with ``value``, a cycle's active rule."""
    key: str      # the server_config key
    arg: str      # the keyword that carries the value (select_mode, IncrementalCycle, which keeps it as an attribute)
    mode: int     # the engine mode the rule turns MEAN into
    error: type   # raised wherever the engine cannot apply the rule to a cycle
    lacks: str    # what the node's own averaging, the fall-back a rule forbids, lacks
    # the Engine method that takes the value -- a tuple: its arguments -- (None: the mode alone carries the rule)
    setter: Optional[str] = None
    off: object = None            # what that method takes for "no rule"
    value: object = None          # the parsed setting

    def refuse(self, why: str) -> AggregationError:
        """The rule's error, to raise: ``<key> <why>``."""
        return self.error(f"{self.key} {why}")


# in order of precedence: of two rules set together the earlier one refuses the combination
KINDS = (
    Rule(GEOMED_KEY, "geometric_median", GEOMETRIC_MEDIAN, GeometricMedianUnavailableError, "takes no geometric median",
         "set_geomed", (0, GEOMED_DEFAULTS[1])),
    Rule(MEDIAN_KEY, "median", MEDIAN, MedianUnavailableError, "takes no median"),
    Rule(TRIM_KEY, "trim_count", TRIMMED_MEAN, TrimUnavailableError, "does not trim", "set_trim", 0),
    Rule(CLIP_KEY, "clip_norm", CLIPPED_MEAN, ClipUnavailableError, "does not clip", "set_clip_norm", 0.0),
)

UNSET = object()  # an argument left out: the setting comes from server_config


def rule_of(server_config: dict, clip_norm=UNSET, trim_count=UNSET, median=UNSET, geometric_median=UNSET) -> Optional[Rule]:
    """The cycle's rule, or None.  An argument that is given overrides its ``server_config`` key
    (``None``: off).  Every setting is parsed, so a malformed one raises ``AggregationError`` even
    beside a rule that would win; two valid ones raise the error of the rule earlier in ``KINDS``."""
    if isinstance(geometric_median, tuple):  # the parsed form (a Rule's value) back as the setting
        geometric_median = dict(zip(_GEOMED_FIELDS, geometric_median))
    given = {CLIP_KEY: clip_norm, TRIM_KEY: trim_count, MEDIAN_KEY: median, GEOMED_KEY: geometric_median}
    cfg = {k: server_config.get(k, None) if v is UNSET else v for k, v in given.items()}
    values = {CLIP_KEY: clip_norm_of(cfg), TRIM_KEY: trim_count_of(cfg), MEDIAN_KEY: median_of(cfg) or None,
              GEOMED_KEY: geomed_of(cfg)}
    active = [dataclasses.replace(k, value=values[k.key]) for k in KINDS if values[k.key] is not None]
    if len(active) > 1:
        raise active[0].refuse(f"cannot be combined with {active[1].key}")
    return active[0] if active else None


@contextlib.contextmanager
def failing_closed(rule: Optional[Rule], what: str = "the engine does not average this cycle"):
    """Under a rule, a ``PlanNotAcceleratedError`` (``ModelNotAcceleratedError`` included) raised in
    the block becomes the rule's error: the caller must not fall back to the node's own averaging,
    which does not apply the rule.  Without a rule it passes through."""
    try:
        yield
    except PlanNotAcceleratedError as e:
        if rule is None:
            raise
        raise rule.refuse(f"is set but {what} ({e}); the node's own averaging {rule.lacks}") from e


def set_on_engine(engine, rule: Optional[Rule]):
    """Before a cycle's first ingest: the rule's value set, every other setting cleared -- an engine
    shared across FL processes never carries one over.  An engine without a setter that the cycle
    does not need is left alone; one that lacks the setter the cycle needs, or answers it with
    PGH_E_UNSUPPORTED (a multi-GPU group, a sub-range shard), fails the cycle with the rule's error."""
    def args(v):
        return v if isinstance(v, tuple) else (v,)

    for kind in reversed(KINDS):  # the bound first, then the trim count, as engines have always been called
        if kind.setter is None:
            continue
        if rule is None or rule.key != kind.key:
            if hasattr(engine, kind.setter):
                getattr(engine, kind.setter)(*args(kind.off))
            continue
        try:
            getattr(engine, kind.setter)(*args(rule.value))
        except AttributeError as e:
            raise rule.refuse(f"is set but the engine has no {kind.setter}") from e
        except AggregationError as e:
            if e.status != -6:  # PGH_E_UNSUPPORTED
                raise
            raise rule.refuse(f"is set but this engine cannot apply it: {e}") from e
