"""Everything an FL process can ask of a cycle's close in its ``server_config`` -- a robust-aggregation
rule (``robust.py``), a server optimizer (``serveropt.py``), Gaussian noise beside the clip bound
(``dp.py``), a Multi-Krum selection of the diffs ahead of the average (``krum.py``) -- parsed once, by ``settings_of`` alone, into one ``CloseSettings``, which is what the call
sites hold: its ``fail_closed`` is the one fail-closed decision, ``refusing_original`` the one stand-in for
the node's own averaging, ``set_on_engine`` the one way onto an engine, ``close_stats`` what ``last_close``
says.  Of two things set together the noise speaks before the rule, the rule before the selection, the
selection before the optimizer.

Sits below ``cycle.py`` and ``incremental.py`` (it imports only those four, ``engine`` and ``exceptions``).
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import Callable, Optional

from . import dp, krum as krum_mod, robust, trust as trust_mod
from .dp import DP_KEY, DpNoiseSpec, dp_noise_of
from .exceptions import ClipUnavailableError, DpNoiseUnavailableError, KrumUnavailableError, \
    PlanNotAcceleratedError, ServerOptUnavailableError, TrustUnavailableError
from .krum import KRUM_KEY, KrumSpec, krum_of
from .robust import CLIP_KEY, GEOMED_KEY, MEDIAN_KEY, TRIM_KEY, UNSET, Rule, rule_of
from .serveropt import OPT_KEY, ServerOptSpec, server_opt_of
from .trust import TRUST_KEY, TrustSpec, trust_of


@dataclasses.dataclass(frozen=True)
class CloseSettings:
    """A cycle's parsed settings: each in its module's own parsed form, or None."""
    rule: Optional[Rule] = None
    opt: Optional[ServerOptSpec] = None
    noise: Optional[DpNoiseSpec] = None
    select: Optional[KrumSpec] = None
    trust: Optional[TrustSpec] = None

    def __bool__(self) -> bool:
        return self.rule is not None or self.opt is not None or self.noise is not None or self.select is not None \
            or self.trust is not None

    def rule_kwargs(self) -> dict:
        """The rule as the keyword argument that ``select_mode`` takes."""
        return {} if self.rule is None else {self.rule.arg: self.rule.value}

    @contextlib.contextmanager
    def fail_closed(self, what: str = "the engine does not average this cycle"):
        """A ``PlanNotAcceleratedError`` (``ModelNotAcceleratedError`` included) raised in the block must not
        reach a caller that falls back to the node's own averaging, which clips, trims, steps and noises nothing.
        Under a rule it becomes the rule's error, under the trust rule a ``TrustUnavailableError``; under noise that error in turn, like the clip rule's own
        refusal, a ``DpNoiseUnavailableError``; under a selection without a rule a ``KrumUnavailableError``; under
        an optimizer alone a ``ServerOptUnavailableError``."""
        try:
            with krum_mod.failing_closed(self.select, what), trust_mod.failing_closed(self.trust, what), \
                    robust.failing_closed(self.rule, what):
                yield
        except (PlanNotAcceleratedError, ClipUnavailableError) as e:
            if self.noise is not None:
                raise DpNoiseUnavailableError(f"{DP_KEY} is set but the engine does not average this cycle ({e}); "
                                              "the node's own averaging adds no noise") from e
            if self.opt is not None and isinstance(e, PlanNotAcceleratedError):
                raise ServerOptUnavailableError(f"{OPT_KEY} is set but the engine does not average this cycle ({e}); "
                                                "the node's own averaging applies no optimizer") from e
            raise

    def refusing_original(self, cycle_id) -> Optional[Callable]:
        """What stands in for the node's own ``_average_plan_diffs`` where the engine does not average the
        cycle: it raises, since that averaging lacks what was asked for.  None when nothing is set."""
        if self.noise is not None:
            key, error, lacks = DP_KEY, DpNoiseUnavailableError, "adds no noise"
        elif self.rule is not None:
            key, error, lacks = self.rule.key, self.rule.error, self.rule.lacks
        elif self.trust is not None:
            key, error, lacks = TRUST_KEY, TrustUnavailableError, "trusts every diff"
        elif self.select is not None:
            key, error, lacks = KRUM_KEY, KrumUnavailableError, "selects nothing"
        elif self.opt is not None:
            key, error, lacks = OPT_KEY, ServerOptUnavailableError, "applies no optimizer"
        else:
            return None

        def original(*_a, **_k):
            raise error(f"{key} is set and the engine does not average cycle {cycle_id}; not falling back to the "
                        f"node's own averaging, which {lacks}")
        return original

    def noise_key(self, dp_keys: dp.DpKeys, process) -> Optional[int]:
        """The key this FL process's noise is drawn from (None: no noise)."""
        return None if self.noise is None else dp_keys.key_for(process, self.noise)

    def set_on_engine(self, engine, key: Optional[int] = None, round: Optional[int] = None, noise_only=False) -> None:
        """Before a cycle's first ingest: the rule, then the noise (it is scaled by the bound) drawn from ``key``
        for ``round``, each set or cleared -- an engine shared across FL processes carries none over.
        ``noise_only``: again right before a FINAL pass."""
        if not noise_only:
            robust.set_on_engine(engine, self.rule)
            trust_mod.set_on_engine(engine, self.trust)  # (the cycle's root follows: trust.set_root)
        dp.set_on_engine(engine, self.noise, key, round)

    def _value(self, key: str, off=None):
        return self.rule.value if self.rule is not None and self.rule.key == key else off

    def close_stats(self, engine) -> dict:
        """The rule's and the noise's entries of ``last_close``, read from the engine after the FINAL pass (it
        was reset when the cycle took it: the clip counters are this cycle's rows only; ``noise_std`` is z C / N)."""
        cs = engine.clip_stats() if self._value(CLIP_KEY) is not None else None
        ns = engine.dp_stats() if self.noise is not None else None
        stats = {"clipped": int(cs["clipped"]) if cs else 0, "max_norm": float(cs["max_norm"]) if cs else None,
                 "trim": self._value(TRIM_KEY), "median": self._value(MEDIAN_KEY, False),
                 "noise_multiplier": float(ns["multiplier"]) if ns else None,
                 "noise_std": float(ns["sigma"]) if ns else None}
        if self._value(GEOMED_KEY) is not None:  # one more key, under this rule alone
            gs = engine.geomed_stats()
            stats["geometric_median"] = {"iterations": int(gs["iterations"]), "excluded": int(gs["excluded"]),
                                         "objective": float(gs["objective"]), "max_weight": float(gs["max_weight"])}
        if self.select is not None:  # one more key, under a selection alone
            stats["krum"] = krum_mod.close_stats(engine, self.select)
        if self.trust is not None:  # one more key, under the trust rule alone
            stats["trust"] = trust_mod.close_stats(engine)
        return stats

    def close_message(self, cycle_id, last_close: dict) -> str:
        """One log line on a close under a rule or a selection, from its ``last_close``."""
        kr = last_close.get("krum")
        picked = "" if kr is None else "; %s picked %d of them (f = %d, %d excluded, largest picked score %s)" % (
            KRUM_KEY, kr["picked"], kr["byzantine"], kr["excluded"], kr["max_picked_score"])
        tr = last_close.get("trust")
        if tr is not None:
            return "cycle %s closed with %s over %d diffs (%d trusted, %d excluded, total trust %s, largest weight %s, root norm %s)%s" % (
                cycle_id, TRUST_KEY, last_close.get("n", 0), tr["trusted"], tr["excluded"], tr["total_trust"],
                tr["max_weight"], tr["root_norm"], picked)
        if self.rule is None:
            return "cycle %s closed over %d diffs%s" % (cycle_id, last_close.get("n", 0), picked)
        noised = "" if self.noise is None else "; %s multiplier %s, noise std %s per parameter" % (
            DP_KEY, last_close.get("noise_multiplier"), last_close.get("noise_std"))
        gm = last_close.get("geometric_median")
        if gm is not None:
            return "cycle %s closed with %s=%r over %d diffs (%d excluded, sum of distances %s, largest weight %s)%s" % (
                cycle_id, self.rule.key, self.rule.value, last_close.get("n", 0), gm["excluded"], gm["objective"],
                gm["max_weight"], picked)
        return "cycle %s closed with %s=%r over %d diffs (%d clipped, max norm %s)%s%s" % (
            cycle_id, self.rule.key, self.rule.value, last_close.get("n", 0), last_close.get("clipped", 0),
            last_close.get("max_norm"), noised, picked)


def settings_of(server_config: dict, clip_norm=UNSET, trim_count=UNSET, median=UNSET, dp_noise=UNSET,
                server_opt=UNSET, geometric_median=UNSET, krum=UNSET, trust=UNSET) -> CloseSettings:
    """The cycle's settings.  An argument that is given overrides its ``server_config`` key (``None``: off);
    ``server_opt`` and ``dp_noise`` take the setting's dict or its parsed form.  Every setting is parsed, so a
    malformed one raises ``AggregationError`` even beside one that would speak first; two rules at once raise
    the earlier rule's error (``robust.KINDS``), noise without the clip bound ``DpNoiseUnavailableError``, a
    selection (``krum``: the setting's dict or its parsed form) beside noise ``KrumUnavailableError``, the trust
    rule (``trust``) beside any rule of ``robust.KINDS`` or beside noise ``TrustUnavailableError`` (weights and the
    iterative plan are refused where the mode is chosen, ``cycle.select_mode``)."""
    rule = rule_of(server_config, clip_norm, trim_count, median, geometric_median)
    if not isinstance(server_opt, ServerOptSpec):
        server_opt = server_opt_of(server_config if server_opt is UNSET else {OPT_KEY: server_opt})
    noise = dp_noise_of(server_config, dp_noise)
    tr = trust_of(server_config, trust)
    if tr is not None and rule is not None:
        raise trust_mod.refuse(f"cannot be combined with {rule.key}: the trusted mean is the cycle's averaging rule")
    if tr is not None and noise is not None:
        raise trust_mod.refuse(f"cannot be combined with {DP_KEY}: the noise is calibrated to the clipped mean")
    dp.check_rule(noise, rule)
    select = krum_of(server_config, krum)
    if select is not None and noise is not None:
        raise krum_mod.refuse(f"cannot be combined with {DP_KEY}: the clip-and-noise sensitivity argument does not "
                              "cover a data-dependent selection of the diffs")
    return CloseSettings(rule, server_opt, noise, select, tr)
