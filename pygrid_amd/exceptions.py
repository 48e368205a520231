"""Error types, mirroring the reference's ``PyGridError`` hierarchy
(``apps/node/src/app/main/core/exceptions.py:4``).

The reference's cycle-close task catches every exception and logs it
(``apps/node/src/app/main/model_centric/tasks/cycle.py:28-37``); raising a ``PyGridError``
subclass from the engine keeps that contract.
"""


class PyGridError(Exception):
    def __init__(self, message):
        super().__init__(message)


class AggregationError(PyGridError):
    """A libpygrid_hip call returned a negative status."""

    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status


class EngineUnavailableError(PyGridError):
    """The HIP library is not built or no GPU is visible.  The product path never falls back
    to a CPU implementation: it raises this instead."""


class StateParseError(AggregationError):
    """Malformed syft State protobuf bytes."""


class PlanNotAcceleratedError(PyGridError):
    """The hosted avg plan is not one the engine implements (user-defined non-iterative plan,
    or an iterative plan that does not match ``(avg * num + item) / (num + 1)``).  The caller
    keeps running the reference's own CPU path for it."""


class ClipUnavailableError(AggregationError):
    """The FL process asks for per-client L2 clipping (``server_config["diff_clip_norm"]``) and the
    engine cannot clip this cycle: a hosted iterative or unaccelerated plan, a non-float32 model, a
    multi-GPU group engine, or aggregation weights given together with the bound.  Deliberately NOT
    a ``PlanNotAcceleratedError``: the node's own averaging does not clip, so falling back to it
    would silently drop the defence the operator configured -- the close fails instead."""


class TrimUnavailableError(AggregationError):
    """The FL process asks for the coordinate-wise trimmed mean (``server_config["diff_trim_count"]``)
    and the engine cannot trim this cycle: a hosted iterative or unaccelerated plan, a non-float32
    model, aggregation weights or ``diff_clip_norm`` given together with it, or fewer than
    ``2 b + 1`` diffs at the close.  Like ``ClipUnavailableError`` it is NOT a
    ``PlanNotAcceleratedError``: the node's own averaging does not trim, so the close fails closed."""


class MedianUnavailableError(AggregationError):
    """The FL process asks for the coordinate-wise median (``server_config["diff_median"]``) and the
    engine cannot take it this cycle: a hosted iterative or unaccelerated plan, a non-float32 model,
    aggregation weights, ``diff_clip_norm`` or ``diff_trim_count`` given together with it, or more
    diffs at the close than the slab has slots.  Like ``ClipUnavailableError`` and
    ``TrimUnavailableError`` it is NOT a ``PlanNotAcceleratedError``: the node's own averaging takes
    no median, so the close fails closed."""


class GeometricMedianUnavailableError(AggregationError):
    """The FL process asks for the geometric median (``server_config["diff_geometric_median"]``) and the
    engine cannot take it this cycle: a hosted iterative or unaccelerated plan, a non-float32 model,
    aggregation weights or another rule given together with it, a multi-GPU group or a sub-range shard
    (the distances need whole rows), more diffs at the close than the slab has slots, or no finite diff
    at all.  Like the other rules' errors it is NOT a ``PlanNotAcceleratedError``: the node's own
    averaging takes no geometric median, so the close fails closed."""


class KrumUnavailableError(AggregationError):
    """The FL process asks for the Multi-Krum selection of its diffs (``server_config["diff_krum"]``) and the
    engine cannot select this cycle: it declines the cycle (an unaccelerated plan, a non-float32 model), it has
    no ``krum_select`` or answers PGH_E_UNSUPPORTED (a multi-GPU group, a sub-range shard, more than 1,024
    diffs), ``dp_noise`` is set beside it, or fewer than ``2 f + 3`` finite diffs reached the close.  Like the
    rules' errors it is NOT a ``PlanNotAcceleratedError``: the node's own averaging selects nothing, so the
    close fails closed."""


class TrustUnavailableError(AggregationError):
    """The FL process asks for trust-bootstrapped averaging (``server_config["diff_trust_root"]``) and the engine
    cannot apply it this cycle: no root provider is registered, the provider raised or returned ``None``, the
    root is unusable (another layout, a NaN, an infinity, all zeros), a rule of ``robust.KINDS``, ``dp_noise``,
    aggregation weights or the iterative plan stands beside it, the engine declines the cycle (an unaccelerated
    plan, a non-float32 model), lacks ``set_trust`` or answers PGH_E_UNSUPPORTED (a multi-GPU group, a sub-range
    shard), or no finite diff points along the root.  Like the rules' errors it is NOT a
    ``PlanNotAcceleratedError``: the node's own averaging trusts every diff, so the close fails closed."""


class ServerOptUnavailableError(AggregationError):
    """The FL process asks for a server optimizer (``server_config["server_optimizer"]``) and the
    engine cannot apply it this cycle: it declines the cycle (an unaccelerated plan, a non-float32
    model), it lacks ``set_server_opt``, or it answers PGH_E_UNSUPPORTED.  Like the robust rules'
    errors it is NOT a ``PlanNotAcceleratedError``: the node's own averaging applies no optimizer, so
    the close fails closed."""


class DpNoiseUnavailableError(AggregationError):
    """The FL process asks for Gaussian noise on its clipped close (``server_config["dp_noise"]``) and the
    engine cannot add it this cycle: no ``diff_clip_norm`` beside it, a cycle the engine declines or cannot
    clip (an unaccelerated or iterative plan, a non-float32 model, weights, a multi-GPU group), an engine
    without ``set_dp_noise``, or a close without a round.  Like the rules' errors it is NOT a
    ``PlanNotAcceleratedError``: the node's own averaging adds no noise, so the close fails closed."""


class ModelNotAcceleratedError(PlanNotAcceleratedError):
    """The checkpoint or a diff holds well-formed tensors that are not float32 (another dtype, or a
    serializer other than syft's "all").  The reference averages them with torch's type promotion;
    the engine is fp32-only, so the caller runs the reference path for this cycle, as for an
    unaccelerated plan (malformed bytes still raise ``StateParseError``)."""
