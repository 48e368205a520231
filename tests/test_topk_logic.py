"""CPU: the top-k sparsified update (``update_top_k``, kernel K18) -- the numpy restatement of its definition
(include/pgh_api.h), which tests/test_gpu_topk.py holds the kernel to bit for bit; the settings parser, the
fraction's resolution and the fail-closed mapping."""
import numpy as np
import pytest

from pygrid_amd import exceptions as X
from pygrid_amd import sparsify
from pygrid_amd.settings import CloseSettings, settings_of
from pygrid_amd.sparsify import TOPK_KEY, TopKSpec

F, U = np.float32, np.uint32


def topk(g, e, k):
    """``(s, e', tau_bits, kept)`` of the average ``g``, the committed error memory ``e`` (None: none is kept and no
    addition is made) and ``k``: every step one f32 operation, tau by ``np.partition`` on the keys."""
    g = np.ascontiguousarray(g, F)
    u = g if e is None else (g + np.asarray(e, F)).astype(F)
    key = u.view(U) & U(0x7fffffff)
    tau = np.partition(key, key.size - k)[key.size - k]
    keep = key >= tau
    return np.where(keep, u, F(0.0)), np.where(keep, F(0.0), u), int(tau), int(keep.sum())


def close(ckpt, g, e, k):
    """``(out, e', tau_bits, kept)``: ``out = ckpt - s``."""
    s, e2, tau, kept = topk(g, e, k)
    return (np.asarray(ckpt, F) - s).astype(F), e2, tau, kept


def test_restatement_on_the_header_example_and_its_edges():
    g = np.array([0.5, -3, 0.25, 3, -1], F)
    s, e2, tau, kept = topk(g, np.zeros(5, F), 2)
    assert s.tolist() == [0, -3, 0, 3, 0] and e2.tolist() == [0.5, 0, 0.25, 0, -1]
    assert tau == int(F(3).view(U)) and kept == 2
    assert topk(g, None, 1)[3] == 2  # the tie at tau is kept whole: kept >= k
    s, e2, _, kept = topk(g, None, 5)  # k = P: everything is applied, nothing remembered
    assert np.array_equal(s.view(U), g.view(U)) and not e2.any() and kept == 5
    s, _, tau, kept = topk(np.array([1, np.nan, -np.inf, 2], F), None, 1)  # a NaN ranks above every magnitude
    assert np.isnan(s[1]) and s[[0, 2, 3]].tolist() == [0, 0, 0] and kept == 1 and tau > 0x7f800000
    # the memory is added back: what round one left out wins round two
    _, e2, _, _ = topk(np.array([4, 3, 0], F), np.zeros(3, F), 1)
    assert topk(np.array([0, 0, 2.5], F), e2, 1)[0].tolist() == [0, 3, 0]


GOOD = [({"count": 1}, TopKSpec(count=1)), ({"count": np.int64(7), "error_feedback": False}, TopKSpec(7, None, False)),
        ({"fraction": 0.1}, TopKSpec(fraction=0.1)), ({"fraction": 1}, TopKSpec(fraction=1.0)),
        ({"fraction": np.float32(0.5), "error_feedback": True}, TopKSpec(fraction=0.5)), (None, None)]
BAD = [True, 3, "10", [], {}, {"count": 1, "fraction": 0.1}, {"count": 0}, {"count": -1}, {"count": 1.0},
       {"count": True}, {"count": "3"}, {"fraction": 0.0}, {"fraction": 1.5}, {"fraction": -0.1},
       {"fraction": float("nan")}, {"fraction": True}, {"fraction": "0.1"}, {"count": 1, "k": 2},
       {"count": 1, "error_feedback": 1}, {"count": 1, "error_feedback": None}]


@pytest.mark.parametrize("cfg, want", GOOD, ids=repr)
def test_parser_takes(cfg, want):
    assert sparsify.top_k_of({TOPK_KEY: cfg}) == want == sparsify.top_k_of({}, cfg)
    assert sparsify.top_k_of({}) is None and sparsify.top_k_of({TOPK_KEY: cfg}, None) is None


@pytest.mark.parametrize("cfg", BAD, ids=repr)
def test_parser_refuses(cfg):
    with pytest.raises(X.AggregationError):
        sparsify.top_k_of({TOPK_KEY: cfg})
    with pytest.raises(X.AggregationError):  # parsed even beside a setting that would speak first
        settings_of({TOPK_KEY: cfg, "diff_clip_norm": 1.0})


@pytest.mark.parametrize("spec, p, k", [(TopKSpec(fraction=0.1), 1000, 100), (TopKSpec(fraction=0.1), 1001, 101),
                                        (TopKSpec(fraction=1.0), 7, 7), (TopKSpec(fraction=1e-9), 5, 1),
                                        (TopKSpec(fraction=0.3), 10, 3), (TopKSpec(count=5), 5, 5)])
def test_fraction_resolves_from_the_decimal_as_written(spec, p, k):
    assert sparsify.resolve(spec, p) == k


def test_fail_closed_mapping():
    assert not issubclass(X.TopKUnavailableError, X.PlanNotAcceleratedError)
    with pytest.raises(X.TopKUnavailableError):
        sparsify.resolve(TopKSpec(count=6), 5)
    s = settings_of({TOPK_KEY: {"count": 3}})
    assert s == CloseSettings(top_k=TopKSpec(count=3)) and bool(s) and s.rule is None and s.rule_kwargs() == {}
    with pytest.raises(X.TopKUnavailableError):  # a declined plan must not reach the node's dense averaging
        with s.fail_closed():
            raise X.PlanNotAcceleratedError("a hosted plan")
    with pytest.raises(X.TopKUnavailableError):
        s.refusing_original(7)()
    with pytest.raises(X.TopKUnavailableError):  # the noise is calibrated to the dense clipped mean
        settings_of({TOPK_KEY: {"count": 3}, "diff_clip_norm": 1.0, "dp_noise": {"multiplier": 1.0}})
    both = settings_of({TOPK_KEY: {"count": 3}, "diff_median": True, "server_optimizer": {"kind": "fedadam"}},
                       server_opt=None)
    assert both.rule is not None and both.top_k == TopKSpec(count=3)  # a modifier: it sits beside a rule
    with pytest.raises(both.rule.error):  # ... and the rule speaks first
        with both.fail_closed():
            raise X.PlanNotAcceleratedError("a hosted plan")
