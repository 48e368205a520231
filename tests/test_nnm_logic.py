"""CPU: nearest-neighbour mixing -- the library's host weights against a numpy restatement, the ``diff_nnm`` setting, what
it refuses, and the three host paths over a numpy engine that mixes with ``W @ X``.  The GPU side: tests/test_gpu_mix.py."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import median_oracle as MO  # noqa: E402
from fake_engine import NumpyEngine  # noqa: E402
from pygrid_amd.cycle import CycleAggregator  # noqa: E402
from pygrid_amd.engine import Engine  # noqa: E402
from pygrid_amd.exceptions import AggregationError, NnmUnavailableError  # noqa: E402
from pygrid_amd.incremental import IncrementalCycle  # noqa: E402
from pygrid_amd.settings import settings_of  # noqa: E402
from pygrid_amd.state_schema import build_state_fast, parse_state  # noqa: E402

F = np.float32
CFG = {"diff_nnm": {"byzantine": 2}, "diff_median": True}


def weights(D, f):
    W = np.zeros_like(D)
    for i, near in enumerate(np.argsort(D, axis=1, kind="stable")[:, :len(D) - f]):  # stable: ties to the smaller j
        W[i, near] = 1.0 / (len(D) - f)
    return W


def test_host_weights_match_the_restatement():
    X = np.random.default_rng(3).standard_normal((11, 5))
    D = ((X[:, None] - X[None]) ** 2).sum(axis=2)
    D[4] = [3, 4, 7, 5, 0, 6, 1, 2, 8, 7, 9]  # seven smaller than the tie at 2 and 9: f = 3 keeps eight, the earlier row
    for f in (0, 3, 10):
        assert np.array_equal(Engine.nnm_weights(D, f), weights(D, f))
    assert (Engine.nnm_weights(D, 0) == 1.0 / 11).all() and list(Engine.nnm_weights(D, 3)[4, [2, 9]]) == [0.125, 0.0]
    for bad, f in ((D, -1), (D, 11), (np.full((2, 2), np.nan), 0)):
        with pytest.raises(AggregationError) as e:
            Engine.nnm_weights(bad, f)
        assert e.value.status == -1


@pytest.mark.parametrize("cfg", [3, {"byzantine": True}, {"byzantine": 1.5}, {"byzantine": -1}, {}, {"byzantine": 1, "keep": 2},
                                 {"byzantine": 1, "distances": "fast"}])
def test_a_malformed_setting_raises(cfg):
    with pytest.raises(AggregationError):
        settings_of({"diff_nnm": cfg})


class MixEngine(NumpyEngine):
    """Records what touches it (``calls``) and mixes in numpy: the definition's ``(float)(W @ (double)X)``."""
    nnm_weights = staticmethod(Engine.nnm_weights)

    def _rows(self, slots):
        return np.stack([self.slot[int(s)] for s in slots]).astype(np.float64)

    def row_sumsq(self, slots):
        return (self._rows(slots) ** 2).sum(axis=1)

    def row_pairdist(self, slots):
        X = self._rows(slots)
        return ((X[:, None] - X[None]) ** 2).sum(axis=2)

    def mix_rows(self, src, dst, W):
        self.slot.update(zip(dst, (np.asarray(W) @ self._rows(src)).astype(F)))
        self.calls.append(("mix", len(src), len(dst)))

    def ingest(self, k, flat):
        self.slot[k] = np.asarray(flat, F)
        self.calls.append(("ingest", k))

    def ckpt_upload(self, flat):
        self.ckpt = np.asarray(flat, F).copy()

    def _finish(self, mode, diffs):  # (the C oracle takes no median)
        self.ckpt = MO.fedavg_median(self.ckpt, diffs)


RNG = np.random.default_rng(19)
CKPT, ROWS = RNG.standard_normal(37).astype(F), RNG.standard_normal((9, 37)).astype(F)
ROWS[2] += F(30)
ROWS[5, 7] = np.nan  # excluded: 8 rows are mixed
CK_PB, PBS = build_state_fast([CKPT]), [build_state_fast([d]) for d in ROWS]


def incremental(eng, slots=18, **kw):
    inc = IncrementalCycle(eng, [37], slots=slots, checkpoint=CK_PB, median=True, **kw)
    for w, pb in enumerate(PBS):
        inc.assigned(w, key=w)
        inc.reported(w, pb)
    return inc


def test_the_three_paths_mix_then_apply_the_rule():
    fin = ROWS[np.isfinite(ROWS).all(axis=1)].astype(np.float64)
    want = MO.fedavg_median(CKPT, (weights(((fin[:, None] - fin[None]) ** 2).sum(axis=2), 2) @ fin).astype(F)).view(np.uint32)
    agg = CycleAggregator(eng := MixEngine())
    assert np.array_equal(agg.average_params(CFG, [CKPT], [[d] for d in ROWS])[0].view(np.uint32), want)
    assert ("reserve", 18) in eng.calls and ("mix", 8, 8) in eng.calls and eng.calls[-1] == ("finish", 8)
    assert np.array_equal(parse_state(agg.average_plan_diffs(CFG, CK_PB, PBS, framing="template"))[0].view(np.uint32), want)
    inc = incremental(eng, nnm={"byzantine": 2})
    assert inc._whole and not inc.early_fold
    assert np.array_equal(parse_state(inc.close(CK_PB, framing="template"))[0].view(np.uint32), want)
    assert inc.last_close["nnm"] == {"byzantine": 2, "neighbours": 6, "excluded": 1}
    inc = incremental(eng)  # without the stage: no such key
    inc.close(CK_PB, framing="template")
    assert "nnm" not in inc.last_close
    # too few free slots, too few finite diffs for f: the close fails, it never folds unmixed diffs
    for kw in (dict(slots=12, nnm={"byzantine": 2}), dict(nnm={"byzantine": 4})):
        inc = incremental(MixEngine(), **kw)
        with pytest.raises(NnmUnavailableError):
            inc.close(CK_PB, framing="template")
        assert not any(c[0] in ("mix", "fold", "finish") for c in inc.engine.calls)


@pytest.mark.parametrize("cfg, kw, engine", [
    ({"diff_krum": {"byzantine": 1}}, {}, MixEngine), ({"diff_bulyan": {"byzantine": 1}}, {}, MixEngine),
    ({"diff_trust_root": True}, {}, MixEngine), ({"diff_clip_norm": 1.0}, {}, MixEngine),
    ({"diff_clip_norm": 1.0, "dp_noise": {"multiplier": 1.0}}, {}, MixEngine), ({"diff_geometric_median": True}, {}, MixEngine),
    ({}, {"weights": [1.0] * 9}, MixEngine), ({"iterative_plan": True}, {"avg_plan": lambda avg, item, k: [(a * k + b) / (k + 1) for a, b in zip(avg, item)]}, MixEngine),
    ({}, {"avg_plan": lambda *a: None}, MixEngine), ({}, {}, type("Group", (MixEngine,), {"is_group": True})), ({}, {}, NumpyEngine),
    ({}, {}, lambda: (e := MixEngine(), vars(e).update(P=37, lo=0, hi=20))[0])])  # the last: a sub-range shard [0, 20) of 37
def test_refused_before_anything_is_ingested(cfg, kw, engine):
    cfg, eng = {"diff_nnm": {"byzantine": 2}, **cfg}, engine()
    for close in (lambda a: a.average_params(cfg, [CKPT], [[d] for d in ROWS], **kw),
                  lambda a: a.average_plan_diffs(cfg, CK_PB, PBS, **kw)):
        with pytest.raises(NnmUnavailableError):
            close(CycleAggregator(eng))
    if "avg_plan" not in kw:  # (the plan is the caller's to dispatch: node.select_mode fails it closed before the cycle exists)
        with pytest.raises(NnmUnavailableError):
            IncrementalCycle(eng, [37], slots=18, settings=settings_of(cfg),
                             **({"weights_by_worker": {0: 1.0}, "mode": 2} if "weights" in kw else {}))
    assert eng.calls == []  # the engine untouched
