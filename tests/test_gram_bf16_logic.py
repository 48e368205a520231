"""CPU: the "gram_bf16" distance kind -- its parsing in the three settings, what ``krum.select`` and ``nnm.mix`` hand
the engine, and ``close_stats``."""
import numpy as np
import pytest

from pygrid_amd import Engine
from pygrid_amd.krum import DISTANCES, KrumSpec, close_stats, krum_of, select
from pygrid_amd.nnm import NnmSpec, mix, nnm_of
from pygrid_amd.settings import settings_of


def test_the_kind_is_parsed_in_all_three_settings():
    assert DISTANCES == ("exact", "gram", "gram_bf16")
    cfg = {"byzantine": 2, "distances": "gram_bf16"}
    assert krum_of({"diff_krum": cfg}).distances == nnm_of({"diff_nnm": cfg}).distances == "gram_bf16"
    assert settings_of({"diff_bulyan": cfg}).select == KrumSpec(2, None, bulyan=True, distances="gram_bf16")


class Recorder:
    """Records the keywords it is handed; distances and weights in numpy."""
    P, lo, hi, is_group = 4, 0, 4, False
    krum_stats = staticmethod(lambda: {"picked": 2, "excluded": 0, "max_picked_score": 1.5})
    gram_distances_host, nnm_weights = staticmethod(Engine.gram_distances_host), staticmethod(Engine.nnm_weights)
    X = np.arange(20.0).reshape(5, 4) ** 2

    def krum_select(self, slots, f, m, **kw):
        self.got = kw
        return slots[:2]

    def row_sumsq(self, slots):
        return (self.X[slots] ** 2).sum(axis=1)

    def row_gram(self, slots, **kw):
        self.got = kw
        return self.X[slots] @ self.X[slots].T

    def mix_rows(self, src, dst, W):
        self.mixed = (src, dst)


@pytest.mark.parametrize("kind, krum_kw, gram_kw", [("gram", {"distances": "gram"}, {}), ("gram_bf16", {"distances": "gram_bf16"}, {"kind": "bf16"})])
def test_select_and_mix_hand_the_engine_the_kind(kind, krum_kw, gram_kw):
    eng = Recorder()
    assert select(eng, KrumSpec(1, 2, distances=kind), [0, 1, 2, 3, 4]) == [0, 1] and eng.got == krum_kw
    assert close_stats(eng, KrumSpec(1, 2, distances=kind))["distances"] == kind
    dst, stats = mix(eng, NnmSpec(1, kind), [0, 1, 2, 3, 4], [5, 6, 7, 8, 9])
    assert eng.got == gram_kw and eng.mixed == ([0, 1, 2, 3, 4], dst) and stats["neighbours"] == 4
