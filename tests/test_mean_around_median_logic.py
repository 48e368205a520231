"""CPU: the mean around the median -- the oracle's hand pin, the parsers of ``diff_mean_around_median`` and
``diff_bulyan``, the Bulyan expansion and its refusals."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mam_oracle as MM  # noqa: E402
from pygrid_amd.exceptions import AggregationError, MeanAroundMedianUnavailableError  # noqa: E402
from pygrid_amd.krum import KrumSpec, select  # noqa: E402
from pygrid_amd.robust import MAM_KEY  # noqa: E402
from pygrid_amd.settings import BULYAN_KEY, settings_of  # noqa: E402


def test_hand_pin():
    """(1, 2, 4, 5), c = 1: m = 3, distances (2, 1, 1, 2); positions 1, 2 and 0 are kept (0 wins the tie over 3)."""
    mean, at_e, kept_at_e, _ = MM.mean_around_median(np.array([[1], [2], [4], [5]], np.float32), 1)
    assert mean.dtype == np.float32 and mean[0] == np.float32(7.0 / 3.0) and (at_e[0], kept_at_e[0]) == (2, 1)
    assert MM.fedavg([10.0], [[1], [2], [4], [5]], 1)[0] == np.float32(10.0) - np.float32(7.0 / 3.0)


@pytest.mark.parametrize("key, field", [(MAM_KEY, "drop"), (BULYAN_KEY, "byzantine")])
@pytest.mark.parametrize("value, ok", [(1, True), (3.0, True), (np.int64(2), True), (0, False), (-1, False), (True, False),
                                       (1.5, False), ("1", False), (None, False), (float("nan"), False)])
def test_parsers(key, field, value, ok):
    if not ok:
        with pytest.raises(AggregationError):
            settings_of({key: {field: value}})
        return
    s = settings_of({key: {field: value}})
    assert s.rule.key == MAM_KEY and s.rule.value == int(value) * (2 if key == BULYAN_KEY else 1)
    assert (s.bulyan, s.select) == ((int(value), KrumSpec(int(value), None, True)) if key == BULYAN_KEY else (None, None))


@pytest.mark.parametrize("key, field", [(MAM_KEY, "drop"), (BULYAN_KEY, "byzantine")])
@pytest.mark.parametrize("cfg", [True, 1, "x", [1], {}, {"count": 1}, "extra"])
def test_parsers_refuse_other_shapes(key, field, cfg):
    with pytest.raises(AggregationError):
        settings_of({key: {field: 1, "extra": 1} if cfg == "extra" else cfg})
    assert not settings_of({key: None}) and not settings_of({key: False})


@pytest.mark.parametrize("other", [{"diff_krum": {"byzantine": 1}}, {"diff_median": True}, {"diff_trim_count": 1},
                                   {MAM_KEY: {"drop": 2}}, {"diff_clip_norm": 1.0, "dp_noise": {"multiplier": 1.0}},
                                   {"diff_trust_root": True}])
def test_bulyan_stands_alone(other):
    with pytest.raises(MeanAroundMedianUnavailableError):
        settings_of({BULYAN_KEY: {"byzantine": 1}, **other})


def test_bulyan_stage_one_keeps_n_minus_2f_of_at_least_4f_plus_3():
    class Eng:
        def krum_select(self, slots, f, keep):
            return slots[:keep]

    spec = settings_of({BULYAN_KEY: {"byzantine": 2}}).select
    assert select(Eng(), spec, list(range(11))) == list(range(7))
    with pytest.raises(MeanAroundMedianUnavailableError):
        select(Eng(), spec, list(range(10)))
