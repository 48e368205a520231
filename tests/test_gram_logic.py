"""CPU: the "gram" distance kind of the Multi-Krum stage -- the parsing of ``"distances"``, what ``krum.select`` hands
the engine, and pgh_gram_distances_host against the formula of include/pgh_api.h in numpy, operation by operation, as bits."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from pygrid_amd import Engine
from pygrid_amd.exceptions import AggregationError
from pygrid_amd.krum import KrumSpec, close_stats, krum_of, select
from pygrid_amd.settings import settings_of

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("cfg, want", [({"byzantine": 2}, "exact"), ({"byzantine": 2, "distances": "exact"}, "exact"),
                                       ({"byzantine": 2, "keep": 3, "distances": "gram"}, "gram")])
def test_distances_is_parsed(cfg, want):
    assert krum_of({"diff_krum": cfg}).distances == want
    bul = {k: v for k, v in cfg.items() if k != "keep"}
    assert settings_of({"diff_bulyan": bul}).select == KrumSpec(2, None, bulyan=True, distances=want)


@pytest.mark.parametrize("bad", ["Gram", "", None, 1, True, ["gram"]])
def test_a_bad_distances_value_or_type_is_refused(bad):
    for key in ("diff_krum", "diff_bulyan"):
        with pytest.raises(AggregationError, match="distances"):
            settings_of({key: {"byzantine": 1, "distances": bad}})


class ThreeArgEngine:
    krum_stats = staticmethod(lambda: {"picked": 2, "excluded": 0, "max_picked_score": 1.5})

    def krum_select(self, slots, f, m):
        self.got = (slots, f, m)
        return slots[:2]


def test_select_passes_the_kind_only_when_it_is_not_exact():
    eng = ThreeArgEngine()
    assert select(eng, KrumSpec(1, 2), [4, 5, 6, 7, 8]) == [4, 5] and eng.got == ([4, 5, 6, 7, 8], 1, 2)
    with pytest.raises(TypeError):  # the kind reaches the engine by keyword
        select(eng, KrumSpec(1, 2, distances="gram"), [4, 5, 6, 7, 8])
    assert close_stats(eng, KrumSpec(1, 2, distances="gram"))["distances"] == "gram" and "distances" not in close_stats(eng, KrumSpec(1, 2))


def test_gram_distances_host_is_the_formula_bit_for_bit():
    X = np.random.default_rng(16).standard_normal((7, 50)) * 10.0 ** np.arange(-3, 4)[:, None]
    G = X @ X.T
    s = G.diagonal().copy()
    # rows 0 and 1 coincide: s_0 + s_1 - 2 G_01 is 0 up to rounding, and made negative here
    G[0, 1] = G[1, 0] = np.nextafter(s[0], np.inf)
    s[1], s[5], G[5, 2], G[2, 5] = s[0], np.inf, np.inf, np.inf  # (and an inf - inf)
    with np.errstate(invalid="ignore"):
        d = (s[:, None] + s[None, :]) - 2.0 * G
    want = np.where(np.isnan(d), np.inf, np.where(d < 0, 0.0, d))
    np.fill_diagonal(want, 0.0)
    got = Engine.gram_distances_host(G, s)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert not np.signbit(got[0, 1]) and not got.diagonal().view(np.uint64).any()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_gram_distances_under_asan_ubsan(tmp_path):
    exe = tmp_path / "gram_check_asan_ubsan"  # gram_check.cpp and pgh_host.cpp alone, plain g++: the step is HIP-free
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(ROOT / "tests" / "native" / "gram_check.cpp"),
                    str(ROOT / "pygrid_amd" / "csrc" / "pgh_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
