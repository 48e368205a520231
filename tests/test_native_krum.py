"""CPU: the Multi-Krum selection's host step (pgh_host.h / pgh_host.cpp: krum_select, D -> scores -> picked) in a
stand-alone program under ASan + UBSan, against the picks and bits of tests/golden/krum_cases.npz.  That it
compiles with plain g++ and nothing on the include path is also the proof that the step is HIP-free.
-ffp-contract=off as in the library's build: every f64 addition is rounded on its own."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import gen_krum_golden as GK  # noqa: E402


def case_words(D_bits, n, f, m, picked, score_bits):
    words = [f"{n} {f} {m}"] + ["%x" % int(b) for b in D_bits.reshape(-1)]
    words += [str(len(picked))] + [str(int(p)) for p in picked] + ["%x" % int(b) for b in score_bits]
    return words


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_krum_select_under_asan_ubsan(tmp_path):
    G = np.load(GK.GOLDEN)
    words = [str(len(GK.HOST_SHAPES) + 3)]
    for k, (n, f, m) in enumerate(GK.HOST_SHAPES):
        words += case_words(G[f"host_D_bits_{k}"], n, f, m, G[f"host_picked_{k}"], G[f"host_score_bits_{k}"])
    n = len(G["hostile_included"])
    for m, key in ((0, "hostile_picked"), (1, "hostile_picked_m1"), (3, "hostile_picked_m3")):
        pos = [list(G["hostile_included"]).index(s) for s in G[key]]  # positions among the included rows
        words += case_words(G["hostile_D_bits"], n, GK.HOSTILE_F, m, pos, G["hostile_score_bits"])
    txt = tmp_path / "krum_cases.txt"
    txt.write_text("\n".join(words) + "\n")
    exe = tmp_path / "krum_check_asan_ubsan"
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "native" / "krum_check.cpp"),
                    str(ROOT / "pygrid_amd" / "csrc" / "pgh_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(txt)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")
