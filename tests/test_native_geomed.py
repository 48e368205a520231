"""CPU: the geometric median's host step (pgh_host.h / pgh_host.cpp: geomed_step, D -> beta -> w, W) in a
stand-alone program under ASan + UBSan, against the bits of tests/golden/geomed_cases.npz.  That it compiles
with plain g++ and nothing on the include path is also the proof that the step is HIP-free.
-ffp-contract=off as in the library's build: every f64 operation is rounded on its own."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import gen_geomed_golden as GG  # noqa: E402


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_geomed_step_under_asan_ubsan(tmp_path):
    G = np.load(GG.GOLDEN)
    D = G["step_D"]
    words = [str(D.size), "%x" % int(G["step_nu"].view(np.uint32)[0])]
    words += ["%x" % int(b) for b in D.view(np.uint64)]
    words += ["%x" % int(b) for b in G["step_w_bits"]]
    words += ["%x" % int(G["step_W_bits"][0]), "%x" % int(G["step_obj_bits"][0])]
    txt = tmp_path / "geomed_step.txt"
    txt.write_text("\n".join(words) + "\n")
    exe = tmp_path / "geomed_check_asan_ubsan"
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "native" / "geomed_check.cpp"),
                    str(ROOT / "pygrid_amd" / "csrc" / "pgh_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(txt)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")
