"""CPU: the HIP-free restatement of the DP noise sampler (pgh_host.h / pgh_host.cpp: Philox4x32-10, plog,
the polar method, the windows of dp_normals) in a stand-alone program under ASan + UBSan.  That it compiles
with plain g++ and nothing on the include path is also the proof that it is HIP-free.  -ffp-contract=off
as in the library's build: every f64 operation of the sampler is rounded on its own."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_dp_sampler_under_asan_ubsan(tmp_path):
    exe = tmp_path / "dp_check_asan_ubsan"
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "native" / "dp_check.cpp"),
                    str(ROOT / "pygrid_amd" / "csrc" / "pgh_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")
