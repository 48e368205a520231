"""CPU: the HIP-free host code (pgh_host.h / pgh_host.cpp: the copy pool, the non-temporal copy, the
scatter out of a landed piece) in a stand-alone program, once under TSan and once under ASan + UBSan.
That it compiles with plain g++ and nothing on the include path is also the proof that it is HIP-free."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("name,flags,large", [
    ("tsan", ["-fsanitize=thread"], 24),  # alternations that copy > 4 MiB: a few dozen under TSan
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 200),
])
def test_copy_pool_matches_memcpy(tmp_path, name, flags, large):
    exe = tmp_path / f"copy_pool_check_{name}"
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-fno-omit-frame-pointer", *flags,
                    str(ROOT / "tests" / "native" / "copy_pool_check.cpp"),
                    str(ROOT / "pygrid_amd" / "csrc" / "pgh_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(large)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")
