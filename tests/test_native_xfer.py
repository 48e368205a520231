"""CPU: the HIP-free pieces of the transfer side (pgh_host.h: PieceCursor, the chunk arithmetic of ranged
ingest) in a stand-alone program under ASan + UBSan: the walk over concatenated host pieces against a
memcpy of the concatenation, over zero-length pieces, single bytes and pieces that end on the room's edge;
the ingest chunks tiling the shard row, and a gather chunk never crossing a chunk boundary."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_piece_cursor_and_ingest_chunks(tmp_path):
    exe = tmp_path / "xfer_check"
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "native" / "xfer_check.cpp"),
                    str(ROOT / "pygrid_amd" / "csrc" / "pgh_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")
