"""CPU: the trust rule's host code (pgh_host.h / pgh_host.cpp: trust_weights, sums and dots -> included rows and
weights; row_dot_host, K7's order on the host, where the root's s0 comes from) in a stand-alone program under
ASan + UBSan, against tests/golden/trust_cases.npz and tests/trust_oracle.py.  That it compiles with plain g++ and
nothing on the include path is also the proof that the code is HIP-free.  -ffp-contract=off as in the library's
build: every f64 operation is rounded on its own."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import clip_oracle as CO  # noqa: E402
import gen_trust_golden as GT  # noqa: E402
import trust_oracle as TO  # noqa: E402

F = np.float32


def b64(x):
    return ["%x" % int(b) for b in np.ascontiguousarray(x, np.float64).reshape(-1).view(np.uint64)]


def b32(x):
    return ["%x" % int(b) for b in np.ascontiguousarray(x, F).reshape(-1).view(np.uint32)]


def weight_case(s0, ss, dt):
    ss, dt = np.asarray(ss, np.float64), np.asarray(dt, np.float64)
    words = b64([s0]) + [str(len(ss))] + [w for pair in zip(b64(ss), b64(dt)) for w in pair]
    inc = [k for k, s in enumerate(ss) if np.isfinite(s)]
    try:
        o = TO.trust_weights(s0, ss, dt)
        return words + ["0", str(len(inc))] + [str(k) for k in o["included"]] + b32(o["weights"]) + b64([o["T"]])
    except TO.BadRoot:
        return words + ["-1", "0"] + b64([0.0])
    except TO.NoTrustedRow:  # no row included (-2), or T == 0 (-3): the positions are written, no weight is
        rc = "-2" if not inc else "-3"
        return words + [rc, str(len(inc))] + [str(k) for k in inc] + ["0"] * len(inc) + b64([0.0])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_trust_host_code_under_asan_ubsan(tmp_path):
    G = np.load(GT.GOLDEN)
    cases = [weight_case(float(G["w_s0"][0]), G["w_sumsq"], G["w_dot"]),
             weight_case(G["fold_s0_bits"].view(np.float64)[0], G["fold_sumsq_bits"].view(np.float64), G["fold_dot_bits"].view(np.float64))]
    assert cases[0][-1 - 6:-1] == ["%x" % int(b) for b in G["w_bits"]] and cases[1][-1] == "%x" % int(G["fold_T_bits"][0])
    t = TO.trust(G["hostile_diffs"], G["hostile_root"])
    cases.append(weight_case(t["s0"], t["sumsq"], t["dot"]))
    cases += [weight_case(1.0, [], []), weight_case(1.0, [np.nan, np.inf], [0.0, 0.0]), weight_case(1.0, [1.0, 4.0, 0.0], [-0.5, 0.0, 0.0]),
              weight_case(0.0, [1.0], [1.0]), weight_case(np.nan, [1.0], [1.0]), weight_case(np.inf, [1.0], [1.0]),
              weight_case(2.0, [1e-90], [1e-45])]
    words = [str(len(cases))] + [w for c in cases for w in c]
    rng = np.random.default_rng(14)
    dots = []
    for p in (1, 3, 4095, 4096, 4097, 2 * 4096 + 2048 + 3):
        x = (rng.standard_normal(p) * 10.0 ** rng.integers(-3, 4, p)).astype(F)
        y = rng.standard_normal(p).astype(F)
        dots.append([str(p)] + b32(x) + b32(y) + b64([TO.row_dot(x, y)]))
        dots.append([str(p)] + b32(x) + b32(x) + b64([CO.row_sumsq(x)]))  # a row against itself: K7's sum
    dots.append([str(GT.FOLD_P)] + b32(G["fold_root"]) * 2 + ["%x" % int(G["fold_s0_bits"][0])])
    words += [str(len(dots))] + [w for d in dots for w in d]
    txt = tmp_path / "trust_cases.txt"
    txt.write_text("\n".join(words) + "\n")
    exe = tmp_path / "trust_check_asan_ubsan"
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "native" / "trust_check.cpp"),
                    str(ROOT / "pygrid_amd" / "csrc" / "pgh_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(txt)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")
