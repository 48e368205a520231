"""Writes tests/golden/dp_cases.npz: what tests/dp_oracle.py computed when the definition of the DP noise
was written -- the sampler's normals (as u64 bits) at index 0, at an odd index and above 2^33, and one
noised clipped close (inputs, expected g' and out as u32 bits) -- so that an edit of the oracle cannot
silently move the definition.

    python tests/gen_dp_golden.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import dp_oracle as DO  # noqa: E402
import serveropt_oracle as SO  # noqa: E402

F = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden" / "dp_cases.npz"
KEY, ROUND = 0x0000567800001234, 7
SPANS = ((0, 4099), (7, 1001), ((1 << 33) + 5, 515))
CLOSE = {"p": 1027, "n": 3, "c": 1.0, "z": 1.1, "key": 0xDEADBEEF0BADF00D, "round": 0xFFFFFFFF}


def close_inputs():
    rng = np.random.default_rng(20261)
    p, n = CLOSE["p"], CLOSE["n"]
    ckpt = (rng.standard_normal(p) * 0.1).astype(F)
    diffs = [(rng.standard_normal(p) * s).astype(F) for s in (1e-3, 1e-2, 1.0)][:n]  # the last row is clipped
    return ckpt, diffs


def build() -> dict:
    out = {"key": np.uint64(KEY), "round": np.uint32(ROUND)}
    for k, (i0, n) in enumerate(SPANS):
        out[f"span_{k}"] = np.array([i0, n], np.int64)
        out[f"z_{k}"] = DO.bits64(DO.normals(KEY, ROUND, i0, n))
    ckpt, diffs = close_inputs()
    c = CLOSE
    g = SO.avg_from(lambda ck: CO.fedavg_clipped(ck, diffs, c["c"]), c["p"])
    out.update(ckpt=ckpt, diffs=np.stack(diffs),
               close=np.array([c["p"], c["n"], c["key"] >> 32, c["key"] & 0xFFFFFFFF, c["round"]], np.int64),
               cz=np.array([c["c"], c["z"]], F), sigma=np.float64(DO.sigma_of(c["z"], c["c"], c["n"])),
               g_noised=DO.bits32(DO.noised_avg(g, c["key"], c["round"], c["z"], c["c"], c["n"])),
               out=DO.bits32(DO.close(ckpt, g, c["key"], c["round"], c["z"], c["c"], c["n"])))
    return out


def main():
    GOLDEN.parent.mkdir(exist_ok=True)
    np.savez_compressed(GOLDEN, **build())
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
