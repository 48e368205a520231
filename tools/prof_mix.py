#!/usr/bin/env python3
"""K19 (k_mix_rows, the row mix Y = W X on the matrix cores) beside K16 (k_row_gram), the yardstick: both are f64
MFMA kernels over the same resident rows.  One process, one lease.

    python tools/prof_mix.py [--rows 128 1000] [--pairs 3] [--step-timeout 240] [--out FILE]

ResNet-18 x ``rows`` resident synthetic diffs (``pgh_synth_fill``) in a slab of twice as many slots; W is the
nearest-neighbour matrix of a random distance matrix with f = rows / 4 (the kernel's time does not depend on the
values).  Per row count, after one warm-up of each arm, the two alternate ``--pairs`` times; each is timed as
``pgh_stats`` times its launches (HIP events around every launch).  Run it under ``rocprofv3 --kernel-trace --stats``
for the kernels' own times.  Every step runs under its own time limit (SIGALRM); the first failure ends the run.

One JSON line per measurement, then per row count a summary: K19's time, its rate (2 m n P flops, m = n) against
the 78.6 TFLOP/s f64 matrix peak, K16's (n^2 P flops) and the ratio of the two rates.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tools.prof_gram import F64_MATRIX_PEAK, step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[128, 1000])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", type=Path, default=None, help="also append every line to this file")
    args = ap.parse_args()

    import numpy as np

    import pygrid_amd
    from pygrid_amd import Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, T = sum(numel), args.step_timeout

    with Engine(0) as eng:
        def timed(fn):
            eng.reset_stats()
            fn()
            eng.sync()
            return eng.stats()["kernel_ms_total"]

        for n in args.rows:
            src, dst = list(range(n)), list(range(n, 2 * n))
            with step(f"setup {n}", T):
                eng.set_layout(numel)
                eng.reserve(2 * n)
                eng.synth_fill(1234, n)
                eng.sync()
            D = np.random.default_rng(n).random((n, n))
            W = Engine.nnm_weights(D + D.T, n // 4)
            k19, k16 = [], []
            for r in range(args.pairs + 1):  # pair 0 warms both arms up (allocations, the first launches)
                with step(f"n {n} pair {r}", T):
                    a, b = timed(lambda: eng.mix_rows(src, dst, W)), timed(lambda: eng.row_gram(src))
                    emit({"what": "k19_beside_k16", "rows": n, "pair": r, "k19_ms": a, "k16_ms": b})
                    if r:
                        k19.append(a), k16.append(b)
            a, b = statistics.median(k19), statistics.median(k16)
            r19, r16 = 2.0 * n * n * P / (a * 1e-3), 1.0 * n * n * P / (b * 1e-3)
            emit({"what": "summary", "P": P, "rows": n, "k19_ms": a, "k19_spread_ms": max(k19) - min(k19), "k16_ms": b,
                  "k16_spread_ms": max(k16) - min(k16), "k19_tflops": r19 / 1e12, "k19_share_of_f64_matrix_peak": r19 / F64_MATRIX_PEAK,
                  "k16_tflops": r16 / 1e12, "k19_rate_over_k16_rate": r19 / r16})


if __name__ == "__main__":
    main()
