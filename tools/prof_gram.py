#!/usr/bin/env python3
"""K16 (k_row_gram, the Gram matrix on the matrix cores) against K13 (k_row_pairdist), the two ways to the
Multi-Krum stage's distance matrix.  One process, one lease.

    python tools/prof_gram.py [--rows 32 128] [--pairs 3] [--step-timeout 240] [--out FILE]

ResNet-18 x ``rows`` resident synthetic diffs (``pgh_synth_fill``).  Per row count, after one warm-up of each
arm, the two arms alternate ``--pairs`` times; each is timed as ``pgh_stats`` times its launches (HIP events
around every launch, summed): K16's main kernel and its fold, K13's main kernel and its fold.  The host steps
(``gram_distances_host``) and the copies are not in either figure.  Every step runs under its own time limit
(SIGALRM) and the steps are chained: the first failure ends the run.

One JSON line per measurement, then per row count a summary line with the medians, the spreads, the ratio,
whether K16 was faster in every pair, and K16's rate: n^2 P flops (the triangle and the diagonal, two flops a
product) against the 78.6 TFLOP/s f64 matrix peak.  The largest relative difference between the two distance
matrices is printed beside them: reordered sums, last bits only.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import signal
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

F64_MATRIX_PEAK = 78.6e12


class StepTimeout(RuntimeError):
    pass


@contextlib.contextmanager
def step(name: str, seconds: int):
    def fire(*_a):
        raise StepTimeout(f"step {name!r} ran past its {seconds} s limit")

    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[32, 128])
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
    med = statistics.median

    with Engine(0) as eng:
        def timed(fn):
            eng.reset_stats()
            out = fn()
            eng.sync()
            st = eng.stats()
            return out, st["kernel_ms_total"], st["kernel_launches"]

        for n in args.rows:
            slots = list(range(n))
            with step(f"setup {n}", T):
                eng.set_layout(numel)
                eng.reserve(n)
                eng.synth_fill(1234, n)
                s = eng.row_sumsq(slots)
                eng.sync()
            k16_ms, k13_ms = [], []
            for r in range(args.pairs + 1):  # pair 0 warms both arms up (allocations, the first launches)
                with step(f"n {n} pair {r}", T):
                    G, a_ms, a_n = timed(lambda: eng.row_gram(slots))
                    D, b_ms, b_n = timed(lambda: eng.row_pairdist(slots))
                    Dg = Engine.gram_distances_host(G, s)
                    off = ~np.eye(n, dtype=bool)
                    rel = float(np.max(np.abs(Dg - D)[off] / D[off])) if n > 1 else 0.0
                    assert np.array_equal(G, G.T) and np.isfinite(G).all()
                    emit({"what": "k16_vs_k13", "rows": n, "pair": r, "k16_ms": a_ms, "k16_launches": a_n, "k13_ms": b_ms,
                          "k13_launches": b_n, "k13_over_k16": b_ms / a_ms, "max_rel_diff_of_distances": rel})
                    if r:
                        k16_ms.append(a_ms), k13_ms.append(b_ms)
            a, b = med(k16_ms), med(k13_ms)
            emit({"what": "summary", "P": P, "rows": n, "k16_ms": a, "k16_spread_ms": max(k16_ms) - min(k16_ms), "k13_ms": b,
                  "k13_spread_ms": max(k13_ms) - min(k13_ms), "k13_over_k16": b / a,
                  "k16_faster_in_every_pair": all(x < y for x, y in zip(k16_ms, k13_ms)),
                  "k16_tflops": float(n) * n * P / a / 1e9, "k16_share_of_f64_matrix_peak": float(n) * n * P / (a * 1e-3) / F64_MATRIX_PEAK,
                  "k13_pairs_per_ms": n * (n - 1) / 2 / b, "k16_pairs_per_ms": n * (n - 1) / 2 / a})


if __name__ == "__main__":
    main()
