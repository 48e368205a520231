#!/usr/bin/env python3
"""K13 (k_row_pairdist, Multi-Krum's pairwise distance matrix) against the only other way to the same matrix:
one K12 launch (``row_distsq``) per row as the point.  One process, one lease.

    python tools/prof_krum.py [--rows 32 128] [--pairs 3] [--step-timeout 240]

ResNet-18 x ``rows`` resident synthetic diffs (``pgh_synth_fill``).  Per row count, after one warm-up of each
arm, the two arms alternate ``--pairs`` times; each is timed as ``pgh_stats`` times its launches (HIP events
around every launch, summed).  The K12 arm's point is a random vector: its time does not depend on the values.
Every step runs under its own time limit (SIGALRM) and the steps are chained: the first failure ends the run.

One JSON line per measurement, then per row count a summary line with the medians, the ratio, and K13's rate
against two byte counts: what its workgroups load (``kernel_bytes``: every anchor block's tile and the rows
after it, the partials out and in) and the slab once (what HBM has to deliver when the caches serve the
re-reads).
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

PAIRDIST_RA, PAIRDIST_RC = 8, 32  # pgh_kernels.h


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
    args = ap.parse_args()

    import numpy as np

    import pygrid_amd
    from pygrid_amd import Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, T = sum(numel), args.step_timeout
    med = statistics.median
    point = (np.random.default_rng(13).standard_normal(P) * 1e-7).astype(np.float32)

    with Engine(0) as eng:
        def timed(fn):
            eng.reset_stats()
            out = fn()
            eng.sync()
            st = eng.stats()
            return out, st["kernel_ms_total"], st["kernel_launches"], st["kernel_bytes_total"]

        for n in args.rows:
            slots = list(range(n))
            with step(f"setup {n}", T):
                eng.set_layout(numel)
                eng.reserve(n)
                eng.synth_fill(1234, n)
                eng.sync()

            def k13():
                return eng.row_pairdist(slots)

            def k12():
                return np.stack([eng.row_distsq(slots, point) for _ in range(n)])

            k13_ms, k12_ms, k13_bytes = [], [], 0
            for r in range(args.pairs + 1):  # pair 0 warms both arms up (allocations, the first launches)
                with step(f"n {n} pair {r}", T):
                    D, a_ms, a_n, k13_bytes = timed(k13)
                    _, b_ms, b_n, _ = timed(k12)
                    assert np.array_equal(D, D.T) and not D.diagonal().any() and np.isfinite(D).all()
                    print(json.dumps({"what": "k13_vs_k12", "rows": n, "pair": r, "k13_ms": a_ms, "k13_launches": a_n,
                                      "k12_ms": b_ms, "k12_launches": b_n, "ratio": b_ms / a_ms}), flush=True)
                    if r:
                        k13_ms.append(a_ms), k12_ms.append(b_ms)
            a, b = med(k13_ms), med(k12_ms)
            print(json.dumps({"what": "summary", "P": P, "rows": n, "ra": PAIRDIST_RA, "rc": PAIRDIST_RC, "k13_ms": a,
                              "k13_spread_ms": max(k13_ms) - min(k13_ms), "k12_ms": b,
                              "k12_spread_ms": max(k12_ms) - min(k12_ms), "k12_over_k13": b / a,
                              "k13_kernel_bytes": k13_bytes, "k13_loaded_gbs": k13_bytes / a / 1e6,
                              "k13_slab_once_gbs": 4.0 * P * n / a / 1e6, "pairs_per_ms": n * (n - 1) / 2 / a}), flush=True)


if __name__ == "__main__":
    main()
