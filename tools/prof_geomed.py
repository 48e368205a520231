#!/usr/bin/env python3
"""K12 (k_row_distsq, the geometric median's distance pass) against K7, and the whole GEOMETRIC_MEDIAN close,
in one process.

    python tools/prof_geomed.py [--rounds 7] [--clients 1000] [--iters 3] [--step-timeout 120]

ResNet-18 x ``clients`` resident synthetic diffs (``pgh_synth_fill``).  Every step runs under its own time
limit (SIGALRM after ``--step-timeout`` seconds) and the steps are chained: the first failure ends the run.

1. K12 against K7 over the same rows.  Per round: a fresh fill (it drops the cached sums), K7 over every row
   (``row_sumsq``), K12 over every row against a random point (``row_distsq``); each timed as ``pgh_stats``
   times its launch (HIP events around it; both launches end in the same k_row_sumsq_fold over the tile
   partials, so the pair is like for like).  Round 0 warms up; medians of the rest.  The bar (DESIGN.md
   section 5): K12 <= K7 x (1 + 1 / DISTSQ_RC) x 1.05.
2. The whole close at ``--iters``: ``fedavg_resident(GEOMETRIC_MEDIAN)`` with the norms cached (they come
   behind the ingests in production) and the weights not (the setting is toggled): wall time, the launches'
   total, and the difference -- the host steps (a D2H of N doubles and the f64 loop per inner iteration, the
   weight uploads).  Beside it the plain mean's close on the same slab and ``iters`` x the weighted fold +
   ``iters - 1`` x K12 from this run.

One JSON line per measurement, then a summary line with the medians.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import signal
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

DISTSQ_RC = 32  # pgh_kernels.h


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()

    import numpy as np

    import pygrid_amd
    from pygrid_amd import GEOMETRIC_MEDIAN, MEAN, WEIGHTED_MEAN, Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, N, T = sum(numel), args.clients, args.step_timeout
    med = statistics.median
    rng = np.random.default_rng(12)
    point = (rng.standard_normal(P) * 1e-7).astype(np.float32)
    slots = list(range(N))
    summary = {"P": P, "clients": N, "iters": args.iters, "rc": DISTSQ_RC}

    with Engine(0) as eng:
        with step("setup", T):
            eng.set_layout(numel)
            eng.reserve(N)
            eng.synth_fill(1234, N)
            eng.ckpt_upload(np.zeros(P, np.float32))
            eng.sync()

        def timed(fn):
            eng.reset_stats()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            wall = (time.perf_counter() - t0) * 1e3
            st = eng.stats()
            return wall, st["kernel_ms_total"], st["kernel_ms_last"], st["kernel_launches"]

        k7, k12 = [], []
        for r in range(args.rounds + 1):  # round 0 warms everything up
            with step(f"k7_k12 round {r}", T):
                eng.synth_fill(1234, N)  # the same rows again: the cached sums go
                eng.sync()
                _, a_ms, _, a_n = timed(lambda: eng.row_sumsq(slots))
                _, b_ms, _, b_n = timed(lambda: eng.row_distsq(slots, point))
                assert (a_n, b_n) == (1, 1), (a_n, b_n)
                print(json.dumps({"what": "k7_vs_k12", "round": r, "k7_ms": a_ms, "k12_ms": b_ms, "ratio": b_ms / a_ms}),
                      flush=True)
                if r:
                    k7.append(a_ms), k12.append(b_ms)
        bar = med(k7) * (1 + 1 / DISTSQ_RC) * 1.05
        rows_bytes = 4.0 * P * N
        summary.update(k7_ms=med(k7), k12_ms=med(k12), k12_over_k7=med(k12) / med(k7), bar_ms=bar,
                       within_bar=med(k12) <= bar, k7_gbs=rows_bytes / med(k7) / 1e6, k12_gbs=rows_bytes / med(k12) / 1e6)

        closes, means, wfolds = [], [], []
        for r in range(args.rounds + 1):
            with step(f"close round {r}", T):
                eng.set_geomed(0)
                _, m_ms, _, m_n = timed(lambda: eng.fedavg_resident(MEAN))
                eng.set_weights([1.0] * N)
                _, w_ms, _, w_n = timed(lambda: eng.fedavg_resident(WEIGHTED_MEAN))
                eng.set_geomed(args.iters, 1e-6)  # (a changed setting: the weights are computed again)
                eng.row_sumsq(slots)              # the norms are there, as behind the ingests
                wall, k_ms, last_ms, n = timed(lambda: eng.fedavg_resident(GEOMETRIC_MEDIAN))
                assert (m_n, w_n, n) == (1, 1, 2 * args.iters - 1), (m_n, w_n, n)
                st = eng.geomed_stats()
                print(json.dumps({"what": "close", "round": r, "wall_ms": wall, "kernels_ms": k_ms, "host_ms": wall - k_ms,
                                  "final_fold_ms": last_ms, "mean_ms": m_ms, "weighted_ms": w_ms, "launches": n,
                                  "excluded": st["excluded"], "max_weight": st["max_weight"]}), flush=True)
                if r:
                    closes.append((wall, k_ms, last_ms)), means.append(m_ms), wfolds.append(w_ms)
        eng.set_geomed(0)
        model = args.iters * med(wfolds) + (args.iters - 1) * med(k12)
        summary.update(close_wall_ms=med([c[0] for c in closes]), close_kernels_ms=med([c[1] for c in closes]),
                       close_host_ms=med([c[0] - c[1] for c in closes]), final_fold_ms=med([c[2] for c in closes]),
                       mean_close_ms=med(means), weighted_fold_ms=med(wfolds), folds_plus_k12_ms=model)
    print(json.dumps({"what": "summary", **summary}), flush=True)


if __name__ == "__main__":
    main()
