#!/usr/bin/env python3
"""K14 (k_row_dot, the trust rule's inner products with the root) against K12 and K7, and the whole TRUSTED_MEAN
close, in one process.

    python tools/prof_trust.py [--rounds 7] [--clients 1000] [--step-timeout 120]

ResNet-18 x ``clients`` resident synthetic diffs (``pgh_synth_fill``).  Every step runs under its own time
limit (SIGALRM after ``--step-timeout`` seconds) and the steps are chained: the first failure ends the run.

1. K14 against K12 (and K7) over the same rows.  Per round: a fresh fill (it drops the cached sums), K7 over
   every row (``row_sumsq``), K12 over every row against a random point (``row_distsq``), K14 over every row
   against the same point (``row_dot``); each timed as ``pgh_stats`` times its launch (HIP events around it; all
   three launches end in the same k_row_sumsq_fold over the tile partials, so they are like for like).  Round 0
   warms up; medians of the rest.  The bar: K14 <= 1.05 x K12.
2. The whole close, ``fedavg_resident(TRUSTED_MEAN)``, two ways: with the dots computed at the close (the root is
   set again: K14 over every row, the host step, one weighted fold) and with the dots cached (they come behind the
   ingests in production; ``set_weights`` makes the weights stale and leaves the dots: the host step, the weights'
   upload and one weighted fold).  Wall time, the launches' total and the difference.  Beside them the plain
   mean's close and the weighted fold on the same slab.

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
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()

    import numpy as np

    import pygrid_amd
    from pygrid_amd import MEAN, TRUSTED_MEAN, WEIGHTED_MEAN, Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, N, T = sum(numel), args.clients, args.step_timeout
    med = statistics.median
    rng = np.random.default_rng(14)
    point = (rng.standard_normal(P) * 1e-7).astype(np.float32)
    slots = list(range(N))
    summary = {"P": P, "clients": N}

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

        k7, k12, k14 = [], [], []
        for r in range(args.rounds + 1):  # round 0 warms everything up
            with step(f"k7_k12_k14 round {r}", T):
                eng.synth_fill(1234, N)  # the same rows again: the cached sums go
                eng.sync()
                _, a_ms, _, a_n = timed(lambda: eng.row_sumsq(slots))
                _, b_ms, _, b_n = timed(lambda: eng.row_distsq(slots, point))
                _, c_ms, _, c_n = timed(lambda: eng.row_dot(slots, point))
                assert (a_n, b_n, c_n) == (1, 1, 1), (a_n, b_n, c_n)
                print(json.dumps({"what": "k7_k12_k14", "round": r, "k7_ms": a_ms, "k12_ms": b_ms, "k14_ms": c_ms,
                                  "k14_over_k12": c_ms / b_ms}), flush=True)
                if r:
                    k7.append(a_ms), k12.append(b_ms), k14.append(c_ms)
        bar = med(k12) * 1.05
        rows_bytes = 4.0 * P * N
        summary.update(k7_ms=med(k7), k12_ms=med(k12), k14_ms=med(k14), k14_over_k12=med(k14) / med(k12),
                       k14_over_k7=med(k14) / med(k7), bar_ms=bar, within_bar=med(k14) <= bar,
                       k12_gbs=rows_bytes / med(k12) / 1e6, k14_gbs=rows_bytes / med(k14) / 1e6)

        cached, at_close, means, wfolds = [], [], [], []
        for r in range(args.rounds + 1):
            with step(f"close round {r}", T):
                eng.set_trust(False)
                _, m_ms, _, m_n = timed(lambda: eng.fedavg_resident(MEAN))
                eng.set_weights([1.0] * N)
                _, w_ms, _, w_n = timed(lambda: eng.fedavg_resident(WEIGHTED_MEAN))
                eng.set_trust(True)
                eng.row_sumsq(slots)    # the norms are there, as behind the ingests
                eng.trust_root(point)   # a new root: no dot is cached
                wall_b, k_b, _, n_b = timed(lambda: eng.fedavg_resident(TRUSTED_MEAN))
                eng.set_weights([1.0] * N)  # the weights are stale, the dots are not: as behind the ingests
                wall_a, k_a, _, n_a = timed(lambda: eng.fedavg_resident(TRUSTED_MEAN))
                assert (m_n, w_n, n_a, n_b) == (1, 1, 1, 2), (m_n, w_n, n_a, n_b)
                st = eng.trust_stats()
                print(json.dumps({"what": "close", "round": r, "cached_wall_ms": wall_a, "cached_kernels_ms": k_a,
                                  "cached_host_ms": wall_a - k_a, "at_close_wall_ms": wall_b, "at_close_kernels_ms": k_b,
                                  "at_close_host_ms": wall_b - k_b, "mean_ms": m_ms, "weighted_ms": w_ms,
                                  "trusted": st["trusted"], "excluded": st["excluded"], "max_weight": st["max_weight"]}),
                      flush=True)
                if r:
                    cached.append((wall_a, k_a)), at_close.append((wall_b, k_b)), means.append(m_ms), wfolds.append(w_ms)
        eng.set_trust(False)
        summary.update(close_cached_wall_ms=med([c[0] for c in cached]), close_cached_kernels_ms=med([c[1] for c in cached]),
                       close_cached_host_ms=med([c[0] - c[1] for c in cached]),
                       close_at_close_wall_ms=med([c[0] for c in at_close]), close_at_close_kernels_ms=med([c[1] for c in at_close]),
                       close_at_close_host_ms=med([c[0] - c[1] for c in at_close]),
                       mean_close_ms=med(means), weighted_fold_ms=med(wfolds), k14_plus_fold_ms=med(k14) + med(wfolds))
    print(json.dumps({"what": "summary", **summary}), flush=True)


if __name__ == "__main__":
    main()
