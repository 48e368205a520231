#!/usr/bin/env python3
"""K9 (k_median, the coordinate-wise median on chip) against the plain mean fold, in one process, and
K9p (k_median_pass, one pass per key bit) once.

    python tools/prof_median.py [--rounds 6] [--clients 1000,256,64,16] [--time-limit 420]

1. ResNet-18 x ``clients`` resident synthetic diffs (one count per K9 tier).  Per round, interleaved
   on the same slab: the PGH_MEAN fold and the PGH_MEDIAN fold, both timed as ``pgh_stats`` times a
   launch (HIP events around it).  Both read the same diff bytes; the expectation (DESIGN.md section
   5) is an ALU-bound K9 at a few times the mean fold.
2. The same slab at the first count in a context made with ``PGH_MEDIAN_PATH=passes``: one K9p fold
   (32 or 33 launches), after one to warm up; the expectation is about 33 mean folds.

The process ends itself after ``--time-limit`` seconds (SIGALRM's default action), whatever it is
doing.  One JSON line per measurement, then a summary line with the medians.
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--clients", default="1000,256,64,16")
    ap.add_argument("--time-limit", type=int, default=420)
    args = ap.parse_args()
    signal.alarm(args.time_limit)

    import numpy as np

    import pygrid_amd
    from pygrid_amd import MEAN, MEDIAN, Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P = sum(numel)
    counts = [int(x) for x in args.clients.split(",")]
    med = statistics.median
    summary = {"P": P}

    def timed(eng, fn):
        eng.reset_stats()
        fn()
        st = eng.stats()
        return st["kernel_ms_total"], st["kernel_launches"], st["kernel_bytes_total"]

    def fill(eng, n):
        eng.set_layout(numel)
        eng.reserve(n)
        eng.synth_fill(1234, n)
        eng.ckpt_upload(np.zeros(P, np.float32))  # (every fold's output is the next one's input)
        eng.sync()

    with Engine(0) as eng:
        for n in counts:
            fill(eng, n)
            assert eng.effective_variant(MEDIAN) == 50
            mean, k9 = [], []
            for r in range(args.rounds + 1):  # round 0 warms both up
                m_ms, _, m_bytes = timed(eng, lambda: (eng.fedavg_resident(MEAN), eng.sync()))
                k_ms, k_n, k_bytes = timed(eng, lambda: (eng.fedavg_resident(MEDIAN), eng.sync()))
                assert k_n == 1 and k_bytes == m_bytes == 4 * P * (n + 2)  # one pass over the slab, ckpt in, out
                print(json.dumps({"what": "k9_vs_mean", "clients": n, "round": r, "mean_ms": m_ms, "median_ms": k_ms,
                                  "ratio": k_ms / m_ms}), flush=True)
                if r:
                    mean.append(m_ms), k9.append(k_ms)
            bytes_ = 4.0 * P * (n + 2)
            summary[f"n{n}"] = {"mean_ms": med(mean), "mean_gbs": bytes_ / med(mean) / 1e6, "k9_ms": med(k9),
                                "k9_gbs": bytes_ / med(k9) / 1e6, "ratio": med(k9) / med(mean),
                                "k9_gkeys_per_s": P * n / med(k9) / 1e6}

    n = counts[0]
    os.environ["PGH_MEDIAN_PATH"] = "passes"
    try:
        eng = Engine(0)
    finally:
        del os.environ["PGH_MEDIAN_PATH"]
    with eng:
        fill(eng, n)
        assert eng.effective_variant(MEDIAN) == 51
        m_ms, _, _ = timed(eng, lambda: (eng.fedavg_resident(MEAN), eng.sync()))
        for r in range(2):  # the second one counts
            p_ms, p_n, p_bytes = timed(eng, lambda: (eng.fedavg_resident(MEDIAN), eng.sync()))
            print(json.dumps({"what": "k9p", "clients": n, "round": r, "mean_ms": m_ms, "k9p_ms": p_ms, "launches": p_n,
                              "bytes": p_bytes, "mean_folds": p_ms / m_ms}), flush=True)
        summary["k9p"] = {"clients": n, "ms": p_ms, "launches": p_n, "gbs": p_bytes / p_ms / 1e6,
                          "mean_folds": p_ms / m_ms}
    print(json.dumps({"what": "summary", **summary}), flush=True)


if __name__ == "__main__":
    main()
