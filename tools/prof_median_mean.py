#!/usr/bin/env python3
"""K15 (k_median_mean, the mean around the median on chip) against K9 (k_median) and the plain mean fold, in one
process, alternating.

    python tools/prof_median_mean.py [--rounds 6] [--clients 1000,256,64] [--time-limit 420]

ResNet-18 x ``clients`` resident synthetic diffs (one count per multi-wave tier and the widest one-wave tier),
the drop count c = N / 4.  Per round, on the same slab: the PGH_MEAN fold, the PGH_MEDIAN fold and the
PGH_MEAN_AROUND_MEDIAN fold, each timed as ``pgh_stats`` times a launch (HIP events around it).  All three read
the same 4 P (N + 2) bytes.  The expectation is an ALU-bound K15 at two to four times K9.
The process ends itself after ``--time-limit`` seconds.  One JSON line per measurement, then a summary line
with the medians and the fraction of the HBM peak (8 TB/s) each kernel's accounted bytes reach.
"""
from __future__ import annotations

import argparse
import json
import signal
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--clients", default="1000,256,64")
    ap.add_argument("--time-limit", type=int, default=420)
    args = ap.parse_args()
    signal.alarm(args.time_limit)

    import numpy as np

    import pygrid_amd
    from pygrid_amd import MEAN, MEAN_AROUND_MEDIAN, MEDIAN, Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P = sum(numel)
    med = statistics.median
    summary = {"P": P}

    def timed(eng, mode):
        eng.reset_stats()
        eng.fedavg_resident(mode)
        eng.sync()
        st = eng.stats()
        assert st["kernel_launches"] == 1
        return st["kernel_ms_total"], st["kernel_bytes_total"]

    with Engine(0) as eng:
        for n in (int(x) for x in args.clients.split(",")):
            eng.set_layout(numel)
            eng.reserve(n)
            eng.set_median_drop(n // 4)
            eng.synth_fill(1234, n)
            eng.ckpt_upload(np.zeros(P, np.float32))  # (every fold's output is the next one's input)
            eng.sync()
            assert eng.effective_variant(MEDIAN) == 50 and eng.effective_variant(MEAN_AROUND_MEDIAN) == 60
            ms = {MEAN: [], MEDIAN: [], MEAN_AROUND_MEDIAN: []}
            for r in range(args.rounds + 1):  # round 0 warms all three up
                row = {}
                for mode in ms:
                    row[mode], nbytes = timed(eng, mode)
                    assert nbytes == 4 * P * (n + 2)  # one pass over the slab, ckpt in, out
                    if r:
                        ms[mode].append(row[mode])
                print(json.dumps({"what": "k15_vs_k9", "clients": n, "drop": n // 4, "round": r, "mean_ms": row[MEAN],
                                  "k9_ms": row[MEDIAN], "k15_ms": row[MEAN_AROUND_MEDIAN]}), flush=True)
            gb = 4.0 * P * (n + 2) / 1e6  # GB/s = gb / ms
            summary[f"n{n}"] = {"mean_ms": med(ms[MEAN]), "k9_ms": med(ms[MEDIAN]), "k15_ms": med(ms[MEAN_AROUND_MEDIAN]),
                                "k15_over_k9": med(ms[MEAN_AROUND_MEDIAN]) / med(ms[MEDIAN]),
                                "k9_hbm_fraction": gb / med(ms[MEDIAN]) / HBM_PEAK_GBS,
                                "k15_hbm_fraction": gb / med(ms[MEAN_AROUND_MEDIAN]) / HBM_PEAK_GBS,
                                "k15_min_ms": min(ms[MEAN_AROUND_MEDIAN]), "k15_max_ms": max(ms[MEAN_AROUND_MEDIAN])}
    print(json.dumps({"what": "summary", **summary}), flush=True)


if __name__ == "__main__":
    main()
