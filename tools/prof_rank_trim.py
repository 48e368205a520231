#!/usr/bin/env python3
"""K17 (k_rank_trim, the rank-trimmed mean on chip) against K15 (k_median_mean), K9 (k_median) and the plain mean
fold, in one process, alternating.

    python tools/prof_rank_trim.py [--rounds 6] [--clients 1000,256,64] [--time-limit 420]

ResNet-18 x ``clients`` resident synthetic diffs (one count per tier measured), the trim count b = N / 10, K15's
drop count c = N / 4 as in ``prof_median_mean.py``.  Per round, on the same slab: the PGH_MEAN fold, the PGH_MEDIAN
fold, the PGH_MEAN_AROUND_MEDIAN fold and the PGH_RANK_TRIMMED_MEAN fold, each timed as ``pgh_stats`` times a
launch (HIP events around it).  All four read the same 4 P (N + 2) bytes.  The yardstick is K15 in the same run
(DESIGN.md section 5).  The process ends itself after ``--time-limit`` seconds.  One JSON line per measurement,
then a summary line with the medians and the fraction of the HBM peak (8 TB/s) each kernel's accounted bytes reach.
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
    from pygrid_amd import MEAN, MEAN_AROUND_MEDIAN, MEDIAN, RANK_TRIMMED_MEAN, Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P = sum(numel)
    med = statistics.median
    names = {MEAN: "mean", MEDIAN: "k9", MEAN_AROUND_MEDIAN: "k15", RANK_TRIMMED_MEAN: "k17"}
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
            eng.set_rank_trim(n // 10)
            eng.synth_fill(1234, n)
            eng.ckpt_upload(np.zeros(P, np.float32))  # (every fold's output is the next one's input)
            eng.sync()
            assert eng.effective_variant(MEDIAN) == 50 and eng.effective_variant(RANK_TRIMMED_MEAN) == 70
            ms = {mode: [] for mode in names}
            for r in range(args.rounds + 1):  # round 0 warms all four up
                row = {}
                for mode in ms:
                    row[mode], nbytes = timed(eng, mode)
                    assert nbytes == 4 * P * (n + 2)  # one pass over the slab, ckpt in, out
                    if r:
                        ms[mode].append(row[mode])
                print(json.dumps({"what": "k17_vs_k15", "clients": n, "trim": n // 10, "drop": n // 4, "round": r,
                                  **{f"{names[m]}_ms": row[m] for m in ms}}), flush=True)
            gb = 4.0 * P * (n + 2) / 1e6  # GB/s = gb / ms
            k17 = ms[RANK_TRIMMED_MEAN]
            summary[f"n{n}"] = {**{f"{names[m]}_ms": med(ms[m]) for m in ms},
                                "k17_over_k15": med(k17) / med(ms[MEAN_AROUND_MEDIAN]), "k17_over_k9": med(k17) / med(ms[MEDIAN]),
                                "k15_hbm_fraction": gb / med(ms[MEAN_AROUND_MEDIAN]) / HBM_PEAK_GBS,
                                "k17_hbm_fraction": gb / med(k17) / HBM_PEAK_GBS, "k17_min_ms": min(k17), "k17_max_ms": max(k17)}
    print(json.dumps({"what": "summary", **summary}), flush=True)


if __name__ == "__main__":
    main()
