#!/usr/bin/env python3
"""K7 (k_row_sumsq, the clipping norm pass) against the fold it precedes, in one process.

    python tools/prof_clip.py [--rounds 8] [--clients 1000] [--cycles 6]

1. ResNet-18 x ``clients`` resident synthetic diffs.  Per round, interleaved: the slab is refilled
   (which drops the cached sums), K7 runs over every row in one batch (``row_sumsq``), and the same
   slab is folded in PGH_MEAN; both are timed as ``pgh_stats`` times a launch (HIP events around it).
   K7 reads exactly the fold's diff bytes; the target is K7 <= 1.10 x the fold in the same run.
2. K7 on one 47 MB row (what a report's ingest queues behind its copy).
3. A report-time close (tools/close_phases.py's shape: 100 assigned, ~72 report in shuffled order
   ``--gap-ms`` apart, worker 0 never, the close right behind the last report) without a bound and
   with one that clips every 10th reporter: wall time of ``IncrementalCycle.close``.

One JSON line per measurement, then a summary line with the medians.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--cycles", type=int, default=6)
    ap.add_argument("--gap-ms", type=float, default=5.0)
    args = ap.parse_args()

    import numpy as np

    import pygrid_amd
    from pygrid_amd import CLIPPED_MEAN, MEAN, Engine
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.state_schema import build_state_fast
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, N = sum(numel), args.clients
    med = statistics.median
    summary = {"P": P, "clients": N}
    rng = np.random.default_rng(77)

    def timed(eng, fn):
        eng.reset_stats()
        fn()
        st = eng.stats()
        return st["kernel_ms_total"], st["kernel_bytes_total"]

    with Engine(0) as eng:
        eng.set_layout(numel)
        eng.reserve(N)
        eng.ckpt_upload(np.zeros(P, np.float32))
        k7, fold = [], []
        for r in range(args.rounds + 1):  # round 0 warms both up
            eng.synth_fill(1234, N)
            eng.sync()
            a_ms, a_b = timed(eng, lambda: eng.row_sumsq(range(N)))
            f_ms, f_b = timed(eng, lambda: (eng.fedavg_resident(MEAN), eng.sync()))
            rec = {"what": "k7_vs_fold", "round": r, "k7_ms": a_ms, "k7_gbs": a_b / a_ms / 1e6, "fold_ms": f_ms,
                   "fold_gbs": f_b / f_ms / 1e6, "ratio": a_ms / f_ms}
            print(json.dumps(rec), flush=True)
            if r:
                k7.append(a_ms), fold.append(f_ms)
        summary.update(k7_ms=med(k7), fold_ms=med(fold), k7_over_fold=med(k7) / med(fold),
                       k7_gbs=(4 * P * N + 8 * N * -(-P // 4096)) / med(k7) / 1e6,
                       k7_frac_of_8tbs=(4 * P * N + 8 * N * -(-P // 4096)) / med(k7) / 1e6 / 8000)
        # the clipped fold itself (sums cached: the weighted kernels over the scales)
        eng.set_clip_norm(1e-3)
        eng.row_sumsq(range(N))
        c_ms = [timed(eng, lambda: (eng.fedavg_resident(CLIPPED_MEAN), eng.sync()))[0] for _ in range(4)]
        summary.update(clipped_fold_ms=med(c_ms[1:]), clip_stats=eng.clip_stats())
        eng.set_clip_norm(0)

        one = []
        for r in range(12):
            eng.synth_ingest(99 + r, 5, 1)  # a new diff in slot 5: its cached sum goes
            eng.sync()
            one.append(timed(eng, lambda: eng.row_sumsq([5]))[0])
            print(json.dumps({"what": "k7_one_row", "round": r, "ms": one[-1]}), flush=True)
        summary.update(k7_one_row_us=med(one[2:]) * 1e3, k7_one_row_gbs=4 * P / med(one[2:]) / 1e6)

    ck = build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(0.05) for s in RESNET18_SHAPES])
    small = [build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(1e-3) for s in RESNET18_SHAPES])
             for _ in range(3)]
    big = build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(1e-1) for s in RESNET18_SHAPES])
    bound = 34.0  # ||small|| ~ 3.4, ||big|| ~ 342
    assigned = 100
    with Engine(0) as eng:
        for arm, clip in (("unclipped", None), ("clipped", bound), ("unclipped", None), ("clipped", bound)):
            walls = []
            ckpt = ck
            for c in range(args.cycles):
                inc = IncrementalCycle(eng, numel, slots=128, checkpoint=ckpt, clip_norm=clip)
                reporters = [w for w in range(1, assigned) if rng.random() >= 0.2]
                rng.shuffle(reporters)
                for w in range(assigned):
                    inc.assigned(w)
                for k, w in enumerate(reporters):
                    inc.reported(w, big if w % 10 == 0 else small[k % 3])
                    time.sleep(args.gap_ms / 1e3)
                t0 = time.perf_counter()
                ckpt = inc.close(ckpt)
                walls.append((time.perf_counter() - t0) * 1e3)
                print(json.dumps({"what": "report_close", "arm": arm, "cycle": c, "close_ms": walls[-1],
                                  "n": inc.last_close["n"], "clipped": inc.last_close["clipped"],
                                  "early": inc.last_close["early"]}), flush=True)
            summary.setdefault(f"close_ms_{arm}", []).append(med(walls[1:]))
    print(json.dumps({"what": "summary", **summary}), flush=True)


if __name__ == "__main__":
    main()
