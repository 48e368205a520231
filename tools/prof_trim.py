#!/usr/bin/env python3
"""K8 (k_fedavg_trim, the coordinate-wise trimmed mean) against the plain mean fold, in one process.

    python tools/prof_trim.py [--rounds 6] [--clients 1000] [--cycles 6] [--b 1,2,4,8]

1. ResNet-18 x ``clients`` resident synthetic diffs, once per column width (``PGH_TRIM_VEC`` = 4,
   then 1; a context reads it when it is made).  Per round and per b, interleaved on the same slab:
   the PGH_MEAN fold and the PGH_TRIMMED_MEAN fold, both timed as ``pgh_stats`` times a launch (HIP
   events around it).  Both read the same diff bytes; the expectation is
   K8 <= 1.10 x the mean fold for b <= 4 and an ALU-bound K8 at b = 8.
2. A smaller shard (``--small-p`` params x 3,000) in both widths: the auto choice's threshold.
3. A report-time close (tools/close_phases.py's shape: 100 assigned, ~72 report in shuffled order
   ``--gap-ms`` apart, worker 0 never, the close right behind the last report) untrimmed and with
   ``trim_count=2``: wall time of ``IncrementalCycle.close``.

One JSON line per measurement, then a summary line with the medians.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--cycles", type=int, default=6)
    ap.add_argument("--gap-ms", type=float, default=5.0)
    ap.add_argument("--b", default="1,2,4,8")
    ap.add_argument("--small-p", default="100000,300000,500000")
    args = ap.parse_args()

    import numpy as np

    import pygrid_amd
    from pygrid_amd import MEAN, TRIMMED_MEAN, Engine
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.state_schema import build_state_fast
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, N = sum(numel), args.clients
    bs = [int(x) for x in args.b.split(",")]
    med = statistics.median
    summary = {"P": P, "clients": N}
    rng = np.random.default_rng(78)

    def timed(eng, fn):
        eng.reset_stats()
        fn()
        st = eng.stats()
        return st["kernel_ms_total"]

    def sweep(layout, n, vec, tag):
        os.environ["PGH_TRIM_VEC"] = str(vec)
        try:
            eng = Engine(0)
        finally:
            del os.environ["PGH_TRIM_VEC"]
        with eng:
            eng.set_layout(layout)
            eng.reserve(n)
            eng.synth_fill(1234, n)
            eng.ckpt_upload(np.zeros(sum(layout), np.float32))  # (every fold's output is the next one's input)
            eng.sync()
            mean, trim = [], {b: [] for b in bs}
            for r in range(args.rounds + 1):  # round 0 warms both up
                for b in bs:
                    eng.set_trim(b)
                    m_ms = timed(eng, lambda: (eng.fedavg_resident(MEAN), eng.sync()))
                    t_ms = timed(eng, lambda: (eng.fedavg_resident(TRIMMED_MEAN), eng.sync()))
                    print(json.dumps({"what": tag, "vec": vec, "b": b, "round": r, "mean_ms": m_ms, "trim_ms": t_ms,
                                      "ratio": t_ms / m_ms}), flush=True)
                    if r:
                        mean.append(m_ms), trim[b].append(t_ms)
            bytes_ = 4.0 * sum(layout) * (n + 2)
            return {"mean_ms": med(mean), "mean_gbs": bytes_ / med(mean) / 1e6,
                    **{f"b{b}": {"ms": med(trim[b]), "ratio": med(trim[b]) / med(mean),
                                 "gbs": bytes_ / med(trim[b]) / 1e6} for b in bs}}

    for vec in (4, 1):
        summary[f"resnet18_vec{vec}"] = sweep(numel, N, vec, "k8_vs_mean")
    for p in [int(x) for x in args.small_p.split(",") if x]:
        for vec in (4, 1):
            summary[f"p{p}_vec{vec}"] = sweep([p], 3000, vec, f"k8_vs_mean_p{p}")

    ck = build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(0.05) for s in RESNET18_SHAPES])
    small = [build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(1e-3) for s in RESNET18_SHAPES])
             for _ in range(3)]
    big = build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(1e-1) for s in RESNET18_SHAPES])
    assigned = 100
    with Engine(0) as eng:
        for arm, trim in (("untrimmed", None), ("trimmed", 2), ("untrimmed", None), ("trimmed", 2)):
            walls = []
            ckpt = ck
            for c in range(args.cycles):
                inc = IncrementalCycle(eng, numel, slots=128, checkpoint=ckpt, trim_count=trim)
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
                                  "n": inc.last_close["n"], "early": inc.last_close["early"]}), flush=True)
            summary.setdefault(f"close_ms_{arm}", []).append(med(walls[1:]))
    print(json.dumps({"what": "summary", **summary}), flush=True)


if __name__ == "__main__":
    main()
