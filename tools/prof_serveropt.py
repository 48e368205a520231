#!/usr/bin/env python3
"""K10 (k_server_opt, the server optimizer's step behind a FINAL fold) against the plain close, in one process.

    python tools/prof_serveropt.py [--rounds 6] [--clients 1000] [--cycles 6] [--kinds fedadam,fedavgm]

1. ResNet-18 x ``clients`` resident synthetic diffs.  Per round, interleaved on the same slab: the plain
   PGH_MEAN close and the same close under each optimizer, timed as ``pgh_stats`` times the launches
   (HIP events around each).  With an optimizer the close is two launches, the fold and K10:
   ``kernel_ms_last`` is K10's own time and the rest of ``kernel_ms_total`` the fold's.  K10 moves
   28 bytes per param (20 for FedAvgM) against the fold's 4 (N + 2): the expectation (DESIGN.md
   section 5) is a close about 0.7 % longer at N = 1,000, and the bar is K10's time <= its accounted
   bytes over HALF the HBM rate the mean fold reaches in the same run.
2. A report-time close (tools/close_phases.py's shape: 100 assigned, ~72 report in shuffled order
   ``--gap-ms`` apart, worker 0 never, the close right behind the last report) plain and with FedAdam:
   wall time of ``IncrementalCycle.close``; K10 adds a launch per 4 MiB range there.  The arms run as
   blocks of ``--cycles`` closes (plain, fedadam, plain, fedadam), not interleaved cycle by cycle.

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
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--cycles", type=int, default=6)
    ap.add_argument("--gap-ms", type=float, default=5.0)
    ap.add_argument("--kinds", default="fedadam,fedavgm")
    args = ap.parse_args()

    import numpy as np

    import pygrid_amd
    from pygrid_amd import MEAN, Engine
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.serveropt import ServerOptStates, server_opt_of
    from pygrid_amd.state_schema import build_state_fast
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, N = sum(numel), args.clients
    specs = {k: server_opt_of({"server_optimizer": {"name": k, "lr": 0.1}}) for k in args.kinds.split(",") if k}
    med = statistics.median
    summary = {"P": P, "clients": N}
    rng = np.random.default_rng(78)

    with Engine(0) as eng:
        eng.set_layout(numel)
        eng.reserve(N)
        eng.synth_fill(1234, N)
        eng.ckpt_upload(np.zeros(P, np.float32))  # (every close's output is the next one's input)
        eng.sync()

        def close():
            eng.reset_stats()
            eng.fedavg_resident(MEAN)
            eng.sync()
            st = eng.stats()
            return st["kernel_ms_total"], st["kernel_ms_last"], st["kernel_launches"]

        plain, opt = [], {k: [] for k in specs}
        for r in range(args.rounds + 1):  # round 0 warms everything up
            for k, spec in specs.items():
                eng.set_server_opt(0)
                p_ms, _, p_n = close()
                eng.set_server_opt(*spec.args())
                t_ms, k10_ms, o_n = close()
                eng.server_opt_commit()
                assert (p_n, o_n) == (1, 2), (p_n, o_n)
                print(json.dumps({"what": "close_vs_plain", "kind": k, "round": r, "plain_ms": p_ms, "opt_ms": t_ms,
                                  "fold_ms": t_ms - k10_ms, "k10_ms": k10_ms, "ratio": t_ms / p_ms}), flush=True)
                if r:
                    plain.append(p_ms), opt[k].append((t_ms, k10_ms))
        eng.set_server_opt(0)
        mean_ms = med(plain)
        mean_gbs = 4.0 * P * (N + 2) / mean_ms / 1e6
        summary.update(mean_ms=mean_ms, mean_gbs=mean_gbs)
        for k, spec in specs.items():
            k10 = med([x[1] for x in opt[k]])
            k10_bytes = (20.0 if k == "fedavgm" else 28.0) * P
            bar_ms = k10_bytes / (0.5 * mean_gbs * 1e6)
            summary[k] = {"close_ms": med([x[0] for x in opt[k]]), "ratio": med([x[0] for x in opt[k]]) / mean_ms,
                          "k10_ms": k10, "k10_gbs": k10_bytes / k10 / 1e6, "bar_ms": bar_ms, "within_bar": k10 <= bar_ms}

    ck = build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(0.05) for s in RESNET18_SHAPES])
    small = [build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(1e-3) for s in RESNET18_SHAPES])
             for _ in range(3)]
    big = build_state_fast([rng.standard_normal(s, dtype=np.float32) * np.float32(1e-1) for s in RESNET18_SHAPES])
    assigned = 100
    adam = server_opt_of({"server_optimizer": {"name": "fedadam", "lr": 0.1}})
    states = ServerOptStates()
    with Engine(0) as eng:
        for arm, spec in (("plain", None), ("fedadam", adam), ("plain", None), ("fedadam", adam)):
            walls = []
            ckpt = ck
            for c in range(args.cycles):
                inc = IncrementalCycle(eng, numel, slots=128, checkpoint=ckpt, server_opt=spec,
                                       opt_key="prof" if spec else None, opt_states=states)
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
