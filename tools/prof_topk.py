#!/usr/bin/env python3
"""K18 (k_topk_hist / k_topk_pick / k_topk_apply, the top-k sparsified update behind a FINAL fold) against the
plain mean close of the parent commit, on one GPU in one command.

    python tools/prof_topk.py [--rounds 8] [--clients 1000] [--parent-tree DIR] [--blocks 2] [--fraction 0.01]

ResNet-18 x ``clients`` resident synthetic diffs.  The measurements run in child processes, one slab each,
alternating ``--blocks`` times between

* ``--parent-tree`` (a built checkout of the parent commit, which knows no top-k): the plain close, PGH_MEAN
  through ``pgh_fedavg_resident``, timed as ``pgh_stats`` times its launch (HIP events around it) -- the
  yardstick, never the code under test;
* this tree: per round, interleaved on the same slab, the plain close with the setting off (one launch) and on,
  with an error memory (eight: the fold into the delta plane, three histogram passes each with its pick, the
  apply pass; ``kernel_ms_last`` is the apply pass's own time).  K18's seven launches together are the close with
  the setting on less the plain close of the same round, both timed launch by launch.

Nothing is gated: K18's share of a close is reported.  One JSON line per round, then a
summary line with the medians, the spread and the fraction of the HBM peak (8 TB/s) that K18's accounted bytes
reach.  Without ``--parent-tree`` the summary says so.
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
HBM_PEAK_GBS = 8000.0


def child(tree: Path, topk: bool, rounds: int, clients: int, fraction: float):
    sys.path.insert(0, str(tree))
    import numpy as np

    import pygrid_amd
    from pygrid_amd import MEAN, Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, N = sum(numel), clients
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
            return st["kernel_ms_total"], st["kernel_ms_last"], st["kernel_launches"], st["kernel_bytes_total"]

        k = math.ceil(P * fraction)
        for r in range(rounds + 1):  # round 0 warms everything up
            rec = {"what": "topk" if topk else "parent_mean", "round": r, "P": P, "clients": N}
            if topk:
                eng.set_topk(0)
                rec["plain_ms"], _, n0, b0 = close()
                eng.set_topk(k, True)  # (set anew each round: the memory starts at zero, the first close clears the block)
                close()
                rec["topk_ms"], rec["apply_ms"], n1, b1 = close()
                assert (n0, n1) == (1, 8), (n0, n1)
                rec["k18_ms"], rec["k18_bytes_per_param"] = rec["topk_ms"] - rec["plain_ms"], (b1 - b0) / P
                st = eng.topk_stats()
                rec.update(k=st["k"], kept=st["kept"], threshold=st["threshold"])
            else:
                rec["mean_ms"], _, n0, _ = close()
                assert n0 == 1, n0
            print(json.dumps(rec), flush=True)


def run_child(tree: Path, topk: bool, args) -> list:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "topk" if topk else "parent", "--tree", str(tree),
           "--rounds", str(args.rounds), "--clients", str(args.clients), "--fraction", str(args.fraction)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    recs = []
    for ln in out.stdout.splitlines():
        if ln.startswith("{"):
            print(ln, flush=True)
            recs.append(json.loads(ln))
    return [r for r in recs if r.get("round", 0) > 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--fraction", type=float, default=0.01)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", choices=["parent", "topk"], default=None)
    ap.add_argument("--tree", default=str(HERE))
    args = ap.parse_args()
    if args.child:
        return child(Path(args.tree).resolve(), args.child == "topk", args.rounds, args.clients, args.fraction)

    med = statistics.median
    parent, ours = [], []
    for _ in range(args.blocks):
        if args.parent_tree:
            parent += run_child(Path(args.parent_tree).resolve(), False, args)
        ours += run_child(HERE, True, args)
    k18 = [r["k18_ms"] for r in ours]
    P, per = ours[0]["P"], ours[0]["k18_bytes_per_param"]
    summary = {"what": "summary", "clients": args.clients, "P": P, "k": ours[0]["k"], "kept": ours[0]["kept"],
               "plain_ms": med([r["plain_ms"] for r in ours]), "plain_min_ms": min(r["plain_ms"] for r in ours),
               "plain_max_ms": max(r["plain_ms"] for r in ours), "topk_ms": med([r["topk_ms"] for r in ours]),
               "k18_ms": med(k18), "k18_min_ms": min(k18), "k18_max_ms": max(k18),
               "apply_ms": med([r["apply_ms"] for r in ours]), "k18_bytes_per_param": per,
               "k18_hbm_fraction": per * P / 1e6 / med(k18) / HBM_PEAK_GBS,
               "k18_share_of_close": med(k18) / med([r["topk_ms"] for r in ours])}
    if parent:
        p = med([r["mean_ms"] for r in parent])
        summary.update(parent_mean_ms=p, parent_min_ms=min(r["mean_ms"] for r in parent),
                       parent_max_ms=max(r["mean_ms"] for r in parent), plain_over_parent=summary["plain_ms"] / p,
                       k18_over_parent=med(k18) / p)
    else:
        summary.update(parent_mean_ms=None, note="no --parent-tree: the parent's close was not measured")
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
