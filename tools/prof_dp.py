#!/usr/bin/env python3
"""K11 (k_dp_noise, the Gaussian noise behind a clipped FINAL fold) against the clipped close of the parent
commit, on one GPU in one command.

    python tools/prof_dp.py [--rounds 8] [--clients 1000] [--parent-tree DIR] [--blocks 2]

ResNet-18 x ``clients`` resident synthetic diffs, a bound that clips, the sums of squares cached.  The
measurements run in child processes, one slab each, alternating ``--blocks`` times between

* ``--parent-tree`` (a built checkout of the parent commit, which knows no noise): the clipped close,
  PGH_CLIPPED_MEAN through ``pgh_fedavg_resident``, timed as ``pgh_stats`` times its launch (HIP events
  around it) -- the reference the bar is set against, never the code under test;
* this tree: per round, interleaved on the same slab, the clipped close with the noise off (one launch)
  and on (two: the fold into the delta plane, then K11; ``kernel_ms_last`` is K11's own time).

The bar: K11's kernel time <= 2 % of the parent's clipped-close kernel time -- the
lease-to-lease spread of the fold itself, below which a difference cannot be told from the box.  One JSON
line per round, then a summary line with the medians.  Without ``--parent-tree`` the summary says so and
gives no verdict.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
BAR = 0.02


def child(tree: Path, noise: bool, rounds: int, clients: int):
    sys.path.insert(0, str(tree))
    import numpy as np

    import pygrid_amd
    from pygrid_amd import CLIPPED_MEAN, Engine
    from pygrid_amd.workloads import RESNET18_SHAPES

    pygrid_amd.tune_process(hw_queues=False)
    numel = [int(np.prod(s)) for s in RESNET18_SHAPES]
    P, N = sum(numel), clients
    with Engine(0) as eng:
        eng.set_layout(numel)
        eng.reserve(N)
        eng.synth_fill(1234, N)
        eng.ckpt_upload(np.zeros(P, np.float32))  # (every close's output is the next one's input)
        eng.set_clip_norm(1e-3)
        eng.row_sumsq(range(N))  # cached: the closes below are the fold (and K11) alone
        eng.sync()

        def close():
            eng.reset_stats()
            eng.fedavg_resident(CLIPPED_MEAN)
            eng.sync()
            st = eng.stats()
            return st["kernel_ms_total"], st["kernel_ms_last"], st["kernel_launches"]

        for r in range(rounds + 1):  # round 0 warms everything up
            rec = {"what": "noised" if noise else "parent_clipped", "round": r, "P": P, "clients": N}
            if noise:
                eng.set_dp_noise(0.0)
                rec["plain_ms"], _, n0 = close()
                eng.set_dp_noise(1.1, 0x5EED, r)
                rec["noised_ms"], rec["k11_ms"], n1 = close()
                assert (n0, n1) == (1, 2), (n0, n1)
                rec["sigma"] = eng.dp_stats()["sigma"]
            else:
                rec["clipped_ms"], _, n0 = close()
                assert n0 == 1, n0
            print(json.dumps(rec), flush=True)
        rec = {"what": "clip_stats", **eng.clip_stats()}
        print(json.dumps(rec), flush=True)


def run_child(tree: Path, noise: bool, args) -> list:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "noised" if noise else "parent", "--tree", str(tree),
           "--rounds", str(args.rounds), "--clients", str(args.clients)]
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
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", choices=["parent", "noised"], default=None)
    ap.add_argument("--tree", default=str(HERE))
    args = ap.parse_args()
    if args.child:
        return child(Path(args.tree).resolve(), args.child == "noised", args.rounds, args.clients)

    med = statistics.median
    parent, ours = [], []
    for _ in range(args.blocks):
        if args.parent_tree:
            parent += run_child(Path(args.parent_tree).resolve(), False, args)
        ours += run_child(HERE, True, args)
    k11 = med([r["k11_ms"] for r in ours])
    summary = {"what": "summary", "clients": args.clients, "P": ours[0]["P"], "k11_ms": k11,
               "k11_gbs": 12.0 * ours[0]["P"] / k11 / 1e6,
               "plain_ms": med([r["plain_ms"] for r in ours]), "noised_ms": med([r["noised_ms"] for r in ours]),
               "noised_fold_ms": med([r["noised_ms"] - r["k11_ms"] for r in ours]), "bar": BAR}
    if parent:
        p = med([r["clipped_ms"] for r in parent])
        summary.update(parent_clipped_ms=p, parent_min_ms=min(r["clipped_ms"] for r in parent),
                       parent_max_ms=max(r["clipped_ms"] for r in parent), k11_over_parent=k11 / p,
                       noised_over_parent=summary["noised_ms"] / p, within_bar=k11 / p <= BAR)
    else:
        summary.update(parent_clipped_ms=None, within_bar=None, note="no --parent-tree: the parent's close was not measured")
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
