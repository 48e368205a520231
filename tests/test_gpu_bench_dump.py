"""GPU: ``bench.py --dump-outputs DIR`` writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_new_checkpoint_the_oracle_computes(tmp_path):
    """A plain run of the default workload on a small shard (an odd size, more than one block): the
    line carries ms_per_step and the steps asked for and none of the --full parts, and
    new_checkpoint.npy is the fold of the run's own synthetic inputs, bit for bit."""
    from oracle import coracle
    from oracle import oracle as O

    P, N, seed = 70_001, 5, 77
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--params", str(P), "--clients", str(N), "--seed", str(seed), "--dump-outputs", str(tmp_path)],
                       cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["roofline"]["launches"] == 3
    assert rec["cpu_baseline"] is None and "config1" not in rec and "cycle_close_e2e" not in rec
    assert [f.name for f in tmp_path.iterdir()] == ["new_checkpoint.npy"]
    got = np.load(tmp_path / "new_checkpoint.npy")
    assert got.dtype == np.float32 and got.shape == (P,)
    u = np.arange(P, dtype=np.uint64)
    want = coracle.fedavg(0, np.stack([O.synth_diff(seed, c, u) for c in range(N)]), O.synth_ckpt(seed, u))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
