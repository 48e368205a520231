"""GPU: what the averaging rules' state does at each lifecycle event of a context -- a slot written, the
weights replaced, a reset, a reserve, slot folds restarted, a shard set, the context made -- for clipping,
trimming, the median, the geometric median and the trust rule, bit-exact against tests/clip_oracle.py,
tests/trim_oracle.py, tests/median_oracle.py, tests/geomed_oracle.py and tests/trust_oracle.py; and what the rules
share: the two per-slot caches of K7's sums and K14's dots beside the uncached row calls (tests/krum_oracle.py for
the pairwise distances), the fold's weights as clipping, the caller and the geometric median write them in turn,
and the one plane of -0.0f under the server optimizer, the noise (tests/serveropt_oracle.py, tests/dp_oracle.py)
and the geometric median's inner folds.
(The server optimizer's events: test_gpu_serveropt.py::test_state_lifetime.)

    python tests/test_gpu_rule_lifecycle.py median | trimmed     (the child processes)
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import clip_oracle as CO  # noqa: E402
import dp_oracle as DO  # noqa: E402
import geomed_oracle as GO  # noqa: E402
import krum_oracle as KO  # noqa: E402
import median_oracle as MO  # noqa: E402
import serveropt_oracle as SO  # noqa: E402
import trim_oracle as TO  # noqa: E402
import trust_oracle as TR  # noqa: E402
from gen_trim_golden import special_rows  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MEAN, WEIGHTED, CLIPPED, TRIMMED, MEDIAN, GEOMED, TRUST = 0, 2, 3, 4, 5, 6, 7
STATE, UNSUPPORTED = -3, -6
P = 4101  # one full SUMSQ_TILE (4096) and a ragged tile of 5: not a multiple of 4
BOUND = 1.0
NU = 1e-6


def device():
    return int(os.environ.get("PGH_DEVICE", "0"))


@pytest.fixture(scope="module")
def eng():
    from pygrid_amd import Engine

    with Engine(device()) as e:
        yield e


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def clip_rows(n, seed):
    """n rows of norm ~0.64; rows 1, 4 and 7 of norm ~3.2 (clipped at BOUND); a checkpoint."""
    rng = np.random.default_rng(seed)
    d = (rng.standard_normal((n, P)) * 0.01).astype(F)
    d[1::3] *= F(5)
    return d, rng.standard_normal(P).astype(F)


def sums(rows):
    return [CO.row_sumsq(r) for r in rows]


def refused(status, text, fn, *a):
    from pygrid_amd.exceptions import AggregationError

    with pytest.raises(AggregationError) as e:
        fn(*a)
    assert e.value.status == status and text in str(e.value), e.value


# ---- clip: a slot written, the weights replaced ------------------------------------------------------------

@pytest.mark.parametrize("how", ["raw", "state"])
def test_clip_slot_written(eng, how):
    from pygrid_amd.state_schema import build_state_fast

    def ingest(slot, row):
        eng.ingest(slot, row) if how == "raw" else eng.ingest_state(slot, build_state_fast([row]))

    diffs, ckpt = clip_rows(6, 41)
    other = (diffs[0][::-1] * F(3)).astype(F)  # norm ~1.9: clipped, by another scale than rows 1 and 4
    s_other = CO.scale(CO.row_sumsq(other), BOUND)
    assert CO.scale(CO.row_sumsq(diffs[2]), BOUND) == 1 and s_other < 1 and s_other != CO.scales(diffs, BOUND)[1]
    diffs2 = diffs.copy()
    diffs2[2] = other
    eng.set_clip_norm(0)
    eng.set_layout([P])
    eng.reserve(6)
    try:
        # the cached sum of a slot goes with the diff it was of (clipping off: the sums are computed on demand)
        for k, d in enumerate(diffs):
            ingest(k, d)
        assert np.array_equal(u64(eng.row_sumsq(range(6))), u64(sums(diffs)))
        ingest(2, other)
        assert np.array_equal(u64(eng.row_sumsq(range(6))), u64(sums(diffs2)))
        # the same with the bound set (the sums are queued behind each ingest) and a resident fold
        # between the two writes: the slab's scales are computed again
        eng.set_clip_norm(BOUND)
        for k, d in enumerate(diffs):
            ingest(k, d)
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(CO.fedavg_clipped(ckpt, diffs, BOUND)))
        ingest(2, other)
        assert np.array_equal(u64(eng.row_sumsq([2])), u64(sums([other])))
        want2 = CO.fedavg_clipped(ckpt, diffs2, BOUND)
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(want2))
        # weights replaced: they took the place of the scales, which the next clipped fold computes again
        eng.set_weights([5.0] * 6)
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(want2))
    finally:
        eng.set_clip_norm(0)


# ---- clip: reset, reserve, slot folds restarted -------------------------------------------------------------

def test_clip_reset_reserve_restart(eng):
    diffs, ckpt = clip_rows(9, 42)
    norms = np.sqrt(sums(diffs))
    eng.set_layout([P])
    eng.reserve(6)
    eng.set_clip_norm(BOUND)
    try:
        for k in range(6):
            eng.ingest(k, diffs[k])
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(CO.fedavg_clipped(ckpt, diffs[:6], BOUND)))
        assert eng.clip_stats() == {"rows": 6, "clipped": 2, "max_norm": norms[:6].max()}
        eng.reset()
        assert eng.clip_stats() == {"rows": 0, "clipped": 0, "max_norm": 0.0}
        # a larger slab: the sum cache has its length (slots 6 .. 8 did not exist before)
        eng.reserve(9)
        for k in range(9):
            eng.ingest(k, diffs[k])
        assert np.array_equal(u64(eng.row_sumsq(range(9))), u64(sums(diffs)))
        assert eng.clip_stats()["rows"] == 0
        # part of a cycle folded, then the restart: the running tally goes with the folds
        eng.ckpt_upload(ckpt)
        eng.fold_slots(CLIPPED, [0, 1, 2, 3])
        assert eng.clip_stats() == {"rows": 4, "clipped": 1, "max_norm": norms[:4].max()}
        eng.fold_restart()
        assert eng.clip_stats() == {"rows": 0, "clipped": 0, "max_norm": 0.0}
        for k in range(4):  # (a fold frees its slots)
            eng.ingest(k, diffs[k])
        eng.fold_slots(CLIPPED, [0, 1, 2, 3, 4])
        eng.fold_slots_finish_resident(CLIPPED, [5, 6, 7, 8])
        assert np.array_equal(u32(eng.ckpt_download()), u32(CO.fedavg_clipped(ckpt, diffs, BOUND)))
        assert eng.clip_stats() == {"rows": 9, "clipped": 3, "max_norm": norms.max()}
    finally:
        eng.set_clip_norm(0)


# ---- clip: a shard set ---------------------------------------------------------------------------------------

def test_clip_shard_clears_the_bound_for_good(eng):
    diffs, ckpt = clip_rows(3, 43)
    eng.set_layout([P])
    eng.set_clip_norm(BOUND)
    try:
        eng.set_shard(0, 2048)  # a sub-range: a norm needs the whole row
        eng.reserve(3)
        for k in range(3):
            eng.ingest(k, diffs[k][:2048])
        refused(STATE, "PGH_CLIPPED_MEAN needs a bound: call pgh_set_clip_norm first", eng.fedavg, CLIPPED, ckpt[:2048])
        eng.set_shard(0, P)  # the whole model again: the bound does not come back by itself
        eng.reserve(3)
        for k in range(3):
            eng.ingest(k, diffs[k])
        refused(STATE, "PGH_CLIPPED_MEAN needs a bound: call pgh_set_clip_norm first", eng.fedavg, CLIPPED, ckpt)
        eng.set_clip_norm(BOUND)
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(CO.fedavg_clipped(ckpt, diffs, BOUND)))
    finally:
        eng.set_clip_norm(0)


# ---- geometric median: a slot written, the weights replaced ------------------------------------------------------

def geomed_saw(eng, rows, iters):
    """geomed_stats() is what the oracle gives for these rows: the counts, the objective and the largest weight by bits."""
    st, g = eng.geomed_stats(), GO.geomed(rows, iters, NU)
    return (st["iterations"] == iters and st["rows"] == len(rows) and st["excluded"] == g["excluded"] and
            u64([st["objective"]])[0] == u64([g["objective"]])[0] and u32([st["max_weight"]])[0] == u32([g["max_weight"]])[0])


def test_geomed_slot_written(eng):
    diffs, ckpt = clip_rows(6, 44)
    other = (diffs[0][::-1] * F(3)).astype(F)  # another norm than the row it replaces: other weights for every row
    diffs2 = diffs.copy()
    diffs2[2] = other
    diffs3 = diffs2.copy()
    diffs3[4, 1234] = np.inf
    eng.set_layout([P])
    eng.reserve(6)
    eng.set_geomed(3, NU)
    try:
        for k, d in enumerate(diffs):
            eng.ingest(k, d)
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(GO.fedavg_geomed(ckpt, diffs, 3, NU)))
        assert geomed_saw(eng, diffs, 3)
        # the slot's sum went with its diff and the slab's weights are computed again
        eng.ingest(2, other)
        want2 = GO.fedavg_geomed(ckpt, diffs2, 3, NU)
        assert not np.array_equal(u32(want2), u32(GO.fedavg_geomed(ckpt, diffs, 3, NU)))
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want2))
        assert geomed_saw(eng, diffs2, 3)
        # a row with one inf: its sum says so, the row is excluded
        eng.ingest(4, diffs3[4])
        want3 = GO.fedavg_geomed(ckpt, diffs3, 3, NU)
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want3))
        assert eng.geomed_stats()["excluded"] == 1 and geomed_saw(eng, diffs3, 3)
        # weights replaced: they took the place of the rule's, which the next fold computes again
        eng.set_weights([5.0] * 6)
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want3))
    finally:
        eng.set_geomed(0)


# ---- geometric median: reset, reserve, a shard set ----------------------------------------------------------------

def test_geomed_reset_reserve_shard(eng):
    diffs, ckpt = clip_rows(9, 45)
    eng.set_layout([P])
    eng.reserve(6)
    eng.set_geomed(3, NU)
    try:
        for k in range(6):
            eng.ingest(k, diffs[k])
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(GO.fedavg_geomed(ckpt, diffs[:6], 3, NU)))
        assert geomed_saw(eng, diffs[:6], 3)
        eng.reset()  # the tallies go, the setting stays
        assert eng.geomed_stats() == {"iterations": 3, "rows": 0, "excluded": 0, "objective": 0.0, "max_weight": 0.0}
        # another slot count: the sum cache has its length; the iterate plane and the distances are allocated anew
        eng.reserve(9)
        eng.set_geomed(2, NU)
        for k in range(9):
            eng.ingest(k, diffs[k])
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(GO.fedavg_geomed(ckpt, diffs, 2, NU)))
        assert geomed_saw(eng, diffs, 2)
        # a sub-range shard drops the setting: the distances need whole rows
        eng.set_shard(0, 2048)
        assert eng.geomed_stats()["iterations"] == 0
        eng.reserve(3)
        for k in range(3):
            eng.ingest(k, diffs[k][:2048])
        refused(UNSUPPORTED, "a geometric median needs whole rows: the shard [0,2048) is narrower than the model", eng.fedavg, GEOMED,
                ckpt[:2048])
        refused(UNSUPPORTED, "pgh_set_geomed: the shard [0,2048) is narrower than the model", eng.set_geomed, 3, NU)
        eng.set_shard(0, P)  # the whole model again: the setting does not come back by itself
        eng.reserve(3)
        for k in range(3):
            eng.ingest(k, diffs[k])
        refused(STATE, "PGH_GEOMETRIC_MEDIAN needs its setting: call pgh_set_geomed first", eng.fedavg, GEOMED, ckpt)
        eng.set_geomed(2, NU)
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(GO.fedavg_geomed(ckpt, diffs[:3], 2, NU)))
    finally:
        eng.set_layout([P])


# ---- trust rule: a slot written, the root replaced; the uncached row calls beside the two caches ---------------------

def trust_rows(n, p, seed):
    """n rows of p floats of mixed length and angle to a root (about a third pointing away, row 1 among them; rows
    0 and 2 along it), the root and a checkpoint."""
    rng = np.random.default_rng(seed)
    root = (rng.standard_normal(p) * 0.3).astype(F)
    sign = np.where(rng.random(n) < 0.35, -1.0, 1.0)
    sign[[0, 2]] = 1.0
    sign[1] = -1.0
    rows = np.stack([((sign[k] * root + rng.standard_normal(p) * 0.2) * 10.0 ** rng.integers(-1, 2)).astype(F) for k in range(n)])
    return rows, root, rng.standard_normal(p).astype(F)


def trust_saw(eng, rows, root):
    """trust_stats() is what the oracle gives for these rows and this root: the counts, and T, the largest weight
    and the root's norm by bits."""
    st, t = eng.trust_stats(), TR.trust(rows, root)
    return (st["on"] and st["rows"] == len(rows) and st["excluded"] == t["excluded"] and st["trusted"] == t["trusted"] and
            u64([st["total_trust"]])[0] == u64([t["T"]])[0] and u32([st["max_weight"]])[0] == u32([t["max_weight"]])[0] and
            u64([st["root_norm"]])[0] == u64([t["root_norm"]])[0])


def test_trust_slot_written(eng):
    diffs, root, ckpt = trust_rows(6, P, 50)
    rng = np.random.default_rng(51)
    other = ((root * F(0.5) + rng.standard_normal(P)) * F(3)).astype(F)  # another norm and angle than the row it replaces
    diffs2 = diffs.copy()
    diffs2[2] = other
    diffs3 = diffs2.copy()
    diffs3[4, 1234] = np.inf
    diffs4 = diffs3.copy()
    diffs4[1] = (root * F(2) - diffs[1]).astype(F)
    root2 = (root[::-1] * F(0.7) + diffs[0] * F(0.1)).astype(F)
    eng.set_layout([P])
    eng.reserve(6)
    eng.set_trust(True)
    try:
        eng.trust_root(root)  # ahead of the ingests: K14 is queued behind each of them
        for k, d in enumerate(diffs):
            eng.ingest(k, d)
        assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), u32(TR.fedavg_trust(ckpt, diffs, root)))
        assert trust_saw(eng, diffs, root)
        # the slot's sum and dot went with its diff and the slab's weights are computed again
        eng.ingest(2, other)
        want2 = TR.fedavg_trust(ckpt, diffs2, root)
        assert not np.array_equal(u32(want2), u32(TR.fedavg_trust(ckpt, diffs, root)))
        assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), u32(want2))
        assert trust_saw(eng, diffs2, root)
        # a row with one inf: its sum says so, the row is excluded
        eng.ingest(4, diffs3[4])
        assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), u32(TR.fedavg_trust(ckpt, diffs3, root)))
        assert eng.trust_stats()["excluded"] == 1 and trust_saw(eng, diffs3, root)
        # the root replaced between a re-ingest and the close: the dot queued behind the ingest was the old root's
        eng.ingest(1, diffs4[1])
        eng.trust_root(root2)
        want4 = TR.fedavg_trust(ckpt, diffs4, root2)
        assert not np.array_equal(u32(want4), u32(TR.fedavg_trust(ckpt, diffs4, root)))
        assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), u32(want4))
        assert eng.trust_stats()["excluded"] == 1 and trust_saw(eng, diffs4, root2)
    finally:
        eng.set_trust(False)


@pytest.mark.parametrize("slots", [list(range(33)), [5, 2, 7, 0, 3]], ids=["run33", "scattered5"])
def test_row_calls_between_ingest_and_close(eng, slots):
    """p = 4097, n = 33: one param past a tile, one row past a DISTSQ_RC chunk of 32; a scattered list goes to the
    kernels as a row table.  The uncached calls share the tile partials with the queued K7 and K14 and leave both
    caches as they were."""
    p, n = 4097, len(slots)
    rows, root, ckpt = trust_rows(n, p, 52 + n)
    point = np.random.default_rng(53).standard_normal(p).astype(F)
    t = TR.trust(rows, root)
    want = (ckpt - t["acc"]).astype(F)

    def ingest_all():
        for k, d in enumerate(rows):
            eng.ingest(slots[k], d)

    def close():
        if slots == list(range(n)):
            return eng.fedavg(TRUST, ckpt)
        eng.ckpt_upload(ckpt)
        eng.fold_slots_finish_resident(TRUST, slots)
        return eng.ckpt_download()

    eng.set_layout([p])
    eng.reserve(max(slots) + 1)
    eng.set_trust(True)
    try:
        eng.trust_root(root)
        ingest_all()  # K7 and K14 are queued behind each ingest, and nothing has waited for them
        assert np.array_equal(u64(eng.row_dot(slots, point)), u64([TR.row_dot(r, point) for r in rows]))
        assert np.array_equal(u64(eng.row_distsq(slots, point)), u64([GO.row_distsq(r, point) for r in rows]))
        assert np.array_equal(u64(eng.row_pairdist(slots[:5])), u64(KO.pairdist(rows[:5])))
        assert np.array_equal(u64(eng.row_sumsq(slots)), u64(t["sumsq"]))
        assert np.array_equal(u32(close()), u32(want))
        assert t["excluded"] == 0 and 0 < t["trusted"] < n and trust_saw(eng, rows, root)
        if slots != list(range(n)):
            ingest_all()  # (a slot fold frees its slots)
        assert np.array_equal(u32(close()), u32(want))
        assert trust_saw(eng, rows, root)
    finally:
        eng.set_trust(False)


# ---- the fold's weights: clipping, the caller and the geometric median write them in turn ---------------------------

def test_weights_change_hands(eng):
    """37 rows: one K12 chunk of 32 and one of 5 whose second row group repeats its last row; ten K7 row groups."""
    n, iters = 37, 3
    diffs, ckpt = clip_rows(n, 46)
    rows = list(diffs)
    w = (np.random.default_rng(47).random(n) + 0.5).astype(F)
    norms = np.sqrt(sums(rows))
    n_clipped = int(np.sum(CO.scales(rows, BOUND) != 1))
    assert 0 < n_clipped < n
    want_clip = CO.fedavg_clipped(ckpt, rows, BOUND)
    want_w = O.fedavg_weighted([ckpt], [[d] for d in rows], w)[0]
    want_geo = GO.fedavg_geomed(ckpt, rows, iters, NU)
    assert len({u32(x).tobytes() for x in (want_clip, want_w, want_geo)}) == 3

    def clip_saw(closes):  # every close that computed the slab's scales counted its rows
        return eng.clip_stats() == {"rows": closes * n, "clipped": closes * n_clipped, "max_norm": norms.max()}

    eng.set_layout([P])
    eng.reserve(n)
    eng.set_clip_norm(BOUND)
    eng.set_geomed(iters, NU)
    try:
        for k, d in enumerate(rows):
            eng.ingest(k, d)
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(want_clip))  # 1: the scales
        assert clip_saw(1)
        eng.set_weights(w)                                                     # 2: the caller's
        assert np.array_equal(u32(eng.fedavg(WEIGHTED, ckpt)), u32(want_w))
        assert clip_saw(1)
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want_geo))    # 3: the Weiszfeld weights
        assert geomed_saw(eng, rows, iters) and clip_saw(1)
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(want_clip))  # 4: the scales, computed again
        assert clip_saw(2)
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want_geo))    # 5
        assert geomed_saw(eng, rows, iters) and clip_saw(2)
        # 6: the same rows in shuffled slots, the clipped close as slot folds in two calls
        slot_of = np.random.default_rng(48).permutation(n)
        assert np.any(np.diff(slot_of) != 1)
        eng.reset()
        for k, d in enumerate(rows):
            eng.ingest(int(slot_of[k]), d)
        eng.ckpt_upload(ckpt)
        eng.fold_slots(CLIPPED, slot_of[:20])
        eng.fold_slots_finish_resident(CLIPPED, slot_of[20:])
        assert np.array_equal(u32(eng.ckpt_download()), u32(want_clip))
        assert clip_saw(1)
        # 7: again, the geometric median as one slot close: a list that is no run of slots goes as RowTabs
        for k, d in enumerate(rows):
            eng.ingest(int(slot_of[k]), d)
        eng.ckpt_upload(ckpt)
        eng.fold_slots_finish_resident(GEOMED, slot_of)
        assert np.array_equal(u32(eng.ckpt_download()), u32(want_geo))
        assert geomed_saw(eng, rows, iters) and clip_saw(1)
    finally:
        eng.set_clip_norm(0)
        eng.set_geomed(0)


# ---- the -0 plane: one for the server optimizer, the noise and the geometric median ---------------------------------

def test_one_negative_zero_plane(eng):
    """Every tenant folds its FINAL against the context's one plane of -0.0f: it is still -0 after each of them, and
    a tenant switched off does not take it along."""
    n, key, rnd, z = 5, 0xDEADBEEF0BADF00D, 0xFFFFFFFE, 1.1
    lr, beta1 = 0.3, 0.9
    diffs, ckpt = clip_rows(n, 49)
    rows = list(diffs)
    g_clip = SO.avg_from(lambda ck: CO.fedavg_clipped(ck, rows, BOUND), P)
    g_mean = SO.avg_from(lambda ck: O.fedavg_mean([ck], [[d] for d in rows])[0], P)
    m0, v0 = SO.init_state(P, 0.0)

    def momentum(g):
        return SO.step(SO.MOMENTUM, ckpt, g, m0, v0, lr, beta1, 0.0, 0.0)[0]

    eng.set_layout([P])
    eng.reserve(n)
    eng.set_clip_norm(BOUND)
    eng.set_geomed(2, NU)
    try:
        for k, d in enumerate(rows):
            eng.ingest(k, d)
        # FedAvgM behind the noise behind the clipped fold
        eng.set_server_opt(SO.MOMENTUM, lr, beta1)
        eng.set_dp_noise(z, key, rnd)
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(momentum(DO.noised_avg(g_clip, key, rnd, z, BOUND, n))))
        # the optimizer off: the noise alone
        eng.set_server_opt(SO.NONE)
        assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(DO.close(ckpt, g_clip, key, rnd, z, BOUND, n)))
        # the noise off: the geometric median's inner fold
        eng.set_dp_noise(0.0)
        assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(GO.fedavg_geomed(ckpt, rows, 2, NU)))
        # the optimizer on again (its moments begin anew) under a plain mean
        eng.set_server_opt(SO.MOMENTUM, lr, beta1)
        assert np.array_equal(u32(eng.fedavg(MEAN, ckpt)), u32(momentum(g_mean)))
    finally:
        eng.set_server_opt(SO.NONE)
        eng.set_dp_noise(0.0)
        eng.set_clip_norm(0)
        eng.set_geomed(0)


# ---- trim: the state planes over a reserve; b and the slot folds -----------------------------------------------

def three_step_trimmed(eng, diffs, ckpt):
    n = len(diffs)
    for k, d in enumerate(diffs):
        eng.ingest(k, d)
    eng.ckpt_upload(ckpt)
    eng.fold_slots(TRIMMED, [0, 1])
    eng.fold_slots(TRIMMED, [2])
    eng.fold_slots_finish_resident(TRIMMED, list(range(3, n)))
    return eng.ckpt_download()


@pytest.mark.parametrize("b", (1, 2))
def test_trim_planes_over_a_reserve(eng, b):
    n = 2 * b + 3  # 5 slots, 7 slots
    rows = special_rows(2 * n + 3, P, 700 + b)
    ckpt = np.random.default_rng(b).standard_normal(P).astype(F)
    first, second = rows[:n], rows[n:]
    eng.set_trim(0)
    eng.set_layout([P])
    eng.reserve(n)
    eng.set_trim(b)
    try:
        assert TO.same_bits(three_step_trimmed(eng, first, ckpt), TO.fedavg_trimmed(ckpt, first, b))
        eng.reserve(n + 3)  # the planes went with the slab and are made again
        assert TO.same_bits(three_step_trimmed(eng, second, ckpt), TO.fedavg_trimmed(ckpt, second, b))
        # b is the cycle's: fixed while its slot folds are under way
        for k in range(3):
            eng.ingest(k, first[k])
        eng.fold_slots(TRIMMED, [0, 1])
        refused(STATE, "trim count changed", eng.set_trim, b + 1)
        eng.fold_restart()
        eng.set_trim(b + 1)
    finally:
        eng.fold_restart()
        eng.set_trim(0)


# ---- median: the device row table over a reserve; the environment at creation ------------------------------------

def test_median_row_table_over_a_reserve(eng):
    p = 64
    rows = special_rows(600, p, 900, every=5, rows=600)
    ckpt = np.random.default_rng(9).standard_normal(p).astype(F)
    eng.set_layout([p])
    for n in (520, 600):  # both past a RowTab's 512 rows: the slots go to K9 as a device table of `slots` entries
        eng.reserve(n)
        order = np.random.default_rng(n).permutation(n)
        for k in range(n):
            eng.ingest(int(order[k]), rows[k])
        eng.ckpt_upload(ckpt)
        assert eng.effective_variant(MEDIAN) == 50
        eng.fold_slots_finish_resident(MEDIAN, order)
        assert MO.same_bits(eng.ckpt_download(), MO.fedavg_median(ckpt, rows[:n])), n


def child(what, **env):
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), what], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_median_path_is_read_at_creation():
    assert "median variant 51" in child("median", PGH_MEDIAN_PATH="passes")


def test_trim_vec_is_read_at_creation():
    assert child("trimmed", PGH_TRIM_VEC="1").split() == ["trimmed", "variant", "41", "trimmed", "variant", "40"]


if __name__ == "__main__":
    if sys.argv[1:] not in (["median"], ["trimmed"]):
        sys.exit("usage: test_gpu_rule_lifecycle.py median | trimmed")
    from pygrid_amd import Engine

    for vec in (None,) if sys.argv[1] == "median" else (None, "4"):  # (None: the environment as the parent set it)
        if vec:
            os.environ["PGH_TRIM_VEC"] = vec
        with Engine(device()) as made:
            made.set_layout([P])
            made.reserve(5)
            if sys.argv[1] == "median":
                for k in range(5):
                    made.ingest(k, np.full(P, k, F))
                print("median variant", made.effective_variant(MEDIAN))
            else:
                made.set_trim(1)
                print("trimmed variant", made.effective_variant(TRIMMED))
