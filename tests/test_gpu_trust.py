"""GPU: trust-bootstrapped FedAvg (PGH_TRUSTED_MEAN, FLTrust, kernel K14), bit-exact against
tests/trust_oracle.py and the golden file tests/golden/trust_cases.npz -- K14's sums as u64, every close as u32
(NaNs by position).  The definition is in include/pgh_api.h and DESIGN.md section 5."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import gen_trust_golden as GT  # noqa: E402
import krum_oracle as KO  # noqa: E402
import serveropt_oracle as SO  # noqa: E402
import trust_oracle as TO  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
TRUST, MEAN, I64 = 7, 0, 1
UNSUPPORTED, STATE, ARG = -6, -3, -1
RC = 32  # DISTSQ_RC: the rows a K14 workgroup streams past its tile of the root
SHAPE_P = (1, 3, 4095, 4096, 4097, 2 * 4096 + 2048 + 3)  # K7's tile edges and a ragged last tile
SHAPE_N = (1, 3, 4, 5, RC - 1, RC, RC + 1, 2 * RC + 3)  # row-group and row-chunk remainders


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GT.GOLDEN)


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_trust(False)
    engine.set_server_opt(SO.NONE)


def make_engine(**env):
    """A context of its own: PGH_BLOCK_BYTES is read when a context is made."""
    from pygrid_amd import Engine

    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return Engine(int(os.environ.get("PGH_DEVICE", "0")))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def load(eng, diffs, slots=None, cap=None, root=None):
    """A fresh layout and slab; with ``root`` the rule is on and the root set BEFORE the ingests (the dots ride
    behind each of them)."""
    eng.set_layout([diffs.shape[1]])
    eng.reserve(cap or len(diffs))
    if root is not None:
        eng.set_trust(True)
        eng.trust_root(root)
    for k, d in enumerate(diffs):
        eng.ingest(k if slots is None else int(slots[k]), d)


@functools.lru_cache(maxsize=None)
def shape_rows(p, n=SHAPE_N[-1]):
    """n rows of p floats of mixed length and angle to a root (row 0 along it, about a third pointing away), the
    root and a checkpoint: every N takes a prefix."""
    rng = np.random.default_rng(14000 + p)
    root = (rng.standard_normal(p) * 0.3).astype(F)
    root[0] = F(0.25)  # (never all zero, at P = 1 too)
    sign = np.where(rng.random(n) < 0.35, -1.0, 1.0)
    sign[0] = 1.0
    rows = np.stack([((sign[k] * root + rng.standard_normal(p) * 0.2) * 10.0 ** rng.integers(-2, 3)).astype(F) for k in range(n)])
    rows[0] = (root * F(3)).astype(F)
    return rows, root, rng.standard_normal(p).astype(F)


@functools.lru_cache(maxsize=None)
def shape_sums(p):
    rows, root, _ = shape_rows(p)
    return CO.row_sumsq(root), np.array([CO.row_sumsq(r) for r in rows]), np.array([TO.row_dot(r, root) for r in rows])


def want_of(ckpt, rows, s0, ss, dots):
    """The close of ``rows`` (their sums and dots given) from the oracle's host step and fold."""
    w = TO.trust_weights(s0, ss, dots)
    with np.errstate(all="ignore"):
        return (np.asarray(ckpt, F) - TO.weighted_sum([rows[k] for k in w["included"]], w["weights"])).astype(F)


@functools.lru_cache(maxsize=None)
def shape_want(p, n):
    rows, _, ckpt = shape_rows(p)
    s0, ss, dots = shape_sums(p)
    return want_of(ckpt, rows[:n], s0, ss[:n], dots[:n])


# ---- K14 alone ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", SHAPE_P)
def test_row_dot_shapes(eng, p):
    rows, root, ckpt = shape_rows(p)
    load(eng, rows)
    points = {"random": ckpt, "zero": np.zeros(p, F), "row": rows[2].copy(), "root": root}
    want = {k: u64([TO.row_dot(r, pt) for r in rows]) for k, pt in points.items()}
    assert not want["zero"].any()  # +0.0 against zeros, never -0.0
    assert np.array_equal(want["root"], u64(shape_sums(p)[2]))
    sumsq = eng.row_sumsq(list(range(len(rows))))
    assert want["row"][2] == u64(sumsq)[2]  # K14 of a row against itself is K7, bit for bit
    for n in SHAPE_N:
        for k, pt in points.items():
            got = eng.row_dot(list(range(n)), pt)
            assert np.array_equal(u64(got), want[k][:n]), (p, n, k)
    # a row table (scattered, repeated and out of order) gives each row the same bits
    slots = [5, 2, 66, 2, 40, 0, 33]
    assert np.array_equal(u64(eng.row_dot(slots, ckpt)), want["random"][slots])
    assert np.array_equal(u64(eng.row_sumsq(list(range(len(rows))))), u64(sumsq))  # K7's cache is untouched


def test_row_dot_narrow_blocks_and_the_golden_case(G):
    """PGH_BLOCK_BYTES=4096: blocks of 1,024 columns, so every tile straddles four of them."""
    p = 70001
    rng = np.random.default_rng(p)
    rows = (rng.standard_normal((5, p)) * 0.3 + rng.standard_normal(p)).astype(F)
    point, ckpt = rng.standard_normal(p).astype(F), rng.standard_normal(p).astype(F)
    with make_engine(PGH_BLOCK_BYTES="4096") as e:
        load(e, rows, [5, 2, 7, 0, 3], cap=8)
        assert e.slab()[1] == 1024 and e.slab()[2] > 0
        assert np.array_equal(u64(e.row_dot([5, 2, 7, 0, 3], point)), u64([TO.row_dot(r, point) for r in rows]))
        e.set_trust(True)
        e.trust_root(point)
        e.ckpt_upload(ckpt)
        e.fold_slots_finish_resident(TRUST, [5, 2, 7, 0, 3])
        assert np.array_equal(u32(e.ckpt_download()), u32(TO.fedavg_trust(ckpt, rows, point)))
        # the golden case in the same context
        load(e, G["fold_diffs"], [5, 2, 7, 0, 3], cap=8, root=G["fold_root"])
        assert np.array_equal(u64(e.row_dot([5, 2, 7, 0, 3], G["fold_root"])), G["fold_dot_bits"])
        assert np.array_equal(u64(e.row_sumsq([5, 2, 7, 0, 3])), G["fold_sumsq_bits"])
        e.ckpt_upload(G["fold_ckpt"])
        e.fold_slots_finish_resident(TRUST, [5, 2, 7, 0, 3])
        assert np.array_equal(u32(e.ckpt_download()), G["fold_out_bits"])


def test_row_dot_more_rows_than_a_row_table(eng):
    """515 scattered rows over 4,097 params: two RowTab launches; then the close over the same slots."""
    p, n = 4097, 515
    rng = np.random.default_rng(515)
    root = rng.standard_normal(p).astype(F)
    rows = (rng.standard_normal((n, p)) * 0.5 + root * rng.choice([-1.0, 1.0], (n, 1))).astype(F)
    ckpt = rng.standard_normal(p).astype(F)
    slot_of = rng.permutation(n + 3)[:n]
    load(eng, rows, slot_of, cap=n + 3)
    dots = np.array([TO.row_dot(r, root) for r in rows])
    assert np.array_equal(u64(eng.row_dot(slot_of, root)), u64(dots))
    eng.set_trust(True)
    eng.trust_root(root)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(TRUST, slot_of)
    want = want_of(ckpt, rows, CO.row_sumsq(root), [CO.row_sumsq(r) for r in rows], dots)
    assert TO.same_bits(eng.ckpt_download(), want)


def test_row_dot_past_one_chunk_of_the_partials_fold(eng):
    """3 rows of 1,026 tiles, the last tile five params short: the fold of the tile partials takes a second chunk."""
    p = 1026 * 4096 - 5
    rng = np.random.default_rng(1026)
    root = rng.standard_normal(p).astype(F)
    rows = np.stack([(root * s + rng.standard_normal(p)).astype(F) for s in (1.0, -0.5, 0.1)])
    ckpt = rng.standard_normal(p).astype(F)
    load(eng, rows)
    dots = np.array([TO.row_dot(r, root) for r in rows])
    assert np.array_equal(u64(eng.row_dot([0, 1, 2], root)), u64(dots))
    eng.set_trust(True)
    eng.trust_root(root)
    want = want_of(ckpt, rows, CO.row_sumsq(root), [CO.row_sumsq(r) for r in rows], dots)
    assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), u32(want))
    assert u64([eng.trust_stats()["root_norm"]])[0] == u64([np.sqrt(CO.row_sumsq(root))])[0]


# ---- the close ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", SHAPE_P)
def test_close_shapes_through_every_entry_point(eng, p):
    import torch

    rows, root, ckpt = shape_rows(p)
    ck = torch.from_numpy(ckpt).cuda()
    rng = np.random.default_rng(p)
    for n in SHAPE_N:
        want = shape_want(p, n)
        load(eng, rows[:n], root=root)
        got = eng.fedavg(TRUST, ckpt)
        assert np.array_equal(u32(got), u32(want)), (p, n)
        eng.ckpt_upload(ckpt)
        eng.fedavg_resident(TRUST)
        assert np.array_equal(u32(eng.ckpt_download()), u32(want)), (p, n)
        # two unequal ranges at a multiple of 4 that is neither a block nor a tile (one range where P <= 4)
        cut = 0 if p <= 4 else 4 * max(1, (p // 4) // 3)
        out = torch.zeros_like(ck)
        for a, b in ((0, cut), (cut, p)):
            if b > a:
                eng.fedavg_device_range(TRUST, a, b - a, ck.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(u32(out.cpu().numpy()), u32(want)), (p, n)
        # scattered slots, folded in a permuted order
        slot_of = rng.permutation(n + 5)[:n]
        order = rng.permutation(n)
        load(eng, rows[:n], slot_of, cap=n + 5, root=root)
        eng.ckpt_upload(ckpt)
        eng.fold_slots_finish_resident(TRUST, slot_of[order])
        s0, ss, dots = shape_sums(p)
        assert np.array_equal(u32(eng.ckpt_download()), u32(want_of(ckpt, rows[:n][order], s0, ss[:n][order], dots[:n][order]))), (p, n)


def test_golden_close_stats_and_a_repeated_close(eng, G):
    ckpt, diffs, root = G["fold_ckpt"], G["fold_diffs"], G["fold_root"]
    load(eng, diffs, root=root)
    assert eng.effective_variant(TRUST) == eng.effective_variant(2)  # what the weighted fold would run
    assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), G["fold_out_bits"])
    assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), G["fold_out_bits"])  # the close again: the same bits
    st, t = eng.trust_stats(), TO.trust(diffs, root)
    assert st["on"] and st["rows"] == 5 and st["excluded"] == 0 and st["trusted"] == t["trusted"] == 4
    assert u64([st["total_trust"]])[0] == G["fold_T_bits"][0] and u32([st["max_weight"]])[0] == u32([t["max_weight"]])[0]
    assert u64([st["root_norm"] ** 2])[0] != 0 and u64([st["root_norm"]])[0] == u64([t["root_norm"]])[0]
    # the root's s0 is pgh_row_sumsq of a slot holding the root
    eng.ingest(0, root)
    assert u64(eng.row_sumsq([0]))[0] == G["fold_s0_bits"][0]


def test_hostile_majority(eng, G):
    ckpt, diffs, root = G["hostile_ckpt"], G["hostile_diffs"], G["hostile_root"]
    load(eng, diffs, root=root)
    got = eng.fedavg(TRUST, ckpt)
    assert np.isfinite(got).all() and np.array_equal(u32(got), G["hostile_out_bits"])
    st = eng.trust_stats()
    assert st["rows"] == 10 and st["excluded"] == 0 and st["trusted"] == 3
    honest = TO.fedavg_trust(ckpt, diffs[list(GT.HONEST)], root)
    assert np.array_equal(got, honest)  # as values: 7 hostile rows of 10 moved nothing
    acc = ckpt.astype(np.float64) - got
    assert np.linalg.norm(acc) <= st["root_norm"] * 1.001


def test_nan_and_inf_rows_are_excluded(eng, G):
    ckpt, diffs, root = G["fold_ckpt"], G["fold_diffs"].copy(), G["fold_root"]
    diffs[1, 17] = np.nan
    diffs[4, 4098] = np.inf
    load(eng, diffs, root=root)
    got = eng.fedavg(TRUST, ckpt)
    assert np.isfinite(got).all() and np.array_equal(u32(got), u32(TO.fedavg_trust(ckpt, diffs, root)))
    assert np.array_equal(u32(got), u32(TO.fedavg_trust(ckpt, diffs[[0, 2, 3]], root)))
    st = eng.trust_stats()
    assert st["rows"] == 5 and st["excluded"] == 2
    # a clean diff into an excluded slot brings the row back
    eng.ingest(1, G["fold_diffs"][1])
    diffs[1] = G["fold_diffs"][1]
    assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), u32(TO.fedavg_trust(ckpt, diffs, root)))
    assert eng.trust_stats()["excluded"] == 1


def test_root_before_and_after_the_ingests_and_a_replaced_root(eng, G):
    ckpt, diffs, root = G["fold_ckpt"], G["fold_diffs"], G["fold_root"]
    load(eng, diffs, root=root)        # the dots ride behind each ingest
    before = eng.fedavg(TRUST, ckpt)
    load(eng, diffs)                    # the dots in one batch at the close
    eng.set_trust(True)
    eng.trust_root(root)
    after = eng.fedavg(TRUST, ckpt)
    assert np.array_equal(u32(before), G["fold_out_bits"]) and np.array_equal(u32(after), G["fold_out_bits"])
    root2 = (-root[::-1]).copy()
    eng.trust_root(root2)  # a new root: the cached dots and the weights are stale
    assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), u32(TO.fedavg_trust(ckpt, diffs, root2)))
    eng.trust_root(root)
    assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), G["fold_out_bits"])


@pytest.mark.parametrize("kind", SO.KINDS)
def test_server_optimizer_takes_the_trusted_mean(eng, G, kind):
    ckpt, diffs, root = G["fold_ckpt"], G["fold_diffs"], G["fold_root"]
    hp = {"lr": 0.3, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
    g = TO.trust(diffs, root)["acc"]
    m0, v0 = SO.init_state(diffs.shape[1], hp["tau"])
    want, _, _ = SO.step(kind, ckpt, g, m0, v0, **hp)
    load(eng, diffs, root=root)
    eng.set_server_opt(kind, hp["lr"], hp["beta1"], hp["beta2"], hp["tau"])
    assert SO.same_bits(eng.fedavg(TRUST, ckpt), want)
    assert SO.same_bits(eng.fedavg(TRUST, ckpt), want)  # nothing committed: the same step again


def test_after_a_krum_selection(eng, G):
    ckpt, diffs, root = G["hostile_ckpt"], G["hostile_diffs"], G["hostile_root"]
    load(eng, diffs, root=root)
    slots = list(range(len(diffs)))
    picked = eng.krum_select(slots, 2)
    assert picked == [slots[k] for k in KO.krum(diffs, 2, 0)["picked"]] and 0 < len(picked) < len(slots)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(TRUST, picked)
    assert np.array_equal(u32(eng.ckpt_download()), u32(TO.fedavg_trust(ckpt, diffs[picked], root)))


# ---- refusals and lifecycle ---------------------------------------------------------------------------------------

def test_refusals_and_lifecycle(eng, G):
    from pygrid_amd import Engine
    from pygrid_amd.exceptions import AggregationError

    ckpt, diffs, root = G["fold_ckpt"], G["fold_diffs"], G["fold_root"]
    p, n = diffs.shape[1], len(diffs)

    def refused(status, fn, *a):
        with pytest.raises(AggregationError) as e:
            fn(*a)
        assert e.value.status == status, e.value

    def still_right():
        load(eng, diffs, root=root)
        assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), G["fold_out_bits"])
        assert np.array_equal(u32(eng.fedavg(MEAN, ckpt)), u32(O.fedavg_mean([ckpt], [[d] for d in diffs])[0]))

    load(eng, diffs)
    refused(STATE, eng.fedavg, TRUST, ckpt)      # the mode with the rule off
    refused(STATE, eng.trust_root, root)         # the root needs the rule on
    eng.set_trust(True)
    refused(STATE, eng.fedavg, TRUST, ckpt)      # no root yet
    for bad in (np.zeros(p, F), np.where(np.arange(p) == 5, np.nan, root).astype(F),
                np.where(np.arange(p) == p - 1, np.inf, root).astype(F)):
        refused(ARG, eng.trust_root, bad)        # all zero, a NaN, an infinity
        refused(STATE, eng.fedavg, TRUST, ckpt)  # ... and no root is set
    refused(ARG, eng.trust_root, root[:-1])
    eng.trust_root(root)
    assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), G["fold_out_bits"])  # the context is usable
    eng.reset()                                   # reset keeps the rule and drops the root
    assert eng.trust_stats()["on"] and eng.trust_stats()["root_norm"] == 0.0
    for k, d in enumerate(diffs):
        eng.ingest(k, d)
    refused(STATE, eng.fedavg, TRUST, ckpt)
    eng.trust_root(root)
    assert np.array_equal(u32(eng.fedavg(TRUST, ckpt)), G["fold_out_bits"])
    eng.reserve(n)                                # so does reserve
    assert eng.trust_stats()["on"]
    for k, d in enumerate(diffs):
        eng.ingest(k, d)
    refused(STATE, eng.fedavg, TRUST, ckpt)
    eng.set_layout([p])                           # a new layout clears both
    assert not eng.trust_stats()["on"]
    still_right()
    eng.ckpt_upload(ckpt)
    refused(UNSUPPORTED, eng.fold_slots, TRUST, [0, 1])  # nothing can be folded early
    eng.fold_slots_finish_resident(TRUST, list(range(n)))  # ... and nothing was
    assert np.array_equal(u32(eng.ckpt_download()), G["fold_out_bits"])
    still_right()
    refused(UNSUPPORTED, eng.stream_begin, TRUST)
    still_right()
    eng.ckpt_upload(ckpt)
    eng.fold_slots(MEAN, [0, 1])  # a running fold state: the cycle cannot close with every row any more
    refused(STATE, eng.fold_slots_finish_resident, TRUST, list(range(2, n)))
    eng.fold_slots_finish_resident(MEAN, list(range(2, n)))
    still_right()
    # the mode beside DP noise: no un-noised average leaves the context
    eng.set_clip_norm(1.0)
    eng.set_dp_noise(1.0, 7, 1)
    try:
        refused(STATE, eng.fedavg, TRUST, ckpt)
    finally:
        eng.set_dp_noise(0.0)
        eng.set_clip_norm(0.0)
    still_right()
    # every row non-finite, and every row pointing away: nothing to fold
    bad = diffs.copy()
    bad[:, 3] = np.nan
    load(eng, bad, root=root)
    refused(STATE, eng.fedavg, TRUST, ckpt)
    load(eng, -np.abs(diffs), root=np.abs(root) + F(0.1))
    refused(STATE, eng.fedavg, TRUST, ckpt)
    eng.ckpt_upload(ckpt)
    refused(STATE, eng.fold_slots_finish_resident, TRUST, list(range(n)))
    still_right()
    # a streaming context, an int64 slab, a narrow shard, a group of one GPU
    eng.stream_begin(MEAN)
    try:
        refused(UNSUPPORTED, eng.set_trust, True)
    finally:
        eng.reset()
    still_right()
    eng.set_layout([p])
    eng.reserve(n, I64, 2)
    refused(UNSUPPORTED, eng.set_trust, True)
    try:
        eng.set_layout([p])
        eng.set_shard(1000, p)
        eng.reserve(n)
        refused(UNSUPPORTED, eng.set_trust, True)
        refused(UNSUPPORTED, eng.fedavg, TRUST, ckpt[1000:])
    finally:
        eng.set_layout([p])
    still_right()
    with Engine(devices=[0]) as grp:
        grp.set_layout([p])
        grp.reserve(n)
        refused(UNSUPPORTED, grp.set_trust, True)
        for k, d in enumerate(diffs):
            grp.ingest(k, d)
        refused(UNSUPPORTED, grp.fedavg, TRUST, ckpt)
        assert np.array_equal(u32(grp.fedavg(MEAN, ckpt)), u32(O.fedavg_mean([ckpt], [[d] for d in diffs])[0]))


# ---- through the host layer -----------------------------------------------------------------------------------------

SHAPES = [(40, 100), (100,), (7, 3), (1,)]


def model_case(n, hostile=(1, 2, 4, 5)):
    rng = np.random.default_rng(4147)
    ckpt = [rng.standard_normal(s).astype(F) for s in SHAPES]
    root = [(rng.standard_normal(s) * 1e-2).astype(F) for s in SHAPES]
    diffs = [[(r + rng.standard_normal(r.shape) * 2e-3).astype(F) for r in root] for _ in range(n)]
    for w in hostile:  # a hostile majority, pointing away with a large norm
        diffs[w] = [(x * F(-1e6)).astype(F) for x in diffs[w]]
    diffs[hostile[0]][0][0, :3] = (np.nan, np.inf, -np.inf)  # excluded besides
    return ckpt, diffs, root


def flat(ts):
    return np.concatenate([np.asarray(t, F).reshape(-1) for t in ts])


def test_cycle_aggregator_and_incremental_cycle(eng):
    from pygrid_amd import Engine
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.exceptions import TrustUnavailableError
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.settings import settings_of
    from pygrid_amd.state_schema import build_state_fast, parse_state

    ckpt, diffs, root = model_case(7)
    cfg = {"diff_trust_root": True}
    t = TO.trust([flat(d) for d in diffs], flat(root))
    want = (flat(ckpt) - t["acc"]).astype(F)
    assert np.isfinite(want).all() and t["excluded"] == 1 and t["trusted"] == 3
    agg = CycleAggregator(eng)
    pbs = [build_state_fast(d) for d in diffs]
    ck_pb, root_pb = build_state_fast(ckpt), build_state_fast(root)
    new = agg.average_plan_diffs(cfg, ck_pb, pbs, trust_root=root_pb)
    assert np.array_equal(u32(flat(parse_state(new))), u32(want))
    assert np.array_equal(u32(flat(agg.average_params(cfg, ckpt, diffs, trust_root=root))), u32(want))
    with pytest.raises(TrustUnavailableError):
        agg.average_plan_diffs(cfg, ck_pb, pbs)  # no root
    with pytest.raises(TrustUnavailableError):
        agg.average_plan_diffs(dict(cfg, diff_trim_count=1), ck_pb, pbs, trust_root=root_pb)
    with pytest.raises(TrustUnavailableError):
        agg.average_plan_diffs(cfg, ck_pb, pbs, trust_root=[np.zeros(s, F) for s in SHAPES])  # an all-zero root
    new2 = agg.average_plan_diffs({}, new, pbs[2:4])  # the next cycle without the key: the plain mean
    for got, w in zip(parse_state(new2), O.fedavg_mean(parse_state(new), diffs[2:4])):
        assert np.array_equal(u32(got), u32(w))
    assert not eng.trust_stats()["on"]
    # report time: out of order, one worker never reports; everything at the close, in assignment order.  The
    # root at construction (the dots ride behind each report) and at finish (one batch) give the same bytes.
    closes = []
    for when in ("construction", "finish"):
        kw = {"trust_root": root_pb} if when == "construction" else {}
        inc = IncrementalCycle(eng, [int(np.prod(s)) for s in SHAPES], slots=8, fold_batch=2, checkpoint=ck_pb,
                               settings=settings_of(cfg), **kw)
        for w in range(8):
            inc.assigned(w)
        for w in (3, 0, 6, 1, 5, 4, 2):  # worker 7 never reports
            inc.reported(w, pbs[w])
        closes.append(inc.close(ck_pb, **({} if kw else {"trust_root": root})))
        assert np.array_equal(u32(flat(parse_state(closes[-1]))), u32(want))
        lc, st = inc.last_close, eng.trust_stats()
        assert lc["n"] == 7 and lc["early"] == 0
        assert lc["trust"] == {"trusted": 3, "excluded": 1, "total_trust": st["total_trust"], "max_weight": st["max_weight"],
                               "root_norm": st["root_norm"]}
        assert u64([st["total_trust"]])[0] == u64([t["T"]])[0]
    # (fresh framing draws new tensor ids: the payloads are what must agree)
    assert np.array_equal(u32(flat(parse_state(closes[0]))), u32(flat(parse_state(closes[1]))))
    # an engine that cannot apply the rule -- a group -- fails closed instead of falling back
    with Engine(devices=[0]) as grp:
        with pytest.raises(TrustUnavailableError):
            CycleAggregator(grp).average_plan_diffs(cfg, ck_pb, pbs, trust_root=root_pb)
