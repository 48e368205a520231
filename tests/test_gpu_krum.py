"""GPU: the Multi-Krum selection -- kernel K13's pairwise squared distances bit for bit against
tests/krum_oracle.py, K12 and tests/golden/krum_cases.npz, pgh_krum_select and its refusals, and the close over
the picked diffs in every averaging mode through the host layer.  Everything is compared as u64 / u32 bits."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_clip_golden as GG  # noqa: E402
import gen_krum_golden as GK  # noqa: E402
import geomed_oracle as GO  # noqa: E402
import krum_oracle as KO  # noqa: E402
import serveropt_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MEAN, ITERATIVE, WEIGHTED, CLIPPED, TRIMMED, MEDIAN, GEOMED = range(7)
ARG, STATE, OOM, UNSUPPORTED = -1, -3, -4, -6
RA, RC, RB = 8, 32, 4  # PAIRDIST_RA anchors and PAIRDIST_RC streamed rows per workgroup; K7's row group
SHAPE_P = (1, 4095, 4096, 4097, 2 * 4096 + 2048 + 3)  # K7's tile edges and a ragged last tile
# anchor-block, row-group and row-chunk remainders (the rows streamed past the first block are n - 1)
SHAPE_N = (2, 3, 5, 6, RA - 1, RA, RA + 1, RA + RB, 2 * RA + 3, RC + 1, RC + 2, RC + RA + 3)
P1 = 4097


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GK.GOLDEN)


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_clip_norm(0)
    engine.set_trim(0)
    engine.set_geomed(0)
    engine.set_server_opt(SO.NONE)


def make_engine(**env):
    """A context of its own: PGH_BLOCK_BYTES and PGH_PAIRDIST_BUDGET are read when a context is made."""
    from pygrid_amd import Engine

    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return Engine(int(os.environ.get("PGH_DEVICE", "0")))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def load(eng, diffs, slots=None, cap=None):
    eng.set_layout([diffs.shape[1]])
    eng.reserve(cap or len(diffs))
    for k, d in enumerate(diffs):
        eng.ingest(k if slots is None else int(slots[k]), d)


def refused(status, fn, *a):
    from pygrid_amd.exceptions import AggregationError

    with pytest.raises(AggregationError) as e:
        fn(*a)
    assert e.value.status == status, e.value


@functools.lru_cache(maxsize=None)
def shape_case(p, n=SHAPE_N[-1]):
    """n rows of p floats around a common centre, of mixed spread, and their distance matrix by the oracle: every
    smaller n takes the leading rows and the leading block."""
    rng = np.random.default_rng(13000 + p)
    centre = rng.standard_normal(p)
    rows = np.stack([(centre + rng.standard_normal(p) * 10.0 ** rng.integers(-2, 2)).astype(F) for _ in range(n)])
    D = KO.pairdist(rows)
    rows.setflags(write=False)
    D.setflags(write=False)
    return rows, D


def check_matrix(got, want):
    assert np.array_equal(u64(got), u64(want))
    assert np.array_equal(u64(got), u64(got.T))  # symmetric, bit for bit
    assert not u64(got.diagonal()).any()         # +0.0


# ---- K13 alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", SHAPE_P)
def test_row_pairdist_shapes(eng, p):
    rows, D = shape_case(p)
    load(eng, rows)
    sumsq = eng.row_sumsq(list(range(len(rows))))
    for n in SHAPE_N:
        got = eng.row_pairdist(list(range(n)))
        assert got.shape == (n, n)
        check_matrix(got, D[:n, :n])
    # row a of the matrix is K12 against the point d_b, bit for bit
    n = 2 * RA + 3
    got = eng.row_pairdist(list(range(n)))
    for b in (0, 1, RA, n - 1):
        assert np.array_equal(u64(got[:, b]), u64(eng.row_distsq(list(range(n)), rows[b]))), (p, b)
    # a contiguous run that does not start at slot 0
    check_matrix(eng.row_pairdist(list(range(3, 3 + RA + 2))), D[3:3 + RA + 2, 3:3 + RA + 2])
    # scattered, repeated and out of order
    slots = [5, 2, 40, 2, 17, 0, 33, 9, 41, 1, 30]
    want = D[np.ix_(slots, slots)]
    assert want[1, 3] == 0 and want[0, 1] != 0
    check_matrix(eng.row_pairdist(slots), want)
    assert eng.row_pairdist([]).shape == (0, 0) and not u64(eng.row_pairdist([4])).any()
    assert np.array_equal(u64(eng.row_sumsq(list(range(len(rows))))), u64(sumsq))  # K7's cached sums are untouched


def test_row_pairdist_scattered_slots_and_more_rows_than_a_row_table(eng):
    """513 rows in scattered slots of a larger slab, 4,097 params: the oracle for every pair of twelve rows with
    all the others, K12 for three whole columns, and the symmetry of everything."""
    n = 513
    rng = np.random.default_rng(5130)
    rows = (rng.standard_normal((n, P1)) * 0.1 + rng.standard_normal(P1)).astype(F)
    slot_of = rng.permutation(n + 7)[:n]
    load(eng, rows, slot_of, cap=n + 7)
    got = eng.row_pairdist(slot_of)
    assert np.array_equal(u64(got), u64(got.T)) and not u64(got.diagonal()).any()
    for a in (0, 1, 7, 8, 255, 256, 257, 300, 504, 505, 511, 512):
        want = [GO.row_distsq(rows[a], rows[b]) for b in range(n)]
        assert np.array_equal(u64(got[a]), u64(want)), a
    for b in (0, 256, 512):
        assert np.array_equal(u64(got[:, b]), u64(eng.row_distsq(slot_of, rows[b]))), b


def test_row_pairdist_narrow_blocks():
    """PGH_BLOCK_BYTES=4096: blocks of 1,024 columns, so every tile straddles four of them."""
    p = 70001
    rng = np.random.default_rng(p)
    rows = (rng.standard_normal((5, p)) * 0.3 + rng.standard_normal(p)).astype(F)
    want = KO.pairdist(rows)
    with make_engine(PGH_BLOCK_BYTES="4096") as e:
        load(e, rows, [5, 2, 7, 0, 3], cap=8)
        assert e.slab()[1] == 1024 and e.slab()[2] > 0
        check_matrix(e.row_pairdist([5, 2, 7, 0, 3]), want)
        load(e, rows)
        check_matrix(e.row_pairdist([0, 1, 2, 3, 4]), want)


def test_row_pairdist_past_one_fold_chunk(engine):
    """1,026 tile partials a pair: the fold of the partials fills its LDS chunk a second time."""
    p = 1024 * 4096 + 4097
    assert p in GG.WIDE_P
    rows = GG.wide_rows(p)[[0, 2, 4]]
    want = KO.pairdist(rows)
    assert np.isfinite(want).all() and len(set(u64(want[np.triu_indices(3, 1)]).tolist())) == 3
    for slots, cap in (([0, 1, 2], 3), ([3, 0, 2], 4)):
        load(engine, rows, slots, cap)
        check_matrix(engine.row_pairdist(slots), want)


def test_row_pairdist_batches_of_anchors():
    """The tile partials take 16 n bytes an anchor at 4,097 params: a budget of eight anchors' worth runs
    2 RA + 3 rows in three batches, one of three anchors' worth in batches shorter than an anchor block; the bits
    are the unbatched ones.  A budget below one anchor's worth is PGH_E_OOM and the context stays usable."""
    n = 2 * RA + 3
    rows, D = shape_case(P1)
    per_anchor = 8 * n * 2
    for anchors in (RA, 3, RA + 5):
        with make_engine(PGH_PAIRDIST_BUDGET=str(anchors * per_anchor)) as e:
            load(e, rows[:n])
            check_matrix(e.row_pairdist(list(range(n))), D[:n, :n])
            slots = list(range(n - 1, -1, -1))
            check_matrix(e.row_pairdist(slots), D[np.ix_(slots, slots)])
    with make_engine(PGH_PAIRDIST_BUDGET=str(per_anchor - 8)) as e:
        load(e, rows[:n])
        refused(OOM, e.row_pairdist, list(range(n)))
        check_matrix(e.row_pairdist(list(range(RA))), D[:RA, :RA])  # fewer rows fit


# ---- the selection --------------------------------------------------------------------------------------------------

def test_krum_select_golden_hostile_case(eng, G):
    diffs = G["hostile_diffs"]
    n = len(diffs)
    load(eng, diffs)
    inc = [int(s) for s in G["hostile_included"]]
    for _ in range(2):  # a second call gives identical results
        assert eng.krum_select(list(range(n)), GK.HOSTILE_F) == [int(s) for s in G["hostile_picked"]]
        st = eng.krum_stats()
        assert (st["rows"], st["excluded"], st["picked"]) == (12, 1, 7)
        assert np.array_equal(u64([st["max_picked_score"], st["min_dropped_score"]]), G["hostile_stats_bits"])
        check_matrix(eng.row_pairdist(inc), G["hostile_D_bits"].view(np.float64).reshape(len(inc), len(inc)))
    assert eng.krum_select(list(range(n)), GK.HOSTILE_F, 1) == [int(s) for s in G["hostile_picked_m1"]]
    assert eng.krum_select(list(range(n)), GK.HOSTILE_F, 3) == [int(s) for s in G["hostile_picked_m3"]]
    assert eng.krum_stats()["picked"] == 3
    # the NaN row is excluded wherever it stands, and the picked slots come in list order
    order = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]
    want = KO.krum(diffs[order], GK.HOSTILE_F)
    assert eng.krum_select(order, GK.HOSTILE_F) == [order[k] for k in want["picked"]]
    assert sorted(eng.krum_select(order, GK.HOSTILE_F)) == list(GK.HOSTILE_GOOD)
    # scattered slots of a larger slab
    slots = [14, 3, 9, 0, 21, 7, 12, 1, 19, 5, 16, 2]
    load(eng, diffs, slots, cap=24)
    assert eng.krum_select(slots, GK.HOSTILE_F) == [slots[k] for k in GK.HOSTILE_GOOD]


def test_krum_select_statuses_leave_the_context_usable(eng, G):
    from pygrid_amd import Engine
    from pygrid_amd.engine import I64

    diffs = G["hostile_diffs"]
    n, p = diffs.shape
    picked = [int(s) for s in G["hostile_picked"]]
    every = list(range(n))

    def still_right():
        load(eng, diffs)
        assert eng.krum_select(every, GK.HOSTILE_F) == picked

    load(eng, diffs)
    refused(STATE, eng.krum_select, every, GK.HOSTILE_F + 1)     # n' = 11 < 2 f + 3 = 13
    refused(STATE, eng.krum_select, every, GK.HOSTILE_F, 8)      # m > n' - f = 7
    refused(STATE, eng.krum_select, every[:6], 2)
    assert eng.krum_select(every, GK.HOSTILE_F) == picked
    refused(ARG, eng.krum_select, [0, 1, 2, 3, 1, 5, 6], 1)      # a slot listed twice
    refused(ARG, eng.krum_select, every, -1)
    refused(ARG, eng.krum_select, every, 1, -1)
    refused(ARG, eng.krum_select, [0, 1, 2, 3, 4, n], 1)         # outside the slab
    still_right()
    eng.set_layout([p])
    eng.reserve(n + 2)
    for k, d in enumerate(diffs):
        eng.ingest(k, d)
    refused(ARG, eng.krum_select, every + [n + 1], 1)            # an unoccupied slot
    assert eng.krum_select(every, GK.HOSTILE_F) == picked
    # more rows than PGH_KRUM_MAX_ROWS
    eng.set_layout([64])
    eng.reserve(1025)
    eng.synth_fill(5, 1025)
    refused(UNSUPPORTED, eng.krum_select, list(range(1025)), 1)
    refused(UNSUPPORTED, eng.row_pairdist, list(range(1025)))
    assert len(eng.krum_select(list(range(1024)), 100)) == 924
    still_right()
    # a narrower shard, a streaming context, an int64 slab, a group
    try:
        eng.set_layout([p])
        eng.set_shard(1000, p)
        eng.reserve(n)
        refused(UNSUPPORTED, eng.krum_select, every, 1)
        refused(UNSUPPORTED, eng.row_pairdist, every)
    finally:
        eng.set_layout([p])
    still_right()
    eng.stream_begin(MEAN)
    try:
        refused(UNSUPPORTED, eng.krum_select, every, 1)
        refused(UNSUPPORTED, eng.row_pairdist, every)
    finally:
        eng.set_layout([p])
    still_right()
    eng.set_layout([p])
    eng.reserve(4, I64, 2)
    try:
        refused(UNSUPPORTED, eng.krum_select, [0, 1, 2], 0)
        refused(UNSUPPORTED, eng.row_pairdist, [0, 1, 2])
    finally:
        eng.set_layout([p])
    still_right()
    with Engine(devices=[0, 0]) as grp:
        grp.set_layout([p])
        grp.reserve(n)
        for k, d in enumerate(diffs):
            grp.ingest(k, d)
        refused(UNSUPPORTED, grp.krum_select, every, GK.HOSTILE_F)
        refused(UNSUPPORTED, grp.row_pairdist, every)
        refused(UNSUPPORTED, grp.krum_stats)


# ---- the close over the picked diffs, in every mode, through the host layer --------------------------------------

def canonical(avg, item, num):
    return [(a * num + d) / (num + 1) for a, d in zip(avg, item)]


MODE_CASES = {
    "mean": ({}, {}),
    "iterative": ({"iterative_plan": True}, {"avg_plan": canonical}),
    "weighted": ({}, {"weights": [1.5, 2.0, 9.0, 0.5, 7.0, 1.0, 3.0, 8.0, 2.5, 6.0, 4.0, 5.0]}),
    "clipped": ({"diff_clip_norm": 30.0}, {}),
    "trimmed": ({"diff_trim_count": 2}, {}),
    "median": ({"diff_median": True}, {}),
    "geomed": ({"diff_geometric_median": True}, {}),
}
ADAM = {"server_optimizer": {"name": "fedadam", "lr": 0.05, "tau": 1e-3}}


@pytest.mark.parametrize("opt", [False, True], ids=["plain", "fedadam"])
@pytest.mark.parametrize("mode", list(MODE_CASES))
def test_close_composes_with_every_mode(eng, G, mode, opt):
    from pygrid_amd.cycle import CycleAggregator

    ckpt, diffs = G["hostile_ckpt"], G["hostile_diffs"]
    picked = [int(s) for s in G["hostile_picked"]]
    cfg, kw = MODE_CASES[mode]
    cfg = dict(cfg, **(ADAM if opt else {}))
    kw = dict(kw, **({"opt_key": "p"} if opt else {}))
    kw_picked = dict(kw)
    if "weights" in kw:
        kw_picked["weights"] = [kw["weights"][k] for k in picked]
    # (a fresh aggregator each: the optimizer's moments start again)
    got = CycleAggregator(eng).average_params(cfg, [ckpt], [[d] for d in diffs], krum={"byzantine": GK.HOSTILE_F}, **kw)
    want = CycleAggregator(eng).average_params(cfg, [ckpt], [[diffs[k]] for k in picked], **kw_picked)
    assert np.isfinite(want[0]).all() and np.array_equal(u32(got[0]), u32(want[0]))
    if mode == "mean" and not opt:  # the selection did something: all twelve rows give NaN or about 1e29
        plain = CycleAggregator(eng).average_params({}, [ckpt], [[d] for d in diffs])[0]
        assert np.isnan(plain).any() or np.abs(plain).max() > 1e28


def test_state_bytes_and_report_time_close(eng, G):
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.exceptions import KrumUnavailableError
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.settings import settings_of
    from pygrid_amd.state_schema import build_state_fast, parse_state

    ckpt, diffs = G["hostile_ckpt"], G["hostile_diffs"]
    picked = [int(s) for s in G["hostile_picked"]]
    shapes = [(40, 100), (97,)]
    assert sum(int(np.prod(s)) for s in shapes) == diffs.shape[1]

    def tensors(v):
        return [v[:4000].reshape(40, 100), v[4000:]]

    cfg = {"diff_krum": {"byzantine": GK.HOSTILE_F}, "diff_trim_count": 2}  # Multi-Krum, then the trimmed mean
    ck_pb, pbs = build_state_fast(tensors(ckpt)), [build_state_fast(tensors(d)) for d in diffs]
    agg = CycleAggregator(eng)
    new = agg.average_plan_diffs(cfg, ck_pb, pbs)
    want = agg.average_plan_diffs({"diff_trim_count": 2}, ck_pb, [pbs[k] for k in picked])
    got = np.concatenate([t.reshape(-1) for t in parse_state(new)])
    assert np.isfinite(got).all()
    assert np.array_equal(u32(got), u32(np.concatenate([t.reshape(-1) for t in parse_state(want)])))
    # report time: out of order, one worker never reports; nothing folds early, the close selects and finishes
    inc = IncrementalCycle(eng, [4000, 97], slots=13, fold_batch=2, checkpoint=ck_pb, settings=settings_of(cfg))
    for w in range(13):
        inc.assigned(w)
    for w in (3, 0, 6, 11, 1, 5, 9, 4, 2, 10, 8, 7):  # worker 12 never reports
        inc.reported(w, pbs[w])
    assert inc.folded_early == 0
    new2 = inc.close(ck_pb)
    assert np.array_equal(u32(np.concatenate([t.reshape(-1) for t in parse_state(new2)])), u32(got))
    lc, st = inc.last_close, eng.krum_stats()
    assert lc["n"] == 12 and lc["early"] == 0 and lc["trim"] == 2
    assert lc["krum"] == {"byzantine": GK.HOSTILE_F, "picked": 7, "excluded": 1,
                          "max_picked_score": st["max_picked_score"]}
    # an engine that cannot select -- a group -- fails closed instead of falling back
    from pygrid_amd import Engine

    with Engine(devices=[0]) as grp:
        with pytest.raises(KrumUnavailableError):
            CycleAggregator(grp).average_plan_diffs(cfg, ck_pb, pbs)
