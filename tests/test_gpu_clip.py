"""GPU: per-client L2 clipping (PGH_CLIPPED_MEAN), bit-exact against tests/clip_oracle.py and the
golden file tests/golden/clip_cases.npz -- K7's sums of squares as u64, every fold as u32 (NaNs by
position).  The definition of the sum's order is in DESIGN.md section 5."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import gen_clip_golden as GG  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
UNSUPPORTED, STATE = -6, -3


@pytest.fixture(scope="module")
def G():
    return np.load(GG.GOLDEN)


@pytest.fixture(scope="module")
def fold_case(G):
    """The 7-row slab of case 3 and what the oracle makes of it (computed once, checked against the
    golden file, shared by the fold tests)."""
    ckpt, diffs, c = G["fold_ckpt"], G["fold_diffs"], float(G["fold_c"])
    s = CO.scales(diffs, c)
    assert np.array_equal(s.view(np.uint32), G["fold_scales"].view(np.uint32))
    # a condition on the inputs: rows 2, 4 and 6 are clipped, four are left alone
    assert [bool(x == 1) for x in s] == [True, True, False, True, False, True, False]
    want = CO.fold(diffs, s, ckpt)
    assert np.array_equal(want.view(np.uint32), G["fold_out"].view(np.uint32))
    return ckpt, diffs, c, want


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def load(eng, diffs, slots=None, cap=None):
    P = diffs.shape[1]
    eng.set_layout([P])
    eng.reserve(cap or len(diffs))
    for k, d in enumerate(diffs):
        eng.ingest(k if slots is None else slots[k], d)


def rows_of(G, p):
    return G[f"rows_{p}"] if p <= GG.STORED_P_MAX else GG.mixed_rows(p)


@pytest.mark.parametrize("p", GG.SUMSQ_P)
def test_row_sumsq_shapes(engine, G, p):
    rows = rows_of(G, p)
    slots = [5, 2, 7]
    load(engine, rows, slots, cap=8)
    got = engine.row_sumsq(slots)
    assert np.array_equal(u64(got), G[f"sumsq_bits_{p}"]), (got, G[f"sumsq_bits_{p}"].view(np.float64))
    assert np.array_equal(u64(got), u64([CO.row_sumsq(r) for r in rows]))
    # another diff into one slot: its cached sum goes, the others stay
    other = (rows[0][::-1] * F(3)).astype(F)
    engine.ingest(2, other)
    got = engine.row_sumsq([7, 2, 5])
    assert np.array_equal(u64(got), u64([CO.row_sumsq(rows[2]), CO.row_sumsq(other), CO.row_sumsq(rows[0])]))


def test_row_sumsq_narrow_blocks(monkeypatch, G):
    """PGH_BLOCK_BYTES=4096: blocks of 1,024 columns, so every tile straddles four of them."""
    from pygrid_amd import Engine

    monkeypatch.setenv("PGH_BLOCK_BYTES", "4096")
    rows = GG.mixed_rows(70001)
    with Engine(0) as eng:
        load(eng, rows, [5, 2, 7], cap=8)
        assert eng.slab()[1] == 1024 and eng.slab()[2] > 0
        got = eng.row_sumsq([5, 2, 7])
    assert np.array_equal(u64(got), G["sumsq_bits_70001"])


def _variants(eng):
    from pygrid_amd.exceptions import AggregationError

    ok = []
    for v in range(-1, 64):
        try:
            eng.set_variant(v)
            ok.append(v)
        except AggregationError:
            pass
    eng.set_variant(-1)
    return ok


def test_clipped_fold_every_variant(engine, fold_case):
    import torch

    ckpt, diffs, c, want = fold_case
    P = diffs.shape[1]
    load(engine, diffs)
    engine.set_clip_norm(c)
    variants = _variants(engine)
    assert len(variants) >= 25
    ck = torch.from_numpy(ckpt).cuda()
    try:
        for v in variants:
            engine.set_variant(v)
            assert np.array_equal(u32(engine.fedavg(3, ckpt)), u32(want)), v
            engine.ckpt_upload(ckpt)
            engine.fedavg_resident(3)
            assert np.array_equal(u32(engine.ckpt_download()), u32(want)), v
            out = torch.zeros_like(ck)
            cut = 4100  # a multiple of 4, not of the tile
            engine.fedavg_device_range(3, 0, cut, ck.data_ptr(), out.data_ptr())
            engine.fedavg_device_range(3, cut, P - cut, ck.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(u32(out.cpu().numpy()), u32(want)), v
    finally:
        engine.set_variant(-1)
        engine.set_clip_norm(0)
    st = engine.clip_stats()
    assert st["rows"] == 7 and st["clipped"] == 3  # the scales were computed once for this slab
    norms = np.sqrt([CO.row_sumsq(d) for d in diffs])
    assert st["max_norm"] == norms.max()


def test_huge_bound_is_the_plain_mean(engine, fold_case):
    ckpt, diffs, _, _ = fold_case
    load(engine, diffs)
    engine.set_clip_norm(1e30)
    try:
        got = engine.fedavg(3, ckpt)
    finally:
        engine.set_clip_norm(0)
    mean = engine.fedavg(0, ckpt)
    assert np.array_equal(u32(got), u32(mean))
    assert np.array_equal(u32(got), u32(O.fedavg_mean([ckpt], [[d] for d in diffs])[0]))


def test_boundary_rows(engine, G):
    ckpt, diffs = G["bnd_ckpt"], G["bnd_diffs"]
    load(engine, diffs)
    sums = engine.row_sumsq([0, 1, 2])
    assert sums[0] == 25.0 and np.array_equal(u64(sums), G["bnd_sumsq_bits"])
    try:
        for k, c in enumerate(G["bnd_c"]):
            engine.set_clip_norm(float(c))
            got = engine.fedavg(3, ckpt)
            assert np.array_equal(u32(got), u32(G["bnd_out"][k])), c
            assert np.array_equal(u32(got), u32(CO.fedavg_clipped(ckpt, diffs, c))), c
    finally:
        engine.set_clip_norm(0)
    assert G["bnd_scales"][0][0] == 1 and G["bnd_scales"][1][0] == F(np.float64(G["bnd_c"][1]) / 5.0) < 1


def test_non_finite_rows(engine, G):
    ckpt, diffs, c = G["nf_ckpt"], G["nf_diffs"], float(G["nf_c"])
    load(engine, diffs)
    engine.set_clip_norm(c)
    try:
        sums = engine.row_sumsq([0, 1, 2, 3])
        got = engine.fedavg(3, ckpt)
    finally:
        engine.set_clip_norm(0)
    assert np.isinf(sums[1]) and np.isnan(sums[2]) and np.array_equal(u64(sums[[0, 3]]), u64(
        [CO.row_sumsq(diffs[0]), CO.row_sumsq(diffs[3])]))
    assert G["nf_scales"][1] == 0 and np.isnan(G["nf_scales"][2])
    assert CO.same_bits(got, G["nf_out"]) and CO.same_bits(got, CO.fedavg_clipped(ckpt, diffs, c))
    assert np.isnan(got).all()  # the NaN scale reaches every param; IEEE, not sanitised


def test_more_rows_than_a_row_table(engine):
    """600 slots in shuffled order, three early fold_slots batches plus the finish: more rows than
    one K7 launch or one fold launch takes (512), sums computed at ingest and at the folds."""
    P, N, C = 257, 600, 1.0
    rng = np.random.default_rng(600)
    diffs = (rng.standard_normal((N, P)) * 0.01).astype(F)
    diffs[::10] *= F(50)  # every 10th row has a norm of ~8: clipped
    ckpt = rng.standard_normal(P).astype(F)
    slot_of = rng.permutation(N)
    s = CO.scales(diffs, C)
    assert [bool(x < 1) for x in s] == [k % 10 == 0 for k in range(N)]
    want = CO.fold(diffs, s, ckpt)
    engine.set_layout([P])
    engine.reserve(N)
    for k in range(300):  # half without a bound: their sums are missing when the folds need them
        engine.ingest(int(slot_of[k]), diffs[k])
    engine.set_clip_norm(C)
    try:
        for k in range(300, N):
            engine.ingest(int(slot_of[k]), diffs[k])
        engine.ckpt_upload(ckpt)
        for a, b in ((0, 100), (100, 250), (250, 400)):
            engine.fold_slots(3, slot_of[a:b])
        engine.fold_slots_finish_resident(3, slot_of[400:])
        got = engine.ckpt_download()
        st = engine.clip_stats()
    finally:
        engine.set_clip_norm(0)
    assert np.array_equal(u32(got), u32(want))
    assert st["rows"] == N and st["clipped"] == 60
    assert st["max_norm"] == np.sqrt([CO.row_sumsq(d) for d in diffs]).max()


def test_cycle_aggregator_from_state_bytes(engine):
    """MNIST size, three clients, one clipped; then a chained cycle WITHOUT the key is the plain
    mean: the bound does not leak into the next FL process's cycle."""
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.state_schema import build_state_fast, parse_state

    shapes = [(392, 784), (392,), (10, 392), (10,)]
    assert sum(int(np.prod(s)) for s in shapes) == 311_650
    rng = np.random.default_rng(311)
    ckpt = [rng.standard_normal(s).astype(F) for s in shapes]
    diffs = [[(rng.standard_normal(s) * m).astype(F) for s in shapes] for m in (1e-3, 1e-2, 1.0)]
    C = 20.0
    s = CO.scales([CO.flat(d) for d in diffs], C)
    assert s[0] == 1 and s[1] == 1 and s[2] < 1
    agg = CycleAggregator(engine)
    ck_pb = build_state_fast(ckpt)
    new = agg.average_plan_diffs({"diff_clip_norm": C}, ck_pb, [build_state_fast(d) for d in diffs])
    want = CO.fedavg_clipped_tensors(ckpt, diffs, C)
    for g, w in zip(parse_state(new), want):
        assert np.array_equal(u32(g), u32(w))
    new2 = agg.average_plan_diffs({}, new, [build_state_fast(d) for d in diffs])
    for g, w in zip(parse_state(new2), O.fedavg_mean(want, diffs)):
        assert np.array_equal(u32(g), u32(w))


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
def test_report_time_close(pinned):
    """IncrementalCycle(clip_norm=) on a 1.11 M-param model with ranged ingest on: the last report
    is the clipped one, the close right behind it; a second cycle chained on the resident checkpoint."""
    from pygrid_amd import Engine
    from pygrid_amd.incremental import IncrementalCycle
    import base64

    from pygrid_amd.report import PinnedPool, b64decode
    from pygrid_amd.state_schema import build_state_fast, parse_state

    shapes = [(1100, 1000), (1000,), (10, 1000), (10,)]
    numel = [int(np.prod(s)) for s in shapes]
    rng = np.random.default_rng(1110)
    ckpt = [rng.standard_normal(s).astype(F) for s in shapes]
    diffs = [[(rng.standard_normal(s) * m).astype(F) for s in shapes] for m in (1e-3, 2e-3, 1e-3, 3e-3, 0.5)]
    C = 50.0
    s = CO.scales([CO.flat(d) for d in diffs], C)
    assert [bool(x < 1) for x in s] == [False, False, False, False, True]
    pbs = [build_state_fast(d) for d in diffs]
    pool = PinnedPool(max_blocks=8) if pinned else None

    def as_report(pb):  # the report handler's path: base64 text decoded into a page-locked block
        return b64decode(base64.b64encode(pb).decode(), into=pool)

    with Engine(0) as eng:
        ck_pb = build_state_fast(ckpt)
        want = ckpt
        for cycle in range(2):
            inc = IncrementalCycle(eng, numel, slots=8, checkpoint=ck_pb, clip_norm=C)
            assert os.environ.get("PGH_INGEST_RANGES", "1") != "0"
            for w in range(6):
                inc.assigned(w)
            for w in (3, 1, 2, 0, 4):  # worker 5 never reports; worker 4 (clipped) reports last
                inc.reported(w, as_report(pbs[w]) if pinned else pbs[w])
            ck_pb = inc.close(ck_pb)
            want = CO.fedavg_clipped_tensors(want, diffs, C)
            for g, w in zip(parse_state(ck_pb), want):
                assert np.array_equal(u32(g), u32(w)), cycle
            assert inc.last_close["clipped"] == 1 and inc.last_close["n"] == 5
            assert inc.last_close["max_norm"] == np.sqrt(CO.row_sumsq(CO.flat(diffs[4])))
    if pool is not None:
        pool.close()


def test_refusals_leave_the_context_usable(engine, fold_case):
    from pygrid_amd import Engine
    from pygrid_amd.exceptions import AggregationError

    ckpt, diffs, c, _ = fold_case
    P = diffs.shape[1]
    mean = O.fedavg_mean([ckpt], [[d] for d in diffs])[0]

    def refused(status, fn, *a):
        with pytest.raises(AggregationError) as e:
            fn(*a)
        assert e.value.status == status, e.value

    def plain_mean_ok(eng):
        load(eng, diffs)
        assert np.array_equal(u32(eng.fedavg(0, ckpt)), u32(mean))

    load(engine, diffs)
    refused(STATE, engine.fedavg, 3, ckpt)  # CLIPPED_MEAN with clipping off
    engine.ckpt_upload(ckpt)
    refused(STATE, engine.fedavg_resident, 3)
    refused(STATE, engine.fold_slots, 3, [0, 1])
    plain_mean_ok(engine)
    refused(UNSUPPORTED, engine.stream_begin, 3)
    plain_mean_ok(engine)
    engine.set_layout([P])
    engine.set_shard(64, P)  # a sub-range shard
    refused(UNSUPPORTED, engine.set_clip_norm, c)
    plain_mean_ok(engine)
    engine.set_layout([P])
    engine.reserve(2, 1, 2)  # an int64 slab
    refused(UNSUPPORTED, engine.set_clip_norm, c)
    plain_mean_ok(engine)
    engine.stream_begin(0)
    refused(UNSUPPORTED, engine.set_clip_norm, c)
    plain_mean_ok(engine)
    with Engine(devices=[0, 0]) as grp:
        grp.set_layout([P])
        grp.reserve(len(diffs))
        refused(UNSUPPORTED, grp.set_clip_norm, c)
        grp.set_clip_norm(0)  # "off" is always accepted
        for k, d in enumerate(diffs):
            grp.ingest(k, d)
        refused(UNSUPPORTED, grp.fedavg, 3, ckpt)
        assert np.array_equal(u32(grp.fedavg(0, ckpt)), u32(mean))
