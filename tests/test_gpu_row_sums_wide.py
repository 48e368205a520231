"""GPU: the row sums (K7, K12) and the closes that rest on them where a row has more tile partials than one
chunk of ``k_row_sumsq_fold`` (1,024: ``clip_oracle.FOLD_CHUNK``), so that the chunk loop runs a second and a
third time: the LDS buffer filled again behind the second barrier, a short last chunk, the sum carried from chunk
to chunk by one lane.  The widths are ``gen_clip_golden.WIDE_P`` and no others (clip_oracle's docstring names
them); the rows are ``gen_clip_golden.wide_rows``, which tests/test_row_sums_wide.py shows on the CPU to give
other u64 bits under every wrong chunking, so a bit-equal sum here is not an accident.  Sums as u64 against
tests/clip_oracle.py, tests/geomed_oracle.py and tests/golden/row_sums_wide.npz; closes as u32.

The closes run at ``P_B``: 16.8 MB a row, so a report goes to HBM in three 8 MiB ingest ranges and a row-wise
close waits behind more than one of them."""
import base64
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clip_oracle as CO  # noqa: E402
import gen_clip_golden as GG  # noqa: E402
import gen_row_sums_wide_golden as GW  # noqa: E402
import geomed_oracle as GO  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
CLIPPED, GEOMED = 3, 6
N = GG.WIDE_N
SMALL_P = 4097
SCATTERED, CAP = [6, 1, 7, 3, 4], 8  # no run of consecutive slots: the row table
CONSECUTIVE = list(range(N))
P_A, P_B, P_C = GG.WIDE_P
CLIP_C = 1e5
ITERS, NU = 2, 1e-6
CUT = 2_000_004  # a multiple of 4, not of a tile
assert CUT % 4 == 0 and CUT % CO.TILE and CUT < P_B


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def G():
    return np.load(GW.GOLDEN)


@pytest.fixture(scope="module")
def small():
    """The 4,097-param rows of the clip golden file and their pinned sums."""
    g = np.load(GG.GOLDEN)
    return g[f"rows_{SMALL_P}"], g[f"sumsq_bits_{SMALL_P}"]


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_clip_norm(0)
    engine.set_geomed(0)


def load(eng, rows, slots=None, cap=None):
    eng.set_layout([rows.shape[1]])
    eng.reserve(cap or len(rows))
    for k, d in enumerate(rows):
        eng.ingest(k if slots is None else int(slots[k]), d)


@functools.lru_cache(maxsize=None)
def ckpt_of(p):
    c = np.random.default_rng(92000 + p).standard_normal(p).astype(F)
    c.setflags(write=False)
    return c


# ---- K7 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", GG.WIDE_P)
def test_row_sumsq_past_one_fold_chunk(engine, G, small, p):
    """One context: the small layout, the wide one (scattered slots, then slots 0..4), the small one again --
    the partial buffer is ``slots x ntiles`` and allocated once per slab, so it has to follow the layout."""
    rows, want = GG.wide_rows(p), GW.wide_sums(p)
    assert np.array_equal(u64(want), G[f"sumsq_bits_{p}"])  # the oracle of today is the oracle of the golden file
    assert want[GG.SENTINEL] == GG.sentinel_sumsq(p)
    other, other_sum = GG.wide_other(p), GW.other_sum(p)
    assert u64([other_sum])[0] == G[f"other_bits_{p}"][0]
    srows, sbits = small

    def small_layout():
        load(engine, srows, [5, 2, 7], cap=CAP)
        assert np.array_equal(u64(engine.row_sumsq([5, 2, 7])), sbits)

    small_layout()
    for slots, cap in ((SCATTERED, CAP), (CONSECUTIVE, N)):
        load(engine, rows, slots, cap)
        got = engine.row_sumsq(slots)
        assert np.array_equal(u64(got), u64(want)), (p, slots, got, want)
        assert got[GG.SENTINEL] == GG.sentinel_sumsq(p)
        # another diff into one slot: its sum changes, the others stay
        engine.ingest(slots[2], other)
        got = engine.row_sumsq(slots[::-1])[::-1]
        expect = np.array(want)
        expect[2] = other_sum
        assert np.array_equal(u64(got), u64(expect)), (p, slots, got, expect)
    small_layout()


# ---- K12 --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [P_B, P_C])
def test_row_distsq_past_one_fold_chunk(engine, p):
    rows, sums = GG.wide_rows(p), GW.wide_sums(p)
    points = {"random": np.random.default_rng(93000 + p).standard_normal(p).astype(F), "zero": np.zeros(p, F),
              "row": rows[2].copy()}
    want = {k: u64([GO.row_distsq(r, points[k]) for r in rows]) for k in ("random", "row")}
    want["zero"] = u64(sums)  # (GO.row_distsq against zeros is CO.row_sumsq of the row: x - 0 is x)
    assert want["row"][2] == 0 and len(set(want["random"].tolist())) == N
    for slots, cap in ((CONSECUTIVE, N), (SCATTERED, CAP)):
        load(engine, rows, slots, cap)
        k7 = engine.row_sumsq(slots)
        assert np.array_equal(u64(k7), u64(sums))
        for k, pt in points.items():
            got = engine.row_distsq(slots, pt)
            assert np.array_equal(u64(got), want[k]), (p, slots, k, got)
        assert u64(engine.row_distsq(slots, rows[2]))[2] == 0  # +0.0, not -0.0
        # the tile partials are shared: K7's sums afterwards, cached ...
        assert np.array_equal(u64(engine.row_sumsq(slots)), u64(sums))
        # ... and computed again over the partials K12 left
        engine.ingest(slots[0], rows[0])
        engine.ingest(slots[4], rows[4])
        assert np.array_equal(u64(engine.row_sumsq(slots)), u64(sums))


# ---- the closes at P_B ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def clip_case():
    """(scales, the new checkpoint) of the five rows under CLIP_C, from the oracle: three rows clipped, two not."""
    rows = GG.wide_rows(P_B)
    s = np.array([CO.scale(x, CLIP_C) for x in GW.wide_sums(P_B)], F)
    # a condition on the inputs: rows 0, 2 and the sparse row are clipped, rows 1 and 3 are left alone
    assert [bool(x < 1) for x in s] == [True, False, True, False, True]
    want = CO.flat(CO.fedavg_clipped_tensors(tensors(ckpt_of(P_B)), [tensors(r) for r in rows], CLIP_C))
    assert np.array_equal(u32(want), u32(CO.fold(rows, s, ckpt_of(P_B))))
    return s, want


def test_clipped_close_every_entry_point(eng):
    import torch

    p, rows, ckpt = P_B, GG.wide_rows(P_B), ckpt_of(P_B)
    _, want = clip_case()
    max_norm = np.sqrt(GW.wide_sums(p).max())
    eng.set_layout([p])
    eng.reserve(N)
    eng.set_clip_norm(CLIP_C)  # the bound first: every ingest queues its row's K7 behind the copy
    for k, d in enumerate(rows):
        eng.ingest(k, d)
    assert np.array_equal(u32(eng.fedavg(CLIPPED, ckpt)), u32(want))
    st = eng.clip_stats()
    assert st["rows"] == N and st["clipped"] == 3 and st["max_norm"] == max_norm
    eng.ckpt_upload(ckpt)
    eng.fedavg_resident(CLIPPED)
    assert np.array_equal(u32(eng.ckpt_download()), u32(want))
    ck = torch.from_numpy(np.array(ckpt)).cuda()
    out = torch.zeros_like(ck)
    eng.fedavg_device_range(CLIPPED, 0, CUT, ck.data_ptr(), out.data_ptr())
    eng.fedavg_device_range(CLIPPED, CUT, p - CUT, ck.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(u32(out.cpu().numpy()), u32(want))
    # scattered slots, the bound set after the ingests: the sums are computed at the fold
    eng.set_clip_norm(0)
    load(eng, rows, SCATTERED, CAP)
    eng.set_clip_norm(CLIP_C)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(CLIPPED, SCATTERED)
    assert np.array_equal(u32(eng.ckpt_download()), u32(want))
    st = eng.clip_stats()
    assert st["rows"] == N and st["clipped"] == 3 and st["max_norm"] == max_norm == np.sqrt(GG.sentinel_sumsq(p))


@functools.lru_cache(maxsize=None)
def geomed_case():
    g = GO.geomed(GG.wide_rows(P_B), ITERS, NU)
    assert g["excluded"] == 0
    return g


def geomed_stats_are(eng, g, excluded):
    st = eng.geomed_stats()
    assert st["iterations"] == ITERS and st["rows"] == N and st["excluded"] == excluded == g["excluded"]
    assert u64([st["objective"]])[0] == u64([g["objective"]])[0], (st, g["objective"])
    assert u32([st["max_weight"]])[0] == u32([g["max_weight"]])[0], (st, g["max_weight"])


def test_geomed_close_every_entry_point(eng):
    import torch

    p, rows, ckpt = P_B, GG.wide_rows(P_B), ckpt_of(P_B)
    g = geomed_case()
    want = (ckpt - g["v"]).astype(F)
    load(eng, rows)
    eng.set_geomed(ITERS, NU)
    assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want))
    geomed_stats_are(eng, g, 0)
    eng.ckpt_upload(ckpt)
    eng.fedavg_resident(GEOMED)
    assert np.array_equal(u32(eng.ckpt_download()), u32(want))
    ck = torch.from_numpy(np.array(ckpt)).cuda()
    out = torch.zeros_like(ck)
    eng.fedavg_device_range(GEOMED, 0, CUT, ck.data_ptr(), out.data_ptr())
    eng.fedavg_device_range(GEOMED, CUT, p - CUT, ck.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(u32(out.cpu().numpy()), u32(want))
    eng.set_layout([p])  # (a new layout clears the setting)
    eng.reserve(CAP)
    eng.set_geomed(ITERS, NU)  # the rule first: every ingest queues its row's K7
    for k, d in enumerate(rows):
        eng.ingest(SCATTERED[k], d)
    eng.ckpt_upload(ckpt)
    eng.fold_slots_finish_resident(GEOMED, SCATTERED)
    assert np.array_equal(u32(eng.ckpt_download()), u32(want))
    geomed_stats_are(eng, g, 0)


def test_geomed_excludes_a_row_that_is_infinite_in_its_last_tile_only(eng):
    """P_B's last tile is one param, alone with one other tile in the fold's last chunk: the infinity has to come
    through that chunk into the row's sum for the row to be left out."""
    p, ckpt = P_B, ckpt_of(P_B)
    rows = np.array(GG.wide_rows(p))
    rows[1, p - 1] = np.inf
    assert np.isfinite(rows[1, :p - 1]).all() and (p - 1) // CO.TILE == GG.n_tiles(p) - 1
    g = GO.geomed(rows, ITERS, NU)
    assert g["excluded"] == 1 and g["included"] == [0, 2, 3, 4]
    want = (ckpt - g["v"]).astype(F)
    assert np.isfinite(want).all()
    load(eng, rows)
    eng.set_geomed(ITERS, NU)
    sums = eng.row_sumsq(CONSECUTIVE)
    assert np.isposinf(sums[1]) and np.array_equal(u64(sums[[0, 2, 3, 4]]), u64(GW.wide_sums(p)[[0, 2, 3, 4]]))
    assert np.array_equal(u32(eng.fedavg(GEOMED, ckpt)), u32(want))
    geomed_stats_are(eng, g, 1)


# ---- report time: the close behind an ingest of three ranges ----------------------------------------------------------

SHAPES = [(2048, 2048), (4000,), (9, 10), (7,)]
assert sum(int(np.prod(s)) for s in SHAPES) == P_B


def tensors(flat):
    out, off = [], 0
    for s in SHAPES:
        n = int(np.prod(s))
        out.append(np.asarray(flat[off:off + n]).reshape(s))
        off += n
    return out


@functools.lru_cache(maxsize=None)
def report_bytes():
    """State bytes of the checkpoint, of the five rows and of the diff worker 2 sends first (cached, shared)."""
    from pygrid_amd.state_schema import build_state_fast

    rows = GG.wide_rows(P_B)
    return (build_state_fast(tensors(ckpt_of(P_B))), [build_state_fast(tensors(r)) for r in rows],
            build_state_fast(tensors(GG.wide_other(P_B))))


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
@pytest.mark.parametrize("rule", ["clip", "geomed"])
def test_report_time_close_behind_three_ingest_ranges(eng, rule, pinned):
    """IncrementalCycle on a model of P_B params in four tensors: the sparse row -- clipped hardest, farthest out
    -- reports last with the close right behind it, worker 5 never reports, worker 2 reports another diff first
    and then its own into the same slot; a second cycle chained on the resident checkpoint."""
    from pygrid_amd.incremental import IncrementalCycle
    from pygrid_amd.report import PinnedPool, b64decode
    from pygrid_amd.settings import settings_of
    from pygrid_amd.state_schema import parse_state

    assert os.environ.get("PGH_INGEST_RANGES", "1") != "0" and 4 * P_B > 2 * (8 << 20)
    numel = [int(np.prod(s)) for s in SHAPES]
    rows = GG.wide_rows(P_B)
    ck_pb, pbs, other_pb = report_bytes()
    if rule == "clip":
        s, want = clip_case()  # (CO.fedavg_clipped_tensors over the four tensors)
        wants = [want, CO.fold(rows, s, want)]
        kw = dict(clip_norm=CLIP_C)
    else:
        g = geomed_case()
        want = (ckpt_of(P_B) - g["v"]).astype(F)
        wants = [want, (want - g["v"]).astype(F)]
        kw = dict(settings=settings_of({"diff_geometric_median": {"iterations": ITERS}}))
    pool = PinnedPool(max_blocks=8) if pinned else None

    def as_report(pb):  # the report handler's path: base64 text decoded into a page-locked block
        return b64decode(base64.b64encode(pb).decode(), into=pool) if pinned else pb

    try:
        for cycle in range(2):
            inc = IncrementalCycle(eng, numel, slots=CAP, checkpoint=ck_pb, **kw)
            for w in range(6):
                inc.assigned(w)
            for w in (3, 1, 2, 0):
                inc.reported(w, as_report(other_pb if w == 2 else pbs[w]))
            inc.reported(2, as_report(pbs[2]))
            inc.reported(GG.SENTINEL, as_report(pbs[GG.SENTINEL]))
            ck_pb = inc.close(ck_pb)
            assert np.array_equal(u32(CO.flat(parse_state(ck_pb))), u32(wants[cycle])), (rule, cycle)
            lc = inc.last_close
            assert lc["n"] == N and lc["early"] == 0 and not lc["refold"]
            if rule == "clip":
                assert lc["clipped"] == 3 and lc["max_norm"] == np.sqrt(GG.sentinel_sumsq(P_B))
            else:
                st = eng.geomed_stats()
                assert lc["geometric_median"] == {"iterations": ITERS, "excluded": 0, "objective": st["objective"],
                                                  "max_weight": st["max_weight"]}
                geomed_stats_are(eng, g, 0)
    finally:
        if pool is not None:
            pool.close()
