"""GPU: every launch shape of the column walk through all of its loop regions -- the full-batch
loop, the masked last batch, the grid-stride trip -- bit for bit against the CPU oracles.

The cases come from tests/launch_shapes.py; tests/test_launch_shape_table.py (CPU) holds that
helper against the dispatch switches of pgh_kernels.hip and checks that the cases reach every
region of every shape.  Outputs are prefilled (NaN, or a marker for int64 sums), so a column that a
kernel leaves unwritten shows as a difference.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import launch_shapes as LS  # noqa: E402
from oracle import coracle  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SECAGG = 16  # STREAM_SECAGG
I64 = 1
MARK = -0x0123456789ABCDEF  # prefill of an int64 sum


def u32(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def check_f32(got, want, what):
    """Bit-equal, position by position (the inputs are finite: a NaN is an unwritten param)."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(u32(got) != u32(want))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} params differ, the first at {bad[0]} "
                           f"(got {got[bad[0]]!r}, want {want[bad[0]]!r}), the last at {bad[-1]}")


def check_i64(got, want, what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} sums differ, the first at {bad[0]}, the last at {bad[-1]}"


def inputs(rng, N, P):
    d = (rng.standard_normal((N, P), dtype=F) * F(1e-2)).astype(F)
    c = rng.standard_normal(P, dtype=F)
    w = rng.uniform(0.5, 2.0, N).astype(F)
    return d, c, w


def fold_device(engine, mode, ck, P):
    """One resident fold into a NaN-filled device vector."""
    import torch

    out = torch.full((P,), float("nan"), dtype=torch.float32, device="cuda")
    engine.fedavg_device(mode, ck.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture
def variant(engine):
    """set_variant for the test, the auto choice back afterwards."""
    yield engine.set_variant
    engine.set_variant(-1)


@pytest.fixture(scope="module")
def cu_count(engine):
    import torch

    return int(torch.cuda.get_device_properties(engine.device).multi_processor_count)


@pytest.mark.parametrize("vid", sorted(LS.FOLD_SHAPES))
def test_fold_every_region(engine, variant, vid):
    """fp32 folds in one launch: N over {U, U+1, U+2, 2U, 2U+1, 2U+2, 3U+1, 3U+2} at P = 2.5 tiles
    + 3, the other residues of P at N = 2U + 2; modes 0, 1, 2.  The rows of a layout are ingested
    once, the folds take growing prefixes."""
    import torch

    sh = LS.FOLD_SHAPES[vid]
    rng = np.random.default_rng(7000 + vid)
    variant(vid)
    by_P = {}
    for N, P in LS.fold_cases(sh):
        by_P.setdefault(P, []).append(N)
    for P, Ns in by_P.items():
        d, c, w = inputs(rng, max(Ns), P)
        engine.set_layout([P])
        engine.reserve(max(Ns))
        engine.set_weights(w)
        ck = torch.from_numpy(c).cuda()
        have = 0
        for N in sorted(Ns):
            for k in range(have, N):
                engine.ingest(k, d[k])
            have = N
            for mode in LS.MODES:
                assert engine.effective_variant(mode) == vid
                got = fold_device(engine, mode, ck, P)
                want = coracle.fedavg(mode, d[:N], c, w[:N] if mode == 2 else None)
                check_f32(got, want, f"variant {vid} mode {mode} N {N} P {P}")


@pytest.mark.parametrize("vid", sorted(LS.FOLD_SHAPES))
def test_fold_continuation_launches(engine, variant, vid):
    """The same shape over a FIRST, a middle and a FINAL launch (STREAM ring): the launches that are
    not FIRST read the running state, those that are not FINAL write it, through the ragged last
    column (P mod 4 = 1 and 3); one of them takes a full batch of U rows from r = 0.  Bit-equal to
    the oracle and to the fold in one launch."""
    import torch

    sh = LS.FOLD_SHAPES[vid]
    rng = np.random.default_rng(8000 + vid)
    variant(vid)
    for N, P, R, batch in LS.stream_cases(sh):
        d, c, w = inputs(rng, N, P)
        ck = torch.from_numpy(c).cuda()
        engine.set_layout([P])
        engine.reserve(N)
        engine.set_weights(w)
        for k in range(N):
            engine.ingest(k, d[k])
        single = {mode: fold_device(engine, mode, ck, P) for mode in LS.MODES}
        engine.reserve(R)
        launches = LS.stream_launches(N, R, batch)
        for mode in LS.MODES:
            what = f"variant {vid} mode {mode} N {N} P {P} ring {R} batch {batch}"
            engine.reset_stats()
            engine.stream_begin(mode, batch)
            if mode == 2:
                engine.set_weights(w)
            assert engine.effective_variant(mode) == vid
            for k in range(N):
                engine.ingest(k, d[k])
            out = torch.full((P,), float("nan"), dtype=torch.float32, device="cuda")
            engine.stream_finish_device(ck.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            st = engine.stats()
            assert st["n_folded"] == N and st["kernel_launches"] == len(launches), what
            got = out.cpu().numpy()
            check_f32(got, coracle.fedavg(mode, d, c, w if mode == 2 else None), what)
            check_f32(got, single[mode], what + " against the single launch")


@pytest.mark.parametrize("vid", [1, 3, 5])
def test_fold_persistent_second_trip(engine, variant, cu_count, vid):
    """A persistent grid (4 workgroups per CU) over more than twice as many tiles as it has
    workgroups: the grid-stride step of fedavg_tiles runs, twice for the first workgroups.  Every
    param of the three modes."""
    import torch

    sh = LS.FOLD_SHAPES[vid]
    N, P = LS.PERSISTENT_N, LS.persistent_P(cu_count)
    reg = LS.regions(sh, N, P, True, cu_count)
    if reg.trips < 2:
        pytest.fail(f"variant {vid}: P = {P} on {cu_count} CUs takes {reg.trips} trip(s), not two")
    rng = np.random.default_rng(9000 + vid)
    d, c, w = inputs(rng, N, P)
    variant(vid)
    engine.set_layout([P])
    engine.reserve(N)
    engine.set_weights(w)
    for k in range(N):
        engine.ingest(k, d[k])
    ck = torch.from_numpy(c).cuda()
    try:
        for mode in LS.MODES:
            assert engine.effective_variant(mode) == vid
            got = fold_device(engine, mode, ck, P)
            check_f32(got, coracle.fedavg(mode, d, c, w if mode == 2 else None), f"variant {vid} mode {mode} N {N} P {P}")
    finally:
        engine.set_layout([1])  # release the slab


def poison_resident_buffers(engine, P):
    """NaN in both of the context's checkpoint buffers (the fold of a zero diff into a NaN
    checkpoint, then the swap): what the next finish does not write stays NaN."""
    engine.ckpt_upload(np.full(P, np.nan, F))
    engine.ingest(0, np.zeros(P, F))
    engine.fold_slots_finish_resident(0, [0])


@pytest.mark.parametrize("vid", sorted(LS.ROW_SHAPES))
def test_row_table_shapes(engine, variant, vid):
    """The row-table kernels with the shape set explicitly: the rows sit in a shuffled subset of a
    larger slot range, a first part goes to fold_slots and the rest to fold_slots_finish_resident,
    neither part a multiple of U.  Against the oracle's fold in the given order."""
    sh = LS.ROW_SHAPES[vid]
    rng = np.random.default_rng(10_000 + vid)
    variant(vid)
    for N, P, a in LS.row_cases(sh):
        d, c, w = inputs(rng, N, P)
        n_slots = N + N // 2 + 3
        engine.set_layout([P])
        engine.reserve(n_slots)
        for mode in LS.MODES:
            slot_of = rng.permutation(n_slots)[:N].astype(np.int32)
            poison_resident_buffers(engine, P)
            engine.ckpt_upload(c)
            for k in range(N):
                engine.ingest(int(slot_of[k]), d[k])
            if mode == 2:
                engine.set_weights(w)
            assert engine.effective_variant(mode) == vid
            engine.fold_slots(mode, slot_of[:a])
            engine.fold_slots_finish_resident(mode, slot_of[a:])
            want = coracle.fedavg(mode, d, c, w if mode == 2 else None)
            check_f32(engine.ckpt_download(), want, f"row variant {vid} mode {mode} N {N} = {a} + {N - a} P {P}")


def full_range_shares(rng, N, S, P):
    return rng.integers(-2**63, 2**63 - 1, size=(N, S, P), dtype=np.int64, endpoint=True)


def secagg_outputs(P):
    import torch

    return (torch.full((P,), MARK, dtype=torch.int64, device="cuda"),
            torch.full((P,), float("nan"), dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("vid", sorted(LS.SECAGG_SHAPES))
def test_secagg_every_region(engine, variant, vid):
    """Share sums over the full int64 range (they wrap): N x S rows in {U, U+1, 2U+1, 2U+2}, S in
    {1, 3}, P even and odd; in one launch and through a ring whose middle launch reads and writes
    the running sums."""
    import torch

    sh = LS.SECAGG_SHAPES[vid]
    rng = np.random.default_rng(11_000 + vid)
    variant(vid)
    for N, S, P, batch in LS.secagg_cases(sh):
        what = f"secagg variant {vid} N {N} S {S} P {P}"
        shares = full_range_shares(rng, N, S, P)
        want_s = O.secagg_sum(shares)
        want_d = O.fix_prec_decode(want_s)
        engine.set_layout([P])
        engine.reserve(N, I64, S)
        for k in range(N):
            engine.ingest(k, shares[k])
        assert engine.effective_variant(SECAGG) == vid
        s, dec = secagg_outputs(P)
        engine.secagg_device(s.data_ptr(), dec.data_ptr())
        torch.cuda.synchronize()
        check_i64(s.cpu().numpy(), want_s, what)
        check_f32(dec.cpu().numpy(), want_d, what + " decode")
        # the ring: R = batch clients, so every batch is one launch
        engine.reserve(batch, I64, S)
        engine.reset_stats()
        engine.stream_begin(SECAGG, batch)
        assert engine.effective_variant(SECAGG) == vid
        for k in range(N):
            engine.ingest(k, shares[k])
        s, dec = secagg_outputs(P)
        engine.stream_finish_secagg_device(s.data_ptr(), dec.data_ptr())
        torch.cuda.synchronize()
        what += f" ring of {batch}"
        assert engine.stats()["kernel_launches"] == len(LS.stream_launches(N, batch, batch, rows_per_client=S)), what
        check_i64(s.cpu().numpy(), want_s, what)
        check_f32(dec.cpu().numpy(), want_d, what + " decode")


@pytest.mark.parametrize("vid", [1, 3, 5])
def test_secagg_persistent_second_trip(engine, variant, cu_count, vid):
    """The persistent share-sum grids past their second grid-stride step, P odd."""
    import torch

    sh = LS.SECAGG_SHAPES[vid]
    N, S, P = LS.PERSISTENT_N, 1, LS.persistent_P(cu_count, secagg=True)
    reg = LS.regions(sh, N * S, P, True, cu_count, secagg=True)
    if reg.trips < 2 or P % 2 == 0:
        pytest.fail(f"secagg variant {vid}: P = {P} on {cu_count} CUs takes {reg.trips} trip(s), not two")
    rng = np.random.default_rng(12_000 + vid)
    shares = full_range_shares(rng, N, S, P)
    want_s = O.secagg_sum(shares)
    variant(vid)
    engine.set_layout([P])
    engine.reserve(N, I64, S)
    for k in range(N):
        engine.ingest(k, shares[k])
    assert engine.effective_variant(SECAGG) == vid
    s, dec = secagg_outputs(P)
    engine.secagg_device(s.data_ptr(), dec.data_ptr())
    torch.cuda.synchronize()
    what = f"secagg variant {vid} N {N} S {S} P {P}"
    check_i64(s.cpu().numpy(), want_s, what)
    check_f32(dec.cpu().numpy(), O.fix_prec_decode(want_s), what + " decode")
    engine.set_layout([1])
