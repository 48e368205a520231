"""CPU: tests/launch_shapes.py against pygrid_amd/csrc/pgh_variants.def, the table the dispatch
switches of pgh_kernels.hip are generated from, and the cases it derives against the loop regions of
every shape.

A shape added to or changed in the table without launch_shapes.py following fails the first group; a
case list that no longer reaches a loop region of some shape fails the second.  The second group is
what keeps tests/test_gpu_launch_shapes.py honest: it runs exactly the cases checked here.
"""
import re
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import launch_shapes as LS  # noqa: E402

CSRC = Path(__file__).resolve().parent.parent / "pygrid_amd" / "csrc"
NT = {"nt": True, "plain": False}
GRIDS = ("tile", "persistent", "pipelined", "xmap")


def parse_table(text):
    """pgh_variants.def -> (fold shapes by id, ids with a row-table kernel, share-sum shapes of the
    ids that have their own, the share sum's default shape)."""
    fold, tabbed, own, default = {}, set(), {}, []
    rows = re.findall(r"^PGH_(FOLD|SECAGG|SECAGG_DEFAULT)\(([^()]*)\)$", text, re.M)
    assert len(rows) == len(re.findall(r"^PGH_", text, re.M)), "a row of the table was not understood"
    for kind, args in rows:
        f = [x.strip() for x in args.split(",")]
        if kind == "FOLD":
            v, loads, U, W, tb, vec, grid, tab = f
            assert int(v) not in fold and grid in GRIDS
            fold[int(v)] = LS.Shape(int(U), int(W), int(tb), int(vec), NT[loads], grid == "persistent",
                                    grid == "pipelined", grid == "xmap")
            if {"rowtab": True, "no_rowtab": False}[tab]:
                tabbed.add(int(v))
            continue
        v = f.pop(0) if kind == "SECAGG" else None
        loads, U, tb, vec, grid = f
        assert grid in GRIDS[:2]
        sh = LS.Shape(int(U), 1, int(tb), int(vec), NT[loads], grid == "persistent", False, False)
        if v is None:
            default.append(sh)
        else:
            assert int(v) not in own
            own[int(v)] = sh
    assert len(default) == 1
    return fold, tabbed, own, default[0]


@pytest.fixture(scope="module")
def text():
    return (CSRC / "pgh_variants.def").read_text()


def test_fold_table_is_the_def_file(text):
    fold = parse_table(text)[0]
    assert fold == LS.FOLD_SHAPES
    assert list(fold) == list(range(24))  # N_VARIANTS (pgh_kernels.h counts these rows) == 24
    assert len(LS.FOLD_SHAPES) == 24


def test_row_table_is_the_def_file(text):
    fold, tabbed, _, _ = parse_table(text)
    assert {v: fold[v] for v in tabbed} == LS.ROW_SHAPES
    assert tabbed == set(LS.ROW_SHAPES)  # the explicit ids a row-table fold honours
    for v, sh in LS.ROW_SHAPES.items():  # "same shape as the fold variant of that id"
        assert sh == LS.FOLD_SHAPES[v]


def secagg_shapes(text):
    fold, _, own, default = parse_table(text)
    return {v: own.get(v, default) for v in fold}, {v for v in fold if v not in own}


def test_secagg_table_is_the_def_file(text):
    shapes, defaulted = secagg_shapes(text)
    assert shapes == LS.SECAGG_SHAPES
    assert defaulted == set(LS.SECAGG_DEFAULT_IDS)


def test_a_changed_template_argument_is_noticed(text):
    """The parser reads the arguments, not just the ids: one edited number or flag changes its result."""
    edited = text.replace("PGH_FOLD(17, nt, 64, 1, 64, 1,", "PGH_FOLD(17, nt, 32, 1, 64, 1,")
    assert edited != text and parse_table(edited)[0] != LS.FOLD_SHAPES
    edited = text.replace("PGH_SECAGG(16, nt, 48, 64, 1,", "PGH_SECAGG(16, nt, 48, 64, 2,")
    assert edited != text and secagg_shapes(edited)[0] != LS.SECAGG_SHAPES
    edited = text.replace("PGH_FOLD(14, nt, 32, 1, 64, 1, tile, rowtab)", "PGH_FOLD(14, nt, 32, 1, 64, 1, tile, no_rowtab)")
    assert edited != text and parse_table(edited)[1] != set(LS.ROW_SHAPES)


def test_no_hand_written_case_beside_the_table():
    """The switches over variant ids come from the table: the source has no `case <n>: return go_fedavg...`
    or `go_secagg...` line.  (K8's switch over the trim depth, `return go_trim<b, VEC>`, is no variant id.)"""
    assert not re.search(r"case\s+\d+\s*:\s*return\s+go_(?!trim<)", (CSRC / "pgh_kernels.hip").read_text())


def test_region_arithmetic_on_known_launches():
    """regions() on launches worked out by hand from the kernels."""
    s17, s21, s1 = LS.FOLD_SHAPES[17], LS.FOLD_SHAPES[21], LS.FOLD_SHAPES[1]
    # id 17 (U = 64), FIRST: row 0 seeds the accumulator, 64 rows are left at N = 65
    assert LS.regions(s17, 64, 163, True)[:2] == (0, 63)
    assert LS.regions(s17, 65, 163, True)[:2] == (1, 0)
    assert LS.regions(s17, 64, 163, False)[:2] == (1, 0)
    assert LS.regions(s17, 163, 163, True)[3:5] == (2, 35)  # 163 columns in tiles of 64
    # id 21 (U = 8): buffer A is loaded inside the loop from 1 + 3U rows on
    assert LS.regions(s21, 24, 2563, True).a_reloads == 0
    assert LS.regions(s21, 25, 2563, True).a_reloads == 1
    assert LS.regions(s21, 24, 2563, False).a_reloads == 1
    assert LS.regions(s21, 41, 2563, True).a_reloads == 2
    # id 1: 1,024 workgroups on 256 CUs, a tile is 1,024 params
    assert LS.regions(s1, 3, 1024 * 1024, True).trips == 1
    assert LS.regions(s1, 3, 1024 * 1024 + 1, True).trips == 2
    assert LS.regions(s1, 3, LS.persistent_P(256), True).trips == 3
    assert LS.regions(LS.FOLD_SHAPES[0], 3, LS.persistent_P(256), True).trips == 1
    # the share sum starts at r = 0 whatever the flags; columns of 2 int64
    assert LS.regions(LS.SECAGG_SHAPES[3], 8, 1281, True, secagg=True)[:5] == (1, 0, 0, 2, 129)
    # STREAM: ring of 8, batch 8, 18 clients -> 8 FIRST, 8 middle, 2 FINAL; ring of 9: 9, 9, 0 FINAL
    L = LS.Launch
    assert LS.stream_launches(18, 8, 8) == [L(8, True, False), L(8, False, False), L(2, False, True)]
    assert LS.stream_launches(18, 9, 9) == [L(9, True, False), L(9, False, False), L(0, False, True)]
    # a run that wraps the ring is two launches (ring of 5, batch 2: clients 4-5 sit in slots 4 and 0)
    assert LS.stream_launches(6, 5, 2)[2:4] == [L(1, False, False), L(1, False, False)]
    assert LS.stream_launches(3, 1, 1, rows_per_client=3) == [L(3, True, False), L(3, False, False), L(3, False, False),
                                                              L(0, False, True)]


def check_walk_regions(visits, sh, residues):
    regs = [r for _, r in visits]
    assert any(r.full_batches >= 2 for r in regs), "no launch runs the full-batch loop twice"
    assert any(r.full_batches >= 1 and r.remainder > 0 for r in regs), "no full batch followed by a remainder"
    assert any(r.full_batches == 0 and r.remainder > 0 for r in regs), "no launch with a remainder only"
    assert any(r.full_batches >= 1 and r.remainder == 0 for r in regs), "no launch ends on a batch boundary"
    assert any(r.full_tiles >= 2 and r.partial_tile > 0 for r in regs), "no launch with two full tiles and a partial one"
    assert {P % residues for P, _ in visits} == set(range(residues)), "a residue of P is missing"
    if sh.pipelined:
        assert any(r.a_reloads >= 1 for r in regs), "buffer A is never loaded inside the loop"
    if sh.persistent:
        assert any(r.trips >= 2 for r in regs), "the persistent grid never takes a second trip"
    else:
        assert all(r.trips == 1 for r in regs)


@pytest.mark.parametrize("mode", LS.MODES)
@pytest.mark.parametrize("vid", sorted(LS.FOLD_SHAPES))
def test_fold_cases_visit_every_region(vid, mode):
    # (the cases, and so the regions, are the same for the three modes: each is run in all of them)
    sh = LS.FOLD_SHAPES[vid]
    check_walk_regions(LS.fold_visits(sh), sh, 4)
    # a continuation launch (not FIRST) that takes a full batch from r = 0, one that is neither FIRST
    # nor FINAL, and every stream case with its three kinds of launch
    for N, P, R, batch in LS.stream_cases(sh):
        ls = LS.stream_launches(N, R, batch)
        assert ls[0].first and not ls[0].final and ls[-1].final and not ls[-1].first
        assert any(not l.first and not l.final for l in ls)
        assert any(not l.first and LS.regions(sh, l.n_rows, P, False).full_batches >= 1 for l in ls)
        assert sum(l.n_rows for l in ls) == N
    assert {P % 4 for _, P, _, _ in LS.stream_cases(sh)} == {1, 3}
    assert max(N for N, _ in LS.fold_cases(sh)) <= 194 and max(P for _, P in LS.fold_cases(sh)) <= 10_243


@pytest.mark.parametrize("mode", LS.MODES)
@pytest.mark.parametrize("vid", sorted(LS.ROW_SHAPES))
def test_row_cases_visit_every_region(vid, mode):
    sh = LS.ROW_SHAPES[vid]
    check_walk_regions(LS.row_visits(sh), sh, 4)
    for N, P, a in LS.row_cases(sh):
        assert a % sh.U and (N - a) % sh.U and 0 < a < N <= LS.ROWTAB_MAX
    assert {N for N, _, _ in LS.row_cases(sh)} >= {sh.U + 1, 2 * sh.U + 2}


@pytest.mark.parametrize("vid", sorted(LS.SECAGG_SHAPES))
def test_secagg_cases_visit_every_region(vid):
    sh = LS.SECAGG_SHAPES[vid]
    check_walk_regions(LS.secagg_visits(sh), sh, 2)
    cases = LS.secagg_cases(sh)
    assert {S for _, S, _, _ in cases} == {1, 3}
    assert {N * S for N, S, _, _ in cases} <= {sh.U, sh.U + 1, 2 * sh.U + 1, 2 * sh.U + 2}
    for N, S, P, batch in cases:
        ls = LS.stream_launches(N, batch, batch, rows_per_client=S)
        assert any(not l.first and not l.final and l.n_rows > 0 for l in ls), "no launch reads and writes acc"
        assert ls[-1].final and sum(l.n_rows for l in ls) == N * S


def test_persistent_cases_take_a_second_trip():
    for cu in (64, 256, 304):
        for v in (1, 3, 5):
            assert LS.regions(LS.FOLD_SHAPES[v], LS.PERSISTENT_N, LS.persistent_P(cu), True, cu).trips >= 2
            r = LS.regions(LS.SECAGG_SHAPES[v], LS.PERSISTENT_N, LS.persistent_P(cu, secagg=True), True, cu, secagg=True)
            assert r.trips >= 2 and LS.persistent_P(cu, secagg=True) % 2 == 1
    assert [v for v, sh in LS.FOLD_SHAPES.items() if sh.persistent] == [1, 3, 5]
    assert [v for v, sh in LS.SECAGG_SHAPES.items() if sh.persistent] == [1, 3, 5]
