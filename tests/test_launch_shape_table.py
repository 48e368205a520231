"""CPU: tests/launch_shapes.py against the dispatch switches of pygrid_amd/csrc/pgh_kernels.hip, and
the cases it derives against the loop regions of every shape.

A shape added to or changed in the source without the tables following fails the first group; a
case list that no longer reaches a loop region of some shape fails the second.  The second group is
what keeps tests/test_gpu_launch_shapes.py honest: it runs exactly the cases checked here.
"""
import re
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import launch_shapes as LS  # noqa: E402

SRC = Path(__file__).resolve().parent.parent / "pygrid_amd" / "csrc" / "pgh_kernels.hip"
B = {"true": True, "false": False}


def body_of(text, signature):
    """The braces' contents of the one function whose definition starts with `signature`."""
    assert text.count(signature) == 1, signature
    i = text.index("{", text.index(signature))
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
        j += 1


def parse_fold(text):
    body = body_of(text, "hipError_t dispatch_fedavg(const FedavgArgs& a, int variant, hipStream_t s)")
    out = {}
    for m in re.finditer(r"case (\d+): return go_fedavg<MODE, (\d+), (\d+), (true|false), (\d+), (\d+)"
                         r"(?:, (true|false))?>\(a, (true|false), s\);", body):
        v, U, W, nt, tb, vec, xmap, pers = m.groups()
        assert int(v) not in out
        out[int(v)] = LS.Shape(int(U), int(W), int(tb), int(vec), B[nt], B[pers], False, B[xmap or "false"])
    for m in re.finditer(r"case (\d+): return go_fedavg_pipe<MODE, (\d+), (\d+), (\d+)>\(a, s\);", body):
        v, U, tb, vec = m.groups()
        assert int(v) not in out
        out[int(v)] = LS.Shape(int(U), 1, int(tb), int(vec), True, False, True, False)
    assert len(out) == len(re.findall(r"\bcase\b", body)), "a case of dispatch_fedavg was not understood"
    assert "default: return hipErrorInvalidValue;" in body
    return out


def parse_rows(text):
    body = body_of(text, "hipError_t dispatch_fedavg_rows(const FedavgArgs& a, const RowTab& t, int variant, hipStream_t s)")
    out = {}
    for m in re.finditer(r"(case (\d+)|default): return go_fedavg_rows<MODE, (\d+), (\d+), (true|false), (\d+), (\d+)>"
                         r"\(a, t, s\);", body):
        _, v, U, W, nt, tb, vec = m.groups()
        v = 0 if v is None else int(v)  # the default is the shape of variant 0
        assert v not in out
        out[v] = LS.Shape(int(U), int(W), int(tb), int(vec), B[nt], False, False, False)
    assert len(out) == len(re.findall(r"\b(?:case|default)\b", body)), "a case of dispatch_fedavg_rows was not understood"
    return out


def parse_rows_honoured(text):
    body = body_of(text, "hipError_t launch_fedavg_rows(const FedavgArgs& a_, const RowTab& t, hipStream_t s)")
    line = next(ln for ln in body.splitlines() if "v = a.variant" in ln)
    return {int(v) for v in re.findall(r"a\.variant == (\d+)", line)}


def parse_secagg(text):
    body = body_of(text, "hipError_t launch_secagg(const SecaggArgs& a, hipStream_t s)")
    block = int(re.search(r"constexpr int BLOCK = (\d+);", text).group(1))
    sw = body[body.index("switch (v)"):]
    out = {}
    # the persistent ids share one block: if (v == a) ... else if (v == b) ... else ...
    m = re.search(r"((?:case \d+: )+)\{(.*?)\n    \}", sw, re.S)
    ids = [int(v) for v in re.findall(r"case (\d+):", m.group(1))]
    inner = m.group(2)
    assert "grid_for(ncol, BLOCK, true)" in inner
    launches = re.findall(r"(?:if \(v == (\d+)\)|else) k_secagg<(\d+), (true|false), BLOCK, (\d+)><<<g, BLOCK, 0, s>>>", inner)
    assert len(launches) == len(ids)
    named = {int(v) for v, *_ in launches if v}
    for v, U, nt, vec in launches:
        v = int(v) if v else next(i for i in ids if i not in named)
        assert v not in out
        out[v] = LS.Shape(int(U), 1, block, int(vec), B[nt], True, False, False)
    rest = sw[m.end():]
    n_labels = 0
    for m in re.finditer(r"((?:case \d+: )+|default: )return go_secagg<(\d+), (true|false), (\d+), (\d+)>\(a, s\);", rest):
        labels, U, nt, tb, vec = m.groups()
        sh = LS.Shape(int(U), 1, int(tb), int(vec), B[nt], False, False, False)
        if labels.startswith("default"):
            default = sh
            n_labels += 1
            continue
        for v in re.findall(r"case (\d+):", labels):
            assert int(v) not in out
            out[int(v)] = sh
            n_labels += 1
    assert n_labels == len(re.findall(r"\b(?:case|default)\b", rest)), "a case of launch_secagg was not understood"
    assert "if (v >= N_VARIANTS) return hipErrorInvalidValue;" in body
    n = int(re.search(r"constexpr int N_VARIANTS = (\d+);", text).group(1))
    return {v: out.get(v, default) for v in range(n)}, {v for v in range(n) if v not in out}


@pytest.fixture(scope="module")
def text():
    return SRC.read_text()


def test_fold_table_is_the_dispatch_switch(text):
    assert parse_fold(text) == LS.FOLD_SHAPES
    assert int(re.search(r"constexpr int N_VARIANTS = (\d+);", text).group(1)) == len(LS.FOLD_SHAPES) == 24


def test_fold_table_is_the_comment_above_n_variants(text):
    """The variant table in the source's comment says the same as the switch (and so as the helper)."""
    head = text[text.index("//   id  loads  U (rows in flight)"):text.index("constexpr int N_VARIANTS")]
    rows = re.findall(r"//   (\d+)\s+(nt|plain)\s+(\d+)(?: \(\+\d+ next batch\))?\s+(\d+)\s+(\d+)\s+(\d+)\s+(.*)", head)
    assert len(rows) == 24
    for v, loads, U, W, tb, vec, grid in rows:
        sh = LS.FOLD_SHAPES[int(v)]
        assert (sh.U, sh.W, sh.block, sh.VEC, sh.nt) == (int(U), int(W), int(tb), int(vec), loads == "nt"), v
        assert sh.persistent == grid.startswith("persistent"), v
        assert sh.pipelined == ("pipelined" in grid), v
        assert sh.xmap == ("each XCD" in grid), v


def test_row_table_is_the_dispatch_switch(text):
    assert parse_rows(text) == LS.ROW_SHAPES
    assert parse_rows_honoured(text) == set(LS.ROW_SHAPES)
    for v, sh in LS.ROW_SHAPES.items():  # "same shape as the fold variant of that id"
        assert sh == LS.FOLD_SHAPES[v]


def test_secagg_table_is_the_launch_switch(text):
    shapes, defaulted = parse_secagg(text)
    assert shapes == LS.SECAGG_SHAPES
    assert defaulted == set(LS.SECAGG_DEFAULT_IDS)


def test_a_changed_template_argument_is_noticed(text):
    """The parser reads the arguments, not just the labels: one edited number changes its result."""
    edited = text.replace("case 17: return go_fedavg<MODE, 64, 1, true, 64, 1>", "case 17: return go_fedavg<MODE, 32, 1, true, 64, 1>")
    assert edited != text and parse_fold(edited) != LS.FOLD_SHAPES
    edited = text.replace("case 16: return go_secagg<48, true, 64, 1>", "case 16: return go_secagg<48, true, 64, 2>")
    assert edited != text and parse_secagg(edited)[0] != LS.SECAGG_SHAPES
    edited = text.replace("case 14: return go_fedavg_rows<MODE, 32,", "case 14: return go_fedavg_rows<MODE, 16,")
    assert edited != text and parse_rows(edited) != LS.ROW_SHAPES


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
