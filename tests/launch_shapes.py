"""The launch shapes of the column walk in pygrid_amd/csrc/pgh_kernels.hip, as data, and the
arithmetic that says which loop regions of a shape a given launch visits.  No HIP, no GPU.

A shape is one template instantiation: U rows in flight, W columns per lane, the block size, VEC
params per column, the load policy and the grid policy.  Every walk has three code regions: the
steady-state loop over full batches of U rows, the masked last batch, and the grid-stride trip over
tiles of block x W columns.  tests/test_launch_shape_table.py holds these tables against
pygrid_amd/csrc/pgh_variants.def, which the dispatch switches are generated from, and checks that
the cases derived here reach every region of every shape; tests/test_gpu_launch_shapes.py runs the
cases.
"""
from collections import namedtuple

Shape = namedtuple("Shape", "U W block VEC nt persistent pipelined xmap")
Regions = namedtuple("Regions", "full_batches remainder a_reloads full_tiles partial_tile trips")
Launch = namedtuple("Launch", "n_rows first final")

MODES = (0, 1, 2)  # mean, iterative, weighted
ROWTAB_MAX = 512   # rows one row-table launch carries (pgh_kernels.h)
CU_REF = 256       # MI355X


def _s(U, W, block, VEC, nt=True, persistent=False, pipelined=False, xmap=False):
    return Shape(U, W, block, VEC, nt, persistent, pipelined, xmap)


# the fold (the PGH_FOLD rows of pgh_variants.def, restated)
FOLD_SHAPES = {
    0: _s(8, 1, 256, 4),
    1: _s(8, 1, 256, 4, persistent=True),
    2: _s(8, 1, 256, 4, nt=False),
    3: _s(8, 1, 256, 4, nt=False, persistent=True),
    4: _s(16, 1, 256, 4, nt=False),
    5: _s(16, 1, 256, 4, nt=False, persistent=True),
    6: _s(16, 1, 256, 4),
    7: _s(4, 2, 256, 4),
    8: _s(8, 2, 256, 4),
    9: _s(8, 1, 512, 4),
    10: _s(4, 1, 256, 4),
    11: _s(16, 1, 64, 4),
    12: _s(16, 1, 64, 1),
    13: _s(8, 1, 256, 1),
    14: _s(32, 1, 64, 1),
    15: _s(32, 1, 64, 4),
    16: _s(48, 1, 64, 1),
    17: _s(64, 1, 64, 1),
    18: _s(32, 1, 128, 1),
    19: _s(16, 1, 512, 4),
    20: _s(8, 1, 1024, 4),
    21: _s(8, 1, 256, 4, pipelined=True),
    22: _s(4, 1, 256, 4, pipelined=True),
    23: _s(8, 1, 256, 4, xmap=True),
}

# the row-table kernels (any other explicit variant gives the auto choice; one without a kernel, id 0's shape)
ROW_SHAPES = {
    0: _s(8, 1, 256, 4),
    11: _s(16, 1, 64, 4),
    14: _s(32, 1, 64, 1),
    17: _s(64, 1, 64, 1),
}

# launch_secagg: columns of 2 int64 (VEC = 2) or 1; the ids without a case run the default shape
_SECAGG_DEFAULT = _s(8, 1, 256, 2)
_SECAGG_OWN = {
    1: _s(8, 1, 256, 2, persistent=True),
    2: _s(8, 1, 256, 2, nt=False),
    3: _s(8, 1, 256, 2, nt=False, persistent=True),
    4: _s(16, 1, 256, 2, nt=False),
    5: _s(16, 1, 256, 2, nt=False, persistent=True),
    6: _s(16, 1, 256, 2),
    7: _s(4, 1, 256, 2),
    10: _s(4, 1, 256, 2),
    11: _s(16, 1, 64, 2),
    12: _s(16, 1, 64, 1),
    13: _s(8, 1, 256, 1),
    14: _s(32, 1, 64, 1),
    15: _s(32, 1, 64, 2),
    16: _s(48, 1, 64, 1),
    17: _s(64, 1, 64, 1),
    18: _s(32, 1, 128, 1),
}
SECAGG_DEFAULT_IDS = (0, 8, 9, 19, 20, 21, 22, 23)
SECAGG_SHAPES = {v: _SECAGG_OWN.get(v, _SECAGG_DEFAULT) for v in range(24)}


# ---- the kernel's arithmetic -----------------------------------------------------------------------

def tile_cols(sh):
    return sh.block * sh.W


def n_cols(sh, P):
    return -(-P // sh.VEC)


def grid_for(sh, P, cu):
    """grid_for(ncol, tile, persistent): one workgroup per tile, capped at 4 x CU when persistent."""
    full = max(1, -(-n_cols(sh, P) // tile_cols(sh)))
    return min(full, 4 * cu) if sh.persistent else full


def regions(sh, n_rows, P, first, cu=CU_REF, secagg=False):
    """The loop regions one launch visits.  A FIRST fold launch takes row 0 as the accumulator and
    starts at r = 1; the share sum always starts at r = 0."""
    r = 1 if (first and not secagg) else 0
    rest = max(0, n_rows - r)
    full, rem = divmod(rest, sh.U)
    # the pipelined walk loads batch 0 into A before its loop and batch 1 into B; A is loaded again
    # inside the loop for batches 2, 4, ...
    reloads = max(0, (full - 1) // 2) if sh.pipelined else 0
    ncol, tile = n_cols(sh, P), tile_cols(sh)
    ntiles = -(-ncol // tile)
    return Regions(full, rem, reloads, ncol // tile, ncol % tile, -(-ntiles // grid_for(sh, P, cu)))


def stream_launches(N, R, batch, rows_per_client=1):
    """The launches of a STREAM fold of clients 0 .. N-1 ingested in order into a ring of R slots
    with fold batch `batch` (fold_run in pgh_reduce.cpp: a run of ready clients is folded when it
    reaches the batch, one launch per stretch of the ring; the finish folds the rest, FINAL)."""
    batch = max(1, R // 2) if batch <= 0 else min(batch, R)
    out, folded = [], 0

    def run(c0, n, final):
        done = 0
        while True:
            slot = (c0 + done) % R
            seg = min(n - done, R - slot)
            out.append(Launch(seg * rows_per_client, c0 + done == 0, final and done + seg == n))
            done += seg
            if done >= n:
                break

    for k in range(N):
        if k + 1 - folded >= batch:
            run(folded, k + 1 - folded, False)
            folded = k + 1
    run(folded, N - folded, True)
    return out


def slot_launches(parts):
    """fold_slots(parts[0]), ..., fold_slots_finish_resident(parts[-1]): one launch per part."""
    assert all(0 < n <= ROWTAB_MAX for n in parts)
    done, out = 0, []
    for i, n in enumerate(parts):
        out.append(Launch(n, done == 0, i == len(parts) - 1))
        done += n
    return out


# ---- the cases the GPU tests run -------------------------------------------------------------------

def fold_P(sh, r):
    """Two full tiles, half a tile and r params."""
    return (2 * tile_cols(sh) + tile_cols(sh) // 2) * sh.VEC + r


def fold_N_sweep(sh):
    U = sh.U
    return [U, U + 1, U + 2, 2 * U, 2 * U + 1, 2 * U + 2, 3 * U + 1, 3 * U + 2]


def fold_cases(sh):
    """(N, P) of the single-launch folds: the N sweep at r = 3, the residues at N = 2U + 2."""
    return [(N, fold_P(sh, 3)) for N in fold_N_sweep(sh)] + [(2 * sh.U + 2, fold_P(sh, r)) for r in (0, 1, 2)]


def stream_cases(sh):
    """(N, P, R, batch) of the continuation folds.  R = batch = U: a FIRST launch of U rows, a middle
    launch that takes one full batch from r = 0, a FINAL launch of 2 rows.  R = batch = U + 1: the
    FIRST launch takes a full batch from r = 1, the middle one a full batch and a row, the FINAL one
    no row at all (it only reads the state and writes out)."""
    U = sh.U
    return [(2 * U + 2, fold_P(sh, 1), U, U), (2 * U + 2, fold_P(sh, 3), U + 1, U + 1)]


def persistent_P(cu, secagg=False):
    """More than twice the tiles a persistent grid of 4 x CU workgroups holds, a partial one last."""
    tile = 512 if secagg else 1024  # 256 columns of 2 int64 / of 4 fp32
    return 2 * (4 * cu * tile) + tile + 3


PERSISTENT_N = 3


def row_cases(sh):
    """(N, P, first part) of the row-table folds: rows[:first part] go to fold_slots, the rest to
    fold_slots_finish_resident; neither part is a multiple of U.  N = 3U + 2 is there for the
    continuation launch that runs the full-batch loop twice."""
    U = sh.U
    return ([(U + 1, fold_P(sh, 3), 3), (2 * U + 2, fold_P(sh, 3), U + 1), (3 * U + 2, fold_P(sh, 3), 3)] +
            [(2 * U + 2, fold_P(sh, r), U + 1) for r in (0, 1, 2)])


def secagg_P(sh, odd):
    return (2 * sh.block + sh.block // 2) * sh.VEC + (1 if odd else 0)


def secagg_cases(sh):
    """(N clients, S parties, P, ring batch): N x S rows in {U, U+1, 2U+1, 2U+2}, S in {1, 3}, P even
    and odd in turn.  The ring run of a case has R = batch = N // 2 clients: a FIRST launch, a middle
    launch and the FINAL one."""
    U, out = sh.U, []
    for S in (1, 3):
        for rows in (U, U + 1, 2 * U + 1, 2 * U + 2):
            if rows % S == 0:
                N = rows // S
                out.append((N, S, secagg_P(sh, odd=len(out) % 2 == 1), max(1, N // 2)))
    return out


def fold_visits(sh, cu=CU_REF):
    """Regions of every launch of the fold cases of a shape, with the launch's P."""
    out = [(P, regions(sh, N, P, True, cu)) for N, P in fold_cases(sh)]
    for N, P, R, batch in stream_cases(sh):
        out += [(P, regions(sh, l.n_rows, P, l.first, cu)) for l in stream_launches(N, R, batch)]
    if sh.persistent:
        P = persistent_P(cu)
        out.append((P, regions(sh, PERSISTENT_N, P, True, cu)))
    return out


def row_visits(sh, cu=CU_REF):
    out = []
    for N, P, a in row_cases(sh):
        out += [(P, regions(sh, l.n_rows, P, l.first, cu)) for l in slot_launches([a, N - a])]
    return out


def secagg_visits(sh, cu=CU_REF):
    out = []
    for N, S, P, batch in secagg_cases(sh):
        out.append((P, regions(sh, N * S, P, True, cu, secagg=True)))
        out += [(P, regions(sh, l.n_rows, P, l.first, cu, secagg=True))
                for l in stream_launches(N, batch, batch, rows_per_client=S)]
    if sh.persistent:
        P = persistent_P(cu, secagg=True)
        out.append((P, regions(sh, PERSISTENT_N, P, True, cu, secagg=True)))
    return out
