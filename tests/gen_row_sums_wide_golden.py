"""Writes tests/golden/row_sums_wide.npz: the sums of squares (u64 bit patterns) of the rows of
tests/gen_clip_golden.py's ``wide_rows`` at its three widths ``WIDE_P`` -- past one chunk of the engine's fold of
the tile partials -- and of ``wide_other``, as tests/clip_oracle.py computed them when the widths were added.  Bits
only: the rows are regenerated.  The file is written with fixed zip dates, so a second run gives the same bytes
(tests/test_row_sums_wide.py holds it to that).  Run from the repository root:

    python tests/gen_row_sums_wide_golden.py

Only when the definition itself changes (the oracle and this file together) or the widths move with
the fold's chunk."""
from __future__ import annotations

import functools
import io
import sys
import zipfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import clip_oracle as CO  # noqa: E402
import gen_clip_golden as GG  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "row_sums_wide.npz"


@functools.lru_cache(maxsize=None)
def wide_partials(p: int) -> tuple:
    """The tile partials of every row of ``wide_rows(p)`` (cached: the tests fold them in wrong orders too)."""
    return tuple(CO.tile_partials(r) for r in GG.wide_rows(p))


def left_fold(parts) -> np.float64:
    """``row_sumsq``'s fold over partials already computed; nothing folded is +0.0."""
    acc = np.float64(0.0)
    with np.errstate(all="ignore"):
        for x in parts:
            acc = np.float64(acc + x)
    return acc


@functools.lru_cache(maxsize=None)
def wide_sums(p: int) -> np.ndarray:
    s = np.array([left_fold(parts) for parts in wide_partials(p)], np.float64)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def other_sum(p: int) -> np.float64:
    return CO.row_sumsq(GG.wide_other(p))


def build() -> dict:
    out = {"wide_p": np.array(GG.WIDE_P, np.int64)}
    for p in GG.WIDE_P:
        out[f"sumsq_bits_{p}"] = GG.bits64(wide_sums(p)).copy()
        out[f"other_bits_{p}"] = GG.bits64([other_sum(p)]).copy()
    return out


def npz_bytes(arrays: dict) -> bytes:
    """An uncompressed .npz of the arrays, members in name order and dated 1980-01-01: the same bytes every run."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asarray(arrays[name]), version=(1, 0), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())
    return buf.getvalue()


def main():
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    GOLDEN.write_bytes(npz_bytes(build()))
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
