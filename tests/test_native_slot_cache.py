"""CPU: the per-slot state machine of a cached row reduction (pgh_host.h: SlotCache, under RowSums' two caches of
K7's sums and K14's dots) in a stand-alone program under ASan + UBSan: tests/native/slot_cache_check.cpp runs a
scripted sequence of its own, then replays random operation sequences written here against the model below.  That
it compiles with plain g++, nothing on the include path and no other source is also the proof that the state
machine is HIP-free and header-only."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NONE, QUEUED, VALID = 0, 1, 2
SLOTS = 8


class Model:
    """What SlotCache is meant to do, slot by slot: ``state`` and ``value`` per slot, the ``queued`` list."""

    def __init__(self):
        self.state, self.value, self.queued = {}, {}, []

    def apply(self, op, *a):
        """One operation; the list ``missing`` returns for M and Q, else None."""
        st, todo = self.state, None
        if op == "R":
            self.state, self.value, self.queued = {k: NONE for k in range(a[0])}, {k: 0.0 for k in range(a[0])}, []
        elif op == "W":
            st.update({k: NONE for k in range(a[0], a[0] + a[1])})
        elif op in "MQ":
            todo = [s for k, s in enumerate(a[0]) if st[s] == NONE and s not in a[0][:k]]
            if op == "Q":
                st.update({s: QUEUED for s in todo})
                self.queued += todo
        elif op == "H":
            for s in self.queued:
                if st[s] == QUEUED:
                    st[s], self.value[s] = VALID, a[0][s]
            self.queued = []
        elif op in "SF":
            self.state, self.queued = {k: NONE for k in st}, []
        elif op == "C":
            self.state, self.value, self.queued = {}, {}, []
        return todo

    def words(self):
        return [str(len(self.state))] + [f"{self.state[k]} {self.value[k]:.0f}" for k in sorted(self.state)] + [str(int(bool(self.queued)))]


def sequences(count, seed):
    rng = np.random.default_rng(seed)
    out = [str(count)]
    for _ in range(count):
        m, stamp = Model(), 100
        ops = [("R", SLOTS)]
        for _ in range(int(rng.integers(10, 40))):
            n = len(m.state)
            kind = rng.choice(list("QQQQMHHHWWWSFRC"))
            if n == 0 or kind == "R":
                ops.append(("R", int(rng.integers(1, SLOTS + 1))))
            elif kind == "W":
                slot = int(rng.integers(0, n))
                ops.append(("W", slot, int(rng.integers(0, n - slot + 1))))
            elif kind in "QM":
                ops.append((kind, [int(s) for s in rng.integers(0, n, int(rng.integers(0, 2 * n)))]))
            elif kind == "H":
                stamp += 100
                ops.append(("H", [float(stamp + k) for k in range(n)]))
            else:
                ops.append((kind,))
            m.apply(*ops[-1])  # (only to know the length the next operation sees)
        m = Model()
        out.append(str(len(ops)))
        for op in ops:
            todo = m.apply(*op)
            line = [op[0]] + [str(x) for x in op[1:] if not isinstance(x, list)]
            if op[0] in "MQ":
                line += [str(len(op[1]))] + [str(s) for s in op[1]] + [str(len(todo))] + [str(s) for s in todo]
            if op[0] == "H":
                line += [f"{v:.0f}" for v in op[1]]
            out.append(" ".join(line + m.words()))
    return out


def test_the_model_itself():
    m = Model()
    m.apply("R", 4)
    assert m.apply("Q", [2, 0, 2, 3]) == [2, 0, 3] and m.apply("M", [0, 1, 1]) == [1]
    m.apply("W", 3, 1)
    m.apply("H", [5.0, 6.0, 7.0, 8.0])
    assert m.state == {0: VALID, 1: NONE, 2: VALID, 3: NONE} and m.value == {0: 5.0, 1: 0.0, 2: 7.0, 3: 0.0}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_slot_cache_under_asan_ubsan(tmp_path):
    txt = tmp_path / "slot_cache_sequences.txt"
    txt.write_text("\n".join(sequences(300, 15)) + "\n")
    exe = tmp_path / "slot_cache_check_asan_ubsan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "native" / "slot_cache_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(txt)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: the scripted sequence, 300 replayed")
