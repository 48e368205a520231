"""CPU: the server optimizers' arithmetic (the numpy oracle against a scalar restatement, the -0 trick,
the golden file), the ``server_optimizer`` config parser, ``ServerOptStates`` on a fake engine, and the
C ABI's new symbols.  The definition is in include/pgh_api.h and DESIGN.md section 5."""
import ctypes as C
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_serveropt_golden as GG  # noqa: E402
import serveropt_oracle as SO  # noqa: E402
from oracle import oracle as O  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
HP = {"lr": 0.3, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}


def specials():
    return np.array(GG.SPECIAL_BITS, np.uint32).view(F)


# ---- arithmetic --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SO.KINDS)
def test_oracle_matches_scalar_restatement(kind):
    rng = np.random.default_rng(kind)
    sp = specials()
    n = 320
    ck = (rng.standard_normal(n) * 0.1).astype(F)
    g = (rng.standard_normal(n) * 1e-2).astype(F)
    m = (rng.standard_normal(n) * 1e-2).astype(F)
    v = (rng.random(n) * 1e-4).astype(F)
    # specials in g, m and v (v also negative and NaN: the oracle follows IEEE, whatever the state)
    g[:sp.size] = sp
    m[sp.size:2 * sp.size] = sp
    v[2 * sp.size:3 * sp.size] = sp
    g[3 * sp.size:4 * sp.size] = sp
    v[3 * sp.size:4 * sp.size] = sp[::-1]
    out, m2, v2 = SO.step(kind, ck, g, m, v, **HP)
    for i in range(n):
        so, sm, sv = SO.step_scalar(kind, float(ck[i]), float(g[i]), float(m[i]), float(v[i]), **HP)
        for name, got, want in (("out", out[i], so), ("m", m2[i], sm), ("v", v2[i], sv)):
            assert SO.same_bits([got], [F(want)]), (kind, i, name, got, want, ck[i], g[i], m[i], v[i])


def test_minus_zero_minus_g_is_minus_g_bitwise():
    """(-0.0f) - g == -g bit for bit for every non-NaN g: what lets the unchanged fold kernels hand g
    to K10 through a checkpoint plane of -0."""
    rng = np.random.default_rng(3)
    bits = np.concatenate([np.array(GG.SPECIAL_BITS, np.uint32),
                           rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)])
    g = bits.view(F)
    with np.errstate(all="ignore"):
        d = (np.full(g.size, -0.0, F) - g).astype(F)
    ok = ~np.isnan(g)
    assert ok.sum() > 190000
    assert np.array_equal(d.view(np.uint32)[ok], bits[ok] ^ np.uint32(0x80000000))
    assert np.isnan(d[~ok]).all()
    # and flipping the sign bit takes g back, signed zeros included
    assert np.array_equal(SO.flip(d).view(np.uint32)[ok], bits[ok])
    for z in (0.0, -0.0):
        assert math.copysign(1.0, float(F(-0.0) - F(z))) == -math.copysign(1.0, z)


def test_avg_from_equals_the_direct_mean():
    rng = np.random.default_rng(9)
    ds = [(rng.standard_normal(301) * 1e-2).astype(F) for _ in range(4)]
    ds[1][:16] = specials()
    g = SO.avg_from(lambda ck: O.fedavg_mean([ck], [[d] for d in ds])[0], 301)
    with np.errstate(all="ignore"):
        acc = ds[0]
        for d in ds[1:]:
            acc = acc + d
        want = acc / F(4)
    assert SO.same_bits(g, want)


def test_fedavgm_beta0_lr1_is_plain_fedavg_where_avg_is_not_zero():
    rng = np.random.default_rng(11)
    n = 4096
    ck = (rng.standard_normal(n) * 0.1).astype(F)
    g = (rng.standard_normal(n) * 1e-2).astype(F)
    g[:16] = specials()
    m, v = SO.init_state(n, 1e-3)
    out, m2, _ = SO.step(SO.MOMENTUM, ck, g, m, v, lr=1.0, beta1=0.0, beta2=0.0, tau=1e-3)
    with np.errstate(all="ignore"):
        want = ck - g
    nz = g != 0  # (0 * m + (-0) is +0: a zero average may change sign on the way through m)
    assert SO.same_bits(out[nz], want[nz])
    assert np.array_equal(out[~nz & ~np.isnan(g)], ck[~nz & ~np.isnan(g)])  # equal as numbers everywhere
    assert SO.same_bits(m2[nz], g[nz])


def test_golden_file_is_current():
    assert GG.GOLDEN.stat().st_size < 64 << 10
    G = np.load(GG.GOLDEN)
    want = GG.build()
    assert sorted(G.files) == sorted(want)
    for k in want:
        assert SO.same_bits(G[k], want[k]), k


# ---- config parsing ------------------------------------------------------------------------------------

def test_config_accepted_forms():
    from pygrid_amd.engine import OPT_ADAGRAD, OPT_ADAM, OPT_MOMENTUM, OPT_YOGI
    from pygrid_amd.serveropt import server_opt_of

    assert server_opt_of({}) is None
    assert server_opt_of({"server_optimizer": None}) is None
    s = server_opt_of({"server_optimizer": {"name": "fedadam", "lr": 0.1}})
    assert (s.kind, s.lr, s.beta1, s.beta2, s.tau) == (OPT_ADAM, float(F(0.1)), float(F(0.9)), float(F(0.99)), float(F(1e-3)))
    s = server_opt_of({"server_optimizer": {"name": "fedyogi", "lr": 1, "beta1": 0, "beta2": 0.5, "tau": 1e-2}})
    assert (s.kind, s.lr, s.beta1, s.beta2) == (OPT_YOGI, 1.0, 0.0, 0.5)
    s = server_opt_of({"server_optimizer": {"name": "fedadagrad", "lr": np.float32(2.0), "beta2": 7.0}})
    assert (s.kind, s.beta2) == (OPT_ADAGRAD, 0.0)  # beta2 is not Adagrad's: ignored
    s = server_opt_of({"server_optimizer": {"name": "fedavgm", "lr": 1.0, "beta1": 0.5, "tau": -1, "beta2": 3}})
    assert (s.kind, s.beta2, s.tau) == (OPT_MOMENTUM, 0.0, 0.0)  # neither is FedAvgM's
    assert s == server_opt_of({"server_optimizer": {"name": "fedavgm", "lr": 1.0, "beta1": 0.5}})


@pytest.mark.parametrize("cfg", [
    "fedadam", 3, ["fedadam"],
    {"lr": 0.1}, {"name": "adam", "lr": 0.1}, {"name": None, "lr": 0.1}, {"name": 3, "lr": 0.1},
    {"name": "fedadam"}, {"name": "fedadam", "lr": 0.1, "momentum": 0.9}, {"name": "fedadam", "lr": 0.1, 5: 1},
    {"name": "fedadam", "lr": True}, {"name": "fedadam", "lr": "0.1"}, {"name": "fedadam", "lr": None},
    {"name": "fedadam", "lr": 0}, {"name": "fedadam", "lr": -1.0}, {"name": "fedadam", "lr": float("nan")},
    {"name": "fedadam", "lr": float("inf")}, {"name": "fedadam", "lr": 1e39}, {"name": "fedadam", "lr": 1e-50},
    {"name": "fedadam", "lr": 0.1, "beta1": 1.0}, {"name": "fedadam", "lr": 0.1, "beta1": -0.1},
    {"name": "fedadam", "lr": 0.1, "beta1": 0.9999999999}, {"name": "fedadam", "lr": 0.1, "beta1": False},
    {"name": "fedadam", "lr": 0.1, "beta2": 1.0}, {"name": "fedyogi", "lr": 0.1, "beta2": float("nan")},
    {"name": "fedadam", "lr": 0.1, "tau": 0}, {"name": "fedadagrad", "lr": 0.1, "tau": -1e-3},
    {"name": "fedadagrad", "lr": 0.1, "tau": float("inf")}, {"name": "fedavgm", "lr": 0.1, "tau": float("nan")},
    {"name": "fedavgm", "lr": 0.1, "beta2": "x"},
])
def test_config_refused_forms(cfg):
    from pygrid_amd.exceptions import AggregationError
    from pygrid_amd.serveropt import server_opt_of

    with pytest.raises(AggregationError):
        server_opt_of({"server_optimizer": cfg})


# ---- ServerOptStates on a fake engine ------------------------------------------------------------------

class FakeOptEngine:
    """The engine's optimizer surface with the library's semantics (set / commit / download / upload),
    and a 'close' that moves the pending state by a recognisable amount."""

    def __init__(self, p):
        self.p = p
        self.numel = (p,)
        self.opt_owner = None
        self.spec = None
        self.m = self.v = self.m2 = self.v2 = None
        self.pending = False
        self.calls = []

    def set_server_opt(self, kind, lr=0.0, beta1=0.0, beta2=0.0, tau=0.0):
        self.calls.append(("set", kind))
        spec = (kind, lr, beta1, beta2, tau)
        if kind == 0:
            self.spec, self.m, self.v, self.pending, self.opt_owner = None, None, None, False, None
            return
        if spec == self.spec:
            return
        self.spec = spec
        self.m, self.v = np.zeros(self.p, F), np.full(self.p, F(tau) * F(tau), F)
        self.pending = False

    def final(self, by):  # what a FINAL fold does to the state
        if self.spec is None:
            return
        self.m2, self.v2 = self.m + F(by), self.v + F(by)
        self.pending = True

    def server_opt_commit(self):
        from pygrid_amd.exceptions import AggregationError

        self.calls.append(("commit",))
        if not self.pending:
            raise AggregationError("nothing pending", status=-3)
        self.m, self.v, self.pending = self.m2, self.v2, False

    def server_opt_state(self):
        self.calls.append(("download",))
        return self.m.copy(), self.v.copy()

    def load_server_opt_state(self, m, v=None):
        self.calls.append(("upload",))
        self.m, self.v, self.pending = np.array(m, F), np.array(v, F), False


def spec_of(name="fedadam", lr=0.1):
    from pygrid_amd.serveropt import server_opt_of

    return server_opt_of({"server_optimizer": {"name": name, "lr": lr}})


def test_states_two_keys_evict_and_restore_each_other():
    from pygrid_amd.serveropt import ServerOptStates

    eng, st = FakeOptEngine(5), ServerOptStates()
    a, b = spec_of("fedadam"), spec_of("fedadam")  # the same setting: the state must still not leak across keys
    st.bind(eng, "A", a, 5)
    eng.final(1.0)
    st.commit(eng)
    assert eng.opt_owner == (st, "A") and st.steps("A") == 1
    st.bind(eng, "B", b, 5)  # A's committed state goes to the host, B starts fresh
    assert eng.opt_owner == (st, "B") and np.all(eng.m == 0) and st.steps("B") == 0
    eng.final(10.0)
    st.commit(eng)
    eng.final(10.0)
    st.commit(eng)
    st.bind(eng, "A", a, 5)  # B's goes to the host, A's comes back
    assert np.all(eng.m == 1.0) and st.steps("A") == 1
    before = len(eng.calls)
    st.bind(eng, "A", a, 5)  # resident already: nothing moves
    assert eng.calls[before:] == [("set", a.kind)]
    st.bind(eng, "B", b, 5)
    assert np.all(eng.m == 20.0) and st.steps("B") == 2
    m, v, steps = st.state(eng, "A")
    assert np.all(m == 1.0) and steps == 1
    # a changed setting starts again
    st.bind(eng, "A", spec_of("fedadam", lr=0.2), 5)
    assert np.all(eng.m == 0) and st.steps("A") == 0


def test_states_uncommitted_step_is_dropped_and_none_is_set_without_the_key():
    from pygrid_amd.serveropt import ServerOptStates

    eng, st = FakeOptEngine(3), ServerOptStates()
    st.bind(eng, "A", spec_of(), 3)
    eng.final(1.0)
    st.commit(eng)
    eng.final(5.0)  # a close that failed after its fold: no commit
    st.bind(eng, None, None, 3)  # a process without the key: the optimizer is off, A's state parked
    assert eng.spec is None and eng.opt_owner is None and ("set", 0) in eng.calls
    st.bind(eng, "A", spec_of(), 3)
    assert np.all(eng.m == 1.0) and st.steps("A") == 1


def test_states_need_a_key_and_a_capable_engine():
    from pygrid_amd.exceptions import AggregationError, PlanNotAcceleratedError, ServerOptUnavailableError
    from pygrid_amd.serveropt import ServerOptStates

    st = ServerOptStates()
    with pytest.raises(AggregationError):
        st.bind(FakeOptEngine(3), None, spec_of(), 3)
    with pytest.raises(ServerOptUnavailableError):
        st.bind(object(), "A", spec_of(), 3)
    st.bind(object(), None, None, 3)  # no optimizer, an engine without the setter: left alone

    class Refusing(FakeOptEngine):
        def set_server_opt(self, kind, *a):
            if kind:
                raise AggregationError("no", status=-6)

    with pytest.raises(ServerOptUnavailableError):
        st.bind(Refusing(3), "A", spec_of(), 3)
    assert not issubclass(ServerOptUnavailableError, PlanNotAcceleratedError)


class FakeCloseEngine(FakeOptEngine):
    """Enough of an Engine for CycleAggregator.average_params."""
    dtype, parties, max_clients, ckpt_owner = 0, 1, 0, None

    def set_layout(self, numel):
        self.numel, self.opt_owner = tuple(numel), None

    def reserve(self, n, dtype=0, parties=1):
        self.max_clients = n

    def reset(self):
        pass

    def ingest(self, i, flat):
        pass

    fail_close = False

    def fedavg(self, mode, flat):
        from pygrid_amd.exceptions import AggregationError

        self.final(1.0)
        if self.fail_close:
            raise AggregationError("the result never reached the host", status=-2)
        return flat


def test_aggregator_commits_after_the_result_and_not_when_the_close_raises():
    from pygrid_amd.cycle import CycleAggregator
    from pygrid_amd.exceptions import AggregationError, ServerOptUnavailableError

    eng = FakeCloseEngine(4)
    agg = CycleAggregator(eng)
    cfg = {"server_optimizer": {"name": "fedadam", "lr": 0.1}}
    ck, ds = [np.zeros(4, F)], [[np.ones(4, F)], [np.ones(4, F)]]
    agg.average_params(cfg, ck, ds, opt_key=7)
    assert agg.opt_states.steps(7) == 1 and eng.calls[-1] == ("commit",)
    eng.fail_close = True
    with pytest.raises(AggregationError):
        agg.average_params(cfg, ck, ds, opt_key=7)
    assert agg.opt_states.steps(7) == 1 and eng.calls[-1] != ("commit",)
    eng.fail_close = False
    with pytest.raises(AggregationError):  # a configured optimizer needs the key
        agg.average_params(cfg, ck, ds)
    agg.average_params({}, ck, ds)  # another process on the same engine, no optimizer
    assert eng.spec is None
    # the engine declines the cycle (a hosted plan it does not run): fail closed, no fall-back
    with pytest.raises(ServerOptUnavailableError):
        agg.average_params(cfg, ck, ds, avg_plan=lambda *a: None, opt_key=7)


# ---- the C ABI ---------------------------------------------------------------------------------------------

NEW = ("pgh_set_server_opt", "pgh_server_opt_commit", "pgh_server_opt_steps", "pgh_server_opt_download",
       "pgh_server_opt_upload")


def test_header_declares_library_exports_abi_still_10():
    from pygrid_amd import _lib

    text = (ROOT / "include" / "pgh_api.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    for name, val in (("PGH_OPT_NONE", 0), ("PGH_OPT_MOMENTUM", 1), ("PGH_OPT_ADAGRAD", 2), ("PGH_OPT_ADAM", 3),
                      ("PGH_OPT_YOGI", 4)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, val), code), name
    assert re.search(r"#define\s+PGH_ABI_VERSION\s+10\b", code)
    assert lib.pgh_abi_version() == _lib.ABI_VERSION == 10


def test_null_arguments_return_e_arg_without_a_gpu():
    from pygrid_amd import _lib

    lib = _lib.load()
    one = C.c_float(1.0)
    n = C.c_int64(0)
    buf = (C.c_float * 4)()
    assert lib.pgh_set_server_opt(None, 3, one, C.c_float(0.9), C.c_float(0.99), C.c_float(1e-3)) == -1
    assert lib.pgh_set_server_opt(None, 0, one, one, one, one) == -1
    assert lib.pgh_server_opt_commit(None) == -1
    assert lib.pgh_server_opt_steps(None, C.byref(n)) == -1
    assert lib.pgh_server_opt_steps(None, None) == -1
    assert lib.pgh_server_opt_download(None, buf, buf) == -1
    assert lib.pgh_server_opt_upload(None, buf, buf, 16) == -1
