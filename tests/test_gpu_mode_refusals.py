"""GPU: which averaging mode every entry point accepts, on which kind of context -- the returned status
of every combination, held against one literal table.  (The message texts are not part of it.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
OK, ARG, STATE, UNSUPPORTED = 0, -1, -3, -6
# the six averaging modes, PGH_STREAM_SECAGG (a stream kind, not a mode) and a number that is neither
MODES = (0, 1, 2, 3, 4, 5, 16, 99)
KINDS = ("single", "group", "streaming", "unset")
WITH_MODE = ("fedavg", "fedavg_resident", "fedavg_device", "fold_slots", "fold_slots_finish_resident", "stream_begin")
WITHOUT_MODE = ("set_clip_norm", "set_trim", "clip_stats")
N, P = 3, 8

# EXPECTED[kind][entry point]: the status per mode of MODES, or the one status of a call that takes no mode
_ = OK
A, S, U = ARG, STATE, UNSUPPORTED
EXPECTED = {
    "single": {                       # mean it. wtd clip trim med  sec  99
        "fedavg":                     (_, _, _, _, _, _, A, A),
        "fedavg_resident":            (_, _, _, _, _, _, A, A),
        "fedavg_device":              (_, _, _, _, _, _, A, A),
        "fold_slots":                 (_, _, _, _, _, U, A, A),  # a median folds nothing early
        "fold_slots_finish_resident": (_, _, _, _, _, _, A, A),
        "stream_begin":               (_, _, _, U, U, U, S, A),  # (the share sum wants an int64 slab)
        "set_clip_norm": OK, "set_trim": OK, "clip_stats": OK,
    },
    "group": {                        # a group does not clip; device pointers name one GPU
        "fedavg":                     (_, _, _, U, _, _, A, A),
        "fedavg_resident":            (_, _, _, U, _, _, A, A),
        "fedavg_device":              (U, U, U, U, U, U, U, U),
        "fold_slots":                 (_, _, _, U, _, U, A, A),
        "fold_slots_finish_resident": (_, _, _, U, _, _, A, A),
        "stream_begin":               (_, _, _, U, U, U, S, A),
        "set_clip_norm": U, "set_trim": OK, "clip_stats": U,
    },
    "streaming": {                    # an unknown mode is told from the wrong state
        "fedavg":                     (S, S, S, S, S, S, A, A),
        "fedavg_resident":            (S, S, S, S, S, S, A, A),
        "fedavg_device":              (S, S, S, S, S, S, A, A),
        "fold_slots":                 (S, S, S, S, S, U, A, A),
        "fold_slots_finish_resident": (S, S, S, S, S, S, A, A),
        "stream_begin":               (_, _, _, U, U, U, S, A),  # (a new stream replaces the open one)
        "set_clip_norm": U, "set_trim": OK, "clip_stats": OK,
    },
    "unset": {                        # no bound, no count: PGH_E_STATE, but a stream refuses the rule first
        "fedavg":                     (_, _, _, S, S, _, A, A),
        "fedavg_resident":            (_, _, _, S, S, _, A, A),
        "fedavg_device":              (_, _, _, S, S, _, A, A),
        "fold_slots":                 (_, _, _, S, S, U, A, A),
        "fold_slots_finish_resident": (_, _, _, S, S, _, A, A),
        "stream_begin":               (_, _, _, U, U, U, S, A),
        "set_clip_norm": OK, "set_trim": OK, "clip_stats": OK,
    },
}


def status(fn, *a):
    from pygrid_amd.exceptions import AggregationError

    try:
        fn(*a)
    except AggregationError as e:
        return e.status
    return OK


def prepare(eng, kind, diffs, ckpt):
    """single: three fp32 diffs, a resident checkpoint, weights, a clip bound and a trim count.  group:
    the same on a group of one GPU (which takes no clip bound).  streaming: like single, then a MEAN
    stream with one client ingested.  unset: like single without the bound and the count."""
    eng.set_layout([P])
    eng.reserve(N)
    if kind != "group":
        eng.set_clip_norm(0.0 if kind == "unset" else 1.0)
    eng.set_trim(0 if kind == "unset" else 1)
    if kind == "streaming":
        eng.stream_begin(0, 2)
    for k in range(1 if kind == "streaming" else N):
        eng.ingest(k, diffs[k])
    eng.set_weights(np.ones(N, F))
    eng.ckpt_upload(ckpt)


def observe(engines):
    import torch

    diffs = np.random.default_rng(8).standard_normal((N, P)).astype(F)
    ckpt = np.zeros(P, F)
    d_ckpt, d_out = torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
    got = {}
    for kind in KINDS:
        eng = engines["group" if kind == "group" else "single"]
        calls = {
            "fedavg": lambda m: eng.fedavg(m, ckpt),
            "fedavg_resident": eng.fedavg_resident,
            "fedavg_device": lambda m: eng.fedavg_device(m, d_ckpt.data_ptr(), d_out.data_ptr()),
            "fold_slots": lambda m: eng.fold_slots(m, [0]),
            "fold_slots_finish_resident": lambda m: eng.fold_slots_finish_resident(m, [0, 1, 2]),
            "stream_begin": eng.stream_begin,
            "set_clip_norm": lambda: eng.set_clip_norm(2.0),
            "set_trim": lambda: eng.set_trim(1),
            "clip_stats": eng.clip_stats,
        }
        got[kind] = {}
        for entry in WITH_MODE:
            row = []
            for mode in MODES:
                prepare(eng, kind, diffs, ckpt)  # every call meets the same state
                row.append(status(calls[entry], mode))
                torch.cuda.synchronize()
            got[kind][entry] = tuple(row)
        for entry in WITHOUT_MODE:
            prepare(eng, kind, diffs, ckpt)
            got[kind][entry] = status(calls[entry])
    return got


@pytest.fixture
def engines(engine):
    from pygrid_amd import Engine

    with Engine(devices=[0]) as grp:
        yield {"single": engine, "group": grp}
    engine.set_layout([P])  # (ends a stream left open, frees the slab)
    engine.set_clip_norm(0.0)
    engine.set_trim(0)


def test_every_mode_on_every_entry_point(engines):
    got = observe(engines)
    for kind in KINDS:
        for entry in WITH_MODE + WITHOUT_MODE:
            print(kind, entry, got[kind][entry])
    assert got == EXPECTED
