"""particles_amd.smoothing as a module: the history names it shares with particles_amd.collectors, the one replay-tape
reader behind the six smoothing entries (each caller's messages, word for word as they were when every entry read its
own tapes), and the one table of model kinds.  Host only: nothing here reaches the library.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import particles_amd as pa
from particles_amd import _lib, collectors, mcmc, smoothing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, I64 = np.float64, np.int64

HISTORY_NAMES = ("generate_hist_obj", "PartialParticleHistory", "RollingParticleHistory", "ParticleHistory",
                 "DeviceParticleHistory", "DeviceRollingParticleHistory")


@pytest.mark.parametrize("name", HISTORY_NAMES)
def test_history_names_are_shared(name):
    assert getattr(collectors, name) is getattr(smoothing, name)
    assert getattr(pa.smoothing, name) is getattr(pa.collectors, name)


def test_imports_on_its_own():
    """A fresh interpreter imports the module first; at module level it names neither ``core`` nor ``collectors``."""
    code = ("import sys, particles_amd.smoothing as s; "
            "assert not hasattr(s, 'core') and not hasattr(s, 'collectors'); "
            "assert s.DeviceParticleHistory is sys.modules['particles_amd.collectors'].DeviceParticleHistory")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr


# ---- the reader, by the six callers' (who, spec[, subject]) ---------------------------------------------------------
# The expected strings are the callers' own, as each wrote them before there was a reader.
M, T, C, NS, P = 3, 4, 2, 2, 5
CALLERS = {
    "two_filter": ("two-filter smoothing", {"u_fwd": ((P,), F64), "u_info": ((P,), F64), "idx_fwd": ((P,), I64),
                                            "idx_info": ((P,), I64)}, "replay"),
    "qmc_points": ("backward sampling", {"u": ((M, T), F64)}, "replay"),
    "backward": ("backward sampling", {"idx_last": ((M,), I64), "u_last": ((M,), F64), "u_prop": ((T - 1, NS, M), F64),
                                       "u_acc": ((T - 1, NS, M), F64), "u": ((T - 1, M), F64)}, "replay"),
    "one_launch": ("backward sampling", {"u_last": ((1,), F64), "u": ((T - 1, 1), F64)}, "replay"),
    "paris": ("Paris", {"u_prop": ((NS, M), F64), "u_acc": ((NS, M), F64), "u": ((M,), F64)}, "replay(7)"),
    "new_paths": ("new_paths", {"u_last": ((C,), F64), "u": ((T - 1, C), F64)}, "replay"),
}


@pytest.mark.parametrize("caller", sorted(CALLERS))
def test_reader(caller):
    who, spec, subject = CALLERS[caller]
    with pytest.raises(ValueError) as e:
        smoothing.read_tapes(who, {"zz": 1, "aa": 2}, spec, subject)
    assert str(e.value) == "%s: unknown replay tape(s) %s" % (who, ["aa", "zz"])
    for name, (shape, dtype) in spec.items():
        bad = shape[:-1] + (shape[-1] + 1,)
        with pytest.raises(ValueError) as e:
            smoothing.read_tapes(who, {name: np.zeros(bad)}, spec, subject)
        assert str(e.value) == "%s: %s[%r] has shape %s, expected %s" % (who, subject, name, bad, shape)
        # absent and None
        out = smoothing.read_tapes(who, {name: None}, spec, subject)
        assert set(out) == set(spec) and all(v is None for v in out.values())
        assert smoothing.read_tapes(who, None, spec, subject) == dict.fromkeys(spec)
        # Fortran order and another number type come back C-contiguous in the spec's dtype, values kept
        src = np.asfortranarray(np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape))
        a = smoothing.read_tapes(who, {name: src}, spec, subject)[name]
        assert a.flags["C_CONTIGUOUS"] and a.dtype == dtype and a.shape == shape and np.array_equal(a, src)
        a = smoothing.read_tapes(who, {name: src.astype(np.float32).tolist()}, spec, subject)[name]
        assert a.flags["C_CONTIGUOUS"] and a.dtype == dtype and np.array_equal(a, src)
        # a shape of None is not checked
        free = dict(spec, **{name: (None, dtype)})
        a = smoothing.read_tapes(who, {name: np.zeros(bad, dtype=np.int32)}, free, subject)[name]
        assert a.shape == bad and a.dtype == dtype


# ---- the six callers themselves, on stand-ins that stop short of the library ---------------------------------------

def _fake_filter(**kw):
    return types.SimpleNamespace(**dict(dict(_fused=True, _keep_history=1, n_islands=C, _n=T, N=M, qmc=False,
                                             _cond_device=True), **kw))


def _history(**kw):
    h = object.__new__(smoothing.DeviceParticleHistory)
    h._smc = _fake_filter(**kw)
    h.fk = None
    return h


def _raises(msg, f, *a, **kw):
    with pytest.raises(ValueError) as e:
        f(*a, **kw)
    assert str(e.value) == msg


def test_two_filter_replay_messages():
    _raises("two-filter smoothing: unknown replay tape(s) ['u']", smoothing._two_filter_replay, {"u": [0.5]}, P)
    _raises("two-filter smoothing: replay['u_info'] has shape (4,), expected (5,)", smoothing._two_filter_replay,
            {"u_info": np.zeros(4)}, P)
    _raises("two-filter smoothing: replay['idx_fwd'] and replay['idx_info'] are given together",
            smoothing._two_filter_replay, {"idx_fwd": np.zeros(P)}, P)
    out = smoothing._two_filter_replay({"idx_fwd": np.zeros(P), "idx_info": np.ones(P)}, P)
    assert out["idx_info"].dtype == I64 and out["u_fwd"] is None and out["u_info"] is None


def test_qmc_points_messages():
    _raises("backward sampling: M must be at least 1", smoothing._qmc_points, 0, 0, None, {"zz": 1})
    _raises("backward sampling: no step has run yet", smoothing._qmc_points, M, 0, None, {"zz": 1})
    _raises("backward sampling: unknown replay tape(s) ['zz']", smoothing._qmc_points, M, T, None, {"zz": 1})
    _raises("backward sampling: replay['u'] has shape (4, 3), expected (3, 4)", smoothing._qmc_points, M, T, None,
            {"u": np.zeros((T, M))})
    u = smoothing._qmc_points(M, T, None, {"u": np.asfortranarray(np.full((M, T), 0.25))})
    assert u.flags["C_CONTIGUOUS"] and u.shape == (M, T) and np.all(u == 0.25)


def test_backward_messages():
    h = _history()
    _raises("backward sampling: unknown replay tape(s) ['u_acc', 'u_prop']", h._backward, _lib.BACKWARD_ON2, M, 1, 1, 0,
            {"u_prop": 1, "u_acc": 1}, False)
    _raises("backward sampling: unknown replay tape(s) ['u']", h._backward, _lib.BACKWARD_MCMC, M, NS, 1, 0, {"u": 1}, False)
    _raises("backward sampling: replay['u'] has shape (3, 4), expected (3, 3)", h._backward, _lib.BACKWARD_ON2, M, 1, 1, 0,
            {"u": np.zeros((T - 1, M + 1))}, False)
    _raises("backward sampling: replay['u_acc'] has shape (3, 3), expected (3, 2, 3)", h._backward, _lib.BACKWARD_MCMC,
            M, NS, 1, 0, {"u_acc": np.zeros((T - 1, M))}, False)
    _raises("backward sampling: replay['idx_last'] has shape (2,), expected (3,)", h._backward, _lib.BACKWARD_REJECT,
            M, NS, 1, 0, {"idx_last": np.zeros(2), "u": np.zeros(1)}, False)


def test_one_launch_answers_none():
    h = _history()
    assert h._one_launch(1, 0, {"u_prop": np.zeros(1)}, False) is None          # a name of the general route
    assert h._one_launch(1, 0, {"u": np.zeros((T - 1, 2))}, False) is None        # a shape of the general route
    assert h._one_launch(1, 0, {"u_last": np.zeros(2)}, False) is None
    assert h._one_launch(1, C, None, False) is None                             # no such island
    assert _history(_n=0)._one_launch(1, 0, None, False) is None


def test_paris_messages():
    smc = types.SimpleNamespace(t=7, N=M, fk=types.SimpleNamespace(upper_bound_trans=lambda t: 0.5))
    p = collectors.Paris(Nparis=1, max_trials=NS, seed=3, replay=lambda t: {"u_acc": np.zeros((NS, M + 1))})
    _raises("Paris: replay(7)['u_acc'] has shape (2, 4), expected (2, 3)", p._device_extra, smc)
    # a name it does not know is ignored
    p = collectors.Paris(Nparis=1, max_trials=NS, seed=3, replay=lambda t: {"zz": 1, "u": np.arange(M)})
    out = p._device_extra(smc)
    assert out[:4] == (1, NS, 3, 0.5) and out[4] is None and out[5] is None and out[7] is False
    assert out[6].dtype == F64 and np.array_equal(out[6], np.arange(M))
    assert collectors.Paris(Nparis=1, max_trials=NS, seed=3)._device_extra(smc)[4:7] == (None, None, None)


def test_new_paths_messages():
    pf = _fake_filter()
    _raises("new_paths: unknown replay tape(s) ['u_prop']", mcmc.new_paths, pf, True, 1, {"u_prop": 1})
    _raises("new_paths: replay['u_last'] has shape (3,), expected (2,)", mcmc.new_paths, pf, True, 1,
            {"u_last": np.zeros(3)})
    _raises("new_paths: replay['u'] has shape (3, 1), expected (3, 2)", mcmc.new_paths, pf, True, 1,
            {"u": np.zeros((T - 1, 1))})
    _raises("new_paths: no step has run yet", mcmc.new_paths, _fake_filter(_n=0), True, 1, {"u": np.zeros((0, C))})


# ---- the kind table and the small idioms ------------------------------------------------------------------------------

def test_device_kinds():
    assert smoothing.DEVICE_KINDS == (_lib.MODEL_LINGAUSS, _lib.MODEL_STOCHVOL, _lib.MODEL_GORDON,
                                      _lib.MODEL_THETALOGISTIC, _lib.MODEL_DISCRETECOX)
    fk = lambda model: types.SimpleNamespace(_device_model=lambda: model)
    for kind in smoothing.DEVICE_KINDS:
        assert smoothing.device_model(fk({"kind": kind}))["kind"] == kind
    for kind in (_lib.MODEL_SVLEVERAGE, _lib.MODEL_MVLINGAUSS):
        assert smoothing.device_model(fk({"kind": kind})) is None
    assert smoothing.device_model(fk(None)) is None and smoothing.device_model(object()) is None


def test_seed_and_pointer_helpers():
    assert _lib.u64_seed(5) == 5 and _lib.u64_seed(-1) == 2 ** 64 - 1 and _lib.u64_seed(2 ** 64 + 3) == 3
    np.random.seed(11)
    a, b = _lib.u64_seed(None), _lib.u64_seed(None)
    assert a != b and 0 <= a < 2 ** 31 and pa.core._default_seed is _lib._default_seed
    assert _lib.hptr(None, _lib.c_dbl) is None
    x = np.arange(3.0)
    assert _lib.hptr(x, _lib.c_dbl)[2] == 2.0


def test_lazy_views():
    smc = types.SimpleNamespace(_n=5)
    steps, orders = smoothing._LazySteps(smc, lambda t: t), smoothing._LazyOrders(smc, lambda t: t)
    win = smoothing._Window(types.SimpleNamespace(T=3, _smc=smc), lambda t: t)
    assert list(steps) == [0, 1, 2, 3, 4] and list(orders) == [0, 1, 2, 3] and list(win) == [2, 3, 4]
    assert steps[-1] == 4 and orders[-1] == 3 and win[-1] == 4 and win[0] == 2 and win[1:] == [3, 4] and steps[::2] == [0, 2, 4]
    for view, n in ((steps, 5), (orders, 4), (win, 3)):
        assert len(view) == n
        for i in (n, -n - 1):
            with pytest.raises(IndexError, match="history index out of range"):
                view[i]
