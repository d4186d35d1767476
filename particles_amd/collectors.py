"""Counterpart of ``particles.collectors``, the side-cars of the SMC step that must keep working on the device path:
``Summaries`` / ``Collector`` / default collectors ``ESSs, LogLts, Rs_flags`` and ``Moments``
(particles/collectors.py:215-317), and the on-line smoothers ``Online_smooth_naive, Online_smooth_ON2, Paris``
(:345-449).  The history containers and the off-line smoothers are in ``smoothing.py``, as in the reference; their
public names stay importable from here.
"""
import ctypes

import numpy as np

from . import _lib
from . import smoothing
from .smoothing import (generate_hist_obj, PartialParticleHistory, RollingParticleHistory, ParticleHistory,  # noqa: F401
                        DeviceParticleHistory, DeviceRollingParticleHistory,
                        _Frozen)     # (_Frozen: tests/two_filter_cases.py builds host history entries as col._Frozen())
from .smoothing import _ON2_CHUNK_ELEMS, _all_pairs, _exp_and_normalise_cols


class Summaries:
    """Stores and updates summaries (collectors.py:215-231)."""

    def __init__(self, cols):
        self._collectors = [cls() for cls in default_collector_cls]
        if cols is not None:
            self._collectors.extend(col() for col in cols)
        for col in self._collectors:
            setattr(self, col.summary_name, col.summary)

    def collect(self, smc):
        for col in self._collectors:
            col.collect(smc)

    def _extend_defaults(self, ess, logLt, flags):
        """Bulk append of the three default summaries after a device-resident
        run (the values were kept per step in the device ring buffer)."""
        self.ESSs.extend(float(v) for v in ess)
        self.logLts.extend(float(v) for v in logLt)
        self.rs_flags.extend(bool(v) for v in flags)


    def _extend_moments(self, moms):
        """Bulk append for ``Moments`` collectors evaluated on the device."""
        for col in self._collectors:
            if isinstance(col, Moments):
                col.summary.extend(moms)


class Collector:
    """Base class for collectors (collectors.py:234-271)."""

    signature = {}

    @property
    def summary_name(self):
        cn = self.__class__.__name__
        return cn[0].lower() + cn[1:]

    def __init__(self, **kwargs):
        self.summary = []
        for k, v in self.signature.items():
            setattr(self, k, v)
        for k, v in kwargs.items():
            if k in self.signature.keys():
                setattr(self, k, v)
            else:
                raise ValueError(f"Collector {self.__class__.__name__}: unknown parameter {k}")

    def __call__(self):
        return self.__class__(**{k: getattr(self, k) for k in self.signature.keys()})

    def collect(self, smc):
        self.summary.append(self.fetch(smc))


class ESSs(Collector):
    summary_name = "ESSs"

    def fetch(self, smc):
        return smc.wgts.ESS


class LogLts(Collector):
    def fetch(self, smc):
        return smc.logLt


class Rs_flags(Collector):
    def fetch(self, smc):
        return smc.rs_flag


default_collector_cls = [ESSs, LogLts, Rs_flags]


class Moments(Collector):
    """Empirical moments of the particles (collectors.py:301-317); the default
    is the weighted mean and variance, evaluated on the device."""

    signature = {"mom_func": None}

    def fetch(self, smc):
        f = smc.fk.default_moments if self.mom_func is None else self.mom_func
        return f(smc.W, smc.X)


# ---- on-line smoothing (collectors.py:345-449; book 11.1, 11.3) ---------------------------------------------

class _OnlineSmoother(Collector):
    """What the three on-line smoothers share.  ``fetch`` appends ``np.average(Phi, axis=0, weights=W_t)`` and keeps
    ``Phi`` ((N,) for a scalar additive function, else (N, K)).

    On a fused filter (not SQMC) of a stock ``Bootstrap`` / ``GuidedPF`` over one of the univariate models backward
    sampling supports, with ``add_func`` a ``QuadAddFunc``, the update runs on the device behind the step just done
    (smc_filter_online_smooth): Phi and the previous step's X and lw stay in device arrays this object owns, and one
    estimate of K numbers comes back per step.  Everything else -- auxiliary filters, StochVolLeverage, multivariate
    models, SQMC, operator-path and user models, a Python ``add_func`` -- takes the NumPy route on ``smc.X``, ``smc.A``,
    ``smc.W``, ``smc.wgts.lw`` and ``smc.fk.logpt`` / ``add_func``.  Island 0 is what a collector sees."""

    _method = None

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._route = None          # "device" / "host", decided at the first step
        self._dev = None            # (Phi, Xprev, lwprev) DeviceArrays
        self._host = None           # {"Phi", "X", "lw", "W"} NumPy arrays
        self._t_next = 0
        self._psi = None

    # -- which route
    @staticmethod
    def _quad(fk):
        ssm_ = getattr(fk, "ssm", None)
        f = getattr(ssm_, "add_func", None)
        from .state_space_models import QuadAddFunc
        return f if isinstance(f, QuadAddFunc) else None

    def _on_device(self, smc):
        from . import state_space_models as ssm_mod
        fk = smc.fk
        if not getattr(smc, "_fused", False) or smc.qmc or self._quad(fk) is None:
            return False
        if getattr(fk, "_fk_kind", None) not in (_lib.FK_BOOTSTRAP, _lib.FK_GUIDED):
            return False
        if type(fk).add_func is not ssm_mod.Bootstrap.add_func:
            return False
        return smoothing.device_model(fk) is not None

    @property
    def Phi(self):
        if self._route == "device":
            a = self._dev[0].get()
            return a[:, 0] if self._psi.scalar else a
        return None if self._host is None else self._host["Phi"]

    def fetch(self, smc):
        if self._route is None:
            self._route = "device" if self._on_device(smc) else "host"
        if smc.t != self._t_next:
            raise RuntimeError("%s: collected at t = %d after t = %d -- the on-line recursion needs every step"
                               % (type(self).__name__, smc.t, self._t_next - 1))
        self._t_next = smc.t + 1
        return self._fetch_device(smc) if self._route == "device" else self._fetch_host(smc)

    # -- device route
    def _device_extra(self, smc):
        """(n_paris, max_trials, seed, log_bound, u_prop, u_acc, u, want_idx)"""
        return 1, 1, 0, 0.0, None, None, None, False

    def _fetch_device(self, smc):
        N = smc.N
        if self._dev is None:
            self._psi = self._quad(smc.fk)
            self._dev = (_lib.DeviceArray((N, self._psi.K)), _lib.DeviceArray((N,)), _lib.DeviceArray((N,)))
        K = self._psi.K
        n_paris, max_trials, seed, log_bound, u_prop, u_acc, u, want_idx = self._device_extra(smc)
        ptr = _lib.hptr
        est = np.empty(K)
        idx = np.empty((N, n_paris), dtype=np.int64) if want_idx and smc.t > 0 else None
        nprop = _lib.c_i64(0)
        f = self._psi._struct()
        _lib.check(_lib.lib().smc_filter_online_smooth(
            smc._f, 0, self._method, ctypes.byref(f), self._dev[0].ptr, self._dev[1].ptr, self._dev[2].ptr,
            int(n_paris), int(max_trials), _lib.u64_seed(seed), float(log_bound),
            ptr(u_prop, _lib.c_dbl), ptr(u_acc, _lib.c_dbl), ptr(u, _lib.c_dbl), ptr(idx, _lib.c_i64),
            ctypes.byref(nprop), ptr(est, _lib.c_dbl)))
        self._device_done(smc, idx, int(nprop.value))
        return est[0] if self._psi.scalar else est

    def _device_done(self, smc, idx, nprop):
        pass

    # -- host route
    def _fetch_host(self, smc):
        X = np.asarray(smc.X)
        if smc.t == 0:
            self._host = {"Phi": np.asarray(smc.fk.add_func(0, None, X), dtype=np.float64)}
        else:
            self._host["Phi"] = self._update_host(smc, X, self._host)
        W = np.asarray(smc.W)
        out = np.average(self._host["Phi"], axis=0, weights=W)
        self._host.update(X=X.copy(), lw=np.array(smc.wgts.lw, dtype=np.float64), W=W.copy())
        return out

    def _update_host(self, smc, X, prev):
        raise NotImplementedError

    @staticmethod
    def _pair_weights(smc, prev, xs):
        """(sources, len(xs)) normalised backward weights of the targets xs."""
        XP, XT = _all_pairs(prev["X"], xs)
        l = np.asarray(smc.fk.logpt(smc.t, XP, XT), dtype=np.float64).reshape(len(xs), -1).T
        return _exp_and_normalise_cols(prev["lw"][:, None] + l)

    @staticmethod
    def _psi_pairs(smc, prev, xs):
        """(sources, len(xs)[, K]) psi_t(X_{t-1}[m], xs[j])."""
        XP, XT = _all_pairs(prev["X"], xs)
        v =np.asarray(smc.fk.add_func(smc.t, XP, XT), dtype=np.float64)
        v = v.reshape((len(xs), len(prev["X"])) + v.shape[1:])
        return np.swapaxes(v, 0, 1)


class Online_smooth_naive(_OnlineSmoother):
    """Forward-only smoothing along the genealogy (collectors.py:368-370): O(N) per step, degenerates with t."""

    summary_name = "online_smooth_naive"
    _method = _lib.ONLINE_NAIVE

    def _update_host(self, smc, X, prev):
        A = smc.A
        A = np.arange(smc.N) if A is None else np.asarray(A)
        Xp = prev["X"][A]
        return prev["Phi"][A] + np.asarray(smc.fk.add_func(smc.t, Xp, X), dtype=np.float64)


class Online_smooth_ON2(_OnlineSmoother):
    """The O(N^2) forward recursion (collectors.py:373-387): every particle averages over all particles of the step
    before under the backward kernel.  On the device this is the all-pairs kernel k_os_on2."""

    summary_name = "online_smooth_ON2"
    _method = _lib.ONLINE_ON2

    def _update_host(self, smc, X, prev):
        N = smc.N
        Phi = np.empty_like(prev["Phi"])
        step = max(1, _ON2_CHUNK_ELEMS // (N * (Phi.shape[1] if Phi.ndim == 2 else 1)))
        for n0 in range(0, N, step):
            xs = X[n0:n0 + step]
            w = self._pair_weights(smc, prev, xs)                                   # (N, c)
            psi = self._psi_pairs(smc, prev, xs)                                    # (N, c[, K])
            if Phi.ndim == 1:
                Phi[n0:n0 + step] = np.sum(w * (prev["Phi"][:, None] + psi), axis=0)
            else:
                Phi[n0:n0 + step] = np.sum(w[:, :, None] * (prev["Phi"][:, None, :] + psi), axis=0)
        return Phi


class Paris(_OnlineSmoother):
    """The hybrid Paris algorithm (collectors.py:390-449; Olsson & Westerborn 2017, Dau & Chopin 2022): each
    particle draws ``Nparis`` ancestors from the backward kernel -- at most ``max_trials`` rejection trials with
    proposals from W_{t-1}, then the exact draw -- and averages over them.  ``max_trials=None`` means N; it is held
    to 2**24 - 1.  ``nprop[t]`` is the number of trials made at step t.

    seed : Philox key of the device route (streams 4 and 3, counters (n Nparis + r, t - 1, island, .)); None: a
        fresh key.  The host route draws from ``np.random`` as the reference does.
    replay : callable ``t -> dict`` of tapes ``u_prop``, ``u_acc`` (max_trials, N Nparis) and ``u`` (N Nparis,) to use
        instead (device route).
    return_idx : keep the (N, Nparis) indices of the last update in ``As``."""

    summary_name = "paris"
    signature = {"Nparis": 2, "max_trials": None}
    _method = _lib.ONLINE_PARIS

    def __init__(self, seed=None, replay=None, return_idx=False, **kwargs):
        super().__init__(**kwargs)
        self.seed, self.replay, self.return_idx = seed, replay, return_idx
        self.nprop = [0.0]
        self.As = None

    def __call__(self):
        return self.__class__(seed=self.seed, replay=self.replay, return_idx=self.return_idx,
                              **{k: getattr(self, k) for k in self.signature.keys()})

    def _trials(self, smc):
        m = smc.N if self.max_trials is None else self.max_trials
        return int(min(m, _lib.REJECT_MAX_TRIALS))

    def _device_extra(self, smc):
        if self.seed is None:
            self.seed = _lib._default_seed()
        if smc.t == 0:
            return int(self.Nparis), self._trials(smc), self.seed, 0.0, None, None, None, False
        M, mt = smc.N * int(self.Nparis), self._trials(smc)
        spec = {"u_prop": ((mt, M), np.float64), "u_acc": ((mt, M), np.float64), "u": ((M,), np.float64)}
        given = dict(self.replay(smc.t) or {}) if self.replay is not None else {}
        tapes = smoothing.read_tapes("Paris", {k: given[k] for k in spec if k in given}, spec, "replay(%d)" % smc.t)
        return (int(self.Nparis), mt, self.seed, float(smc.fk.upper_bound_trans(smc.t)), tapes["u_prop"], tapes["u_acc"],
                tapes["u"], bool(self.return_idx))

    def _device_done(self, smc, idx, nprop):
        if smc.t > 0:
            self.nprop.append(nprop)
            if self.return_idx:
                self.As = idx

    def _update_host(self, smc, X, prev):
        N, R, mt = smc.N, int(self.Nparis), self._trials(smc)
        logC = smc.fk.upper_bound_trans(smc.t)
        cs = np.cumsum(prev["W"])
        last = np.flatnonzero(prev["W"] > 0)[-1]
        As = np.full(N * R, -1, dtype=np.int64)
        target = np.repeat(np.arange(N), R)
        pending = np.arange(N * R)
        ntries = 0
        for _ in range(mt):
            if not len(pending):
                break
            prop = np.minimum(np.searchsorted(cs, np.random.rand(len(pending)) * cs[-1]), last)
            lp = np.asarray(smc.fk.logpt(smc.t, prev["X"][prop], X[target[pending]])) - logC
            ntries += len(pending)
            acc = np.log(np.random.rand(len(pending))) < lp
            As[pending[acc]] = prop[acc]
            pending = pending[~acc]
        for j in pending:                                        # out of trials: the exact draw
            w = self._pair_weights(smc, prev, X[target[j]:target[j] + 1])[:, 0]
            c = np.cumsum(w)
            As[j] = min(np.searchsorted(c, np.random.rand() * c[-1]), np.flatnonzero(w > 0)[-1])
        self.nprop.append(ntries)
        As = As.reshape(N, R)
        if self.return_idx:
            self.As = As
        Phi = np.zeros_like(prev["Phi"])
        for r in range(R):
            a = As[:, r]
            Phi = Phi + (prev["Phi"][a] + np.asarray(smc.fk.add_func(smc.t, prev["X"][a], X), dtype=np.float64))
        return Phi / R
