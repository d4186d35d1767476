"""Side-cars of the SMC step that must keep working on the device path:
``Summaries`` / ``Collector`` / default collectors ``ESSs, LogLts, Rs_flags``
and ``Moments`` (particles/collectors.py:215-317), and the history containers
the step saves into (particles/smoothing.py:164-255).
"""
from collections import deque

import numpy as np

from . import _lib


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


# ---- history containers (smoothing.py:141-255) -----------------------------

def generate_hist_obj(option, smc):
    if option is True:
        return ParticleHistory(smc.fk, smc.qmc)
    if option is False:
        return None
    if callable(option):
        return PartialParticleHistory(option)
    if isinstance(option, int) and option >= 0:
        return RollingParticleHistory(option)
    raise ValueError("store_history: invalid option")


class PartialParticleHistory:
    def __init__(self, func):
        self.is_save_time = func
        self.X, self.wgts = {}, {}

    def save(self, smc):
        t = smc.t
        if self.is_save_time(t):
            self.X[t] = smc.X
            self.wgts[t] = _frozen_weights(smc.wgts)


class RollingParticleHistory:
    def __init__(self, length):
        self.X = deque([], length)
        self.A = deque([], length)
        self.wgts = deque([], length)

    @property
    def N(self):
        return self.X[0].shape[0]

    @property
    def T(self):
        return len(self.X)

    def save(self, smc):
        self.X.append(smc.X)
        self.A.append(smc.A)
        self.wgts.append(_frozen_weights(smc.wgts))

    def compute_trajectories(self):
        """(T, N) genealogy (smoothing.py:209-219)."""
        Bs = [np.arange(self.N)]
        for A in list(self.A)[-1:0:-1]:
            Bs.append(A[Bs[-1]])
        Bs.reverse()
        return np.array(Bs)


class ParticleHistory(RollingParticleHistory):
    def __init__(self, fk, qmc):
        self.X, self.A, self.wgts = [], [], []
        self.fk = fk
        self.qmc = bool(qmc)

    def backward_sampling_ON2(self, M, **kw):
        """Backward sampling runs on the device-resident history of a fused filter
        (``DeviceParticleHistory``); a history kept on the host has no sampler."""
        if self.qmc:
            raise ValueError("backward sampling: SQMC filters are not supported (backward_sampling_qmc "
                             "is a different algorithm)")
        raise NotImplementedError("backward sampling needs the device-resident history of a fused filter")

    def backward_sampling_mcmc(self, M, nsteps=1, **kw):
        return self.backward_sampling_ON2(M, **kw)

    def backward_sampling_reject(self, M, max_trials=None, **kw):
        return self.backward_sampling_ON2(M, **kw)


class _LazySteps:
    """Sequence over the steps run so far whose items are fetched from the device
    history on access."""

    def __init__(self, smc, fetch):
        self._smc, self._fetch = smc, fetch

    def __len__(self):
        return self._smc._n

    def __getitem__(self, t):
        n = len(self)
        if isinstance(t, slice):
            return [self[i] for i in range(*t.indices(n))]
        if t < 0:
            t += n
        if not 0 <= t < n:
            raise IndexError("history index out of range")
        return self._fetch(t)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class DeviceParticleHistory:
    """``ParticleHistory`` (smoothing.py:222-255: ``X``, ``A``, ``wgts`` of every
    step, ``compute_trajectories``) of a fused run: the history never leaves HBM
    until an item is read -- the device step loop writes step t into slot t of
    (T, N[, d]) arrays (``keep_history``), so ``save`` has nothing to do and
    ``SMC.run`` keeps its single asynchronous launch sequence."""

    def __init__(self, smc):
        self._smc = smc
        self.fk = smc.fk
        # (bound methods, not lambdas: the history object pickles with its filter)
        self.X = _LazySteps(smc, self._X_at)
        # hist.A[0] is the A of a filter that has not resampled yet: None (core.py:229)
        self.A = _LazySteps(smc, self._A_at)
        self.wgts = _LazySteps(smc, self._wgts_at)

    def _X_at(self, t):
        return self._smc._history(_lib.FIELD_X, t)

    def _A_at(self, t):
        return self._smc._history(_lib.FIELD_A, t) if t else None

    def _wgts_at(self, t):
        smc = self._smc
        f = _Frozen()
        f.lw = smc._history(_lib.FIELD_LW, t)
        f.W = smc._history(_lib.FIELD_W, t)
        s = smc._summ()[0, t]
        f.ESS, f.log_mean = float(s[0]), float(s[1])
        f.N = smc.N
        return f

    @property
    def N(self):
        return self._smc.N

    @property
    def T(self):
        return self._smc._n

    def save(self, smc):            # the device already did
        pass

    def compute_trajectories(self):
        """(T, N) genealogy (smoothing.py:209-219), computed on the device."""
        return self._smc._trajectories()

    def extract_one_trajectory(self):
        """A single trajectory (smoothing.py:256-269): the final state is drawn from the final
        weights, its line of ancestors is followed back on the device."""
        from . import resampling as rs
        smc = self._smc
        n = rs.multinomial_once(smc._history(_lib.FIELD_W, smc._n - 1))
        d = getattr(smc, "_d", 1)
        out = np.empty((smc._n, d))
        _lib.check(_lib.lib().smc_filter_one_trajectory(smc._f, 0, n, out.ctypes.data_as(
            _lib.P(_lib.c_dbl))))
        return [row[0] if d == 1 else row.copy() for row in out]

    def backward_sampling_ON2(self, M, seed=None, island=0, replay=None, return_idx=False):
        """Exact FFBS (smoothing.py:291-311), on the device: M trajectories, each step of each drawn
        from ``exp_and_normalise(lw_t + logpt(t + 1, X_t, x_{t+1}))`` -- O(N) work per trajectory
        and step, one workgroup per trajectory (a trajectory's N particles are not split over
        workgroups: M = 1 at large N runs on one compute unit).

        Returns the reference's list of T arrays ``paths[t]`` of shape (M,) (scalars for M = 1);
        with ``return_idx`` also the (T, M) array of particle indices.  The last row holds M iid
        draws from the final weights in draw order -- the reference's ``rs.multinomial(W, M)``
        returns them sorted: the same set of trajectories in law, another order.

        seed : Philox key of the draws (stream 3, counter (m, t, island, 3)); None: a fresh one,
            derived like the filter's default seed.
        replay : dict of uniforms to use instead: ``idx_last`` (M,) int64 or ``u_last`` (M,) for the
            last row, ``u`` (T-1, M) for the backward steps.
        """
        return self._backward(_lib.BACKWARD_ON2, M, 1, seed, island, replay, return_idx)

    def backward_sampling_mcmc(self, M, nsteps=1, seed=None, island=0, replay=None, return_idx=False):
        """MCMC backward sampling (smoothing.py:313-350; Dau & Chopin 2022), on the device: each
        trajectory starts a step from the ancestor of its particle and makes ``nsteps`` independent
        Metropolis steps whose proposals are iid draws from W_t -- O(nsteps) work per trajectory and
        step after one O(N) pass that forms the CDF of W_t.  Returns what ``backward_sampling_ON2``
        returns.  The proposals have the law of the reference's ``multinomial_iid``; its NumPy
        permutation stream is not reproduced.

        replay : ``idx_last`` / ``u_last`` as for ON2, ``u_prop`` and ``u_acc`` (T-1, nsteps, M).
        """
        return self._backward(_lib.BACKWARD_MCMC, M, nsteps, seed, island, replay, return_idx)

    def backward_sampling_reject(self, M, max_trials=None, seed=None, island=0, replay=None, return_idx=False):
        """Hybrid rejection backward sampling (smoothing.py:352-423; Dau & Chopin 2022), on the device: per
        trajectory and step at most ``max_trials`` rejection trials -- a proposal drawn from W_t is accepted with
        probability p_{t+1}(x_{t+1} | proposal) / C_{t+1} -- then the exact draw of ``backward_sampling_ON2`` for
        whatever is left.  The law is exactly the FFBS law; the expected cost per trajectory and step is O(1)
        where the bound is not loose.  ``log C_t`` is ``fk.upper_bound_trans(t)``, evaluated on the host: the
        stock univariate Gaussian models define it, a subclass may override ``upper_bound_log_pt``.

        max_trials : None: M (the reference's default).  Held to 2**24 - 1: "pure rejection" (``inf``) is served
            as that many trials followed by the exact draw, which is still the exact law.
        seed : Philox key: trial i of trajectory m at step t draws from counter (m, t, island, 4 | i << 8), the
            last row and the exact draws from stream 3 as ``backward_sampling_ON2``.
        replay : ``idx_last`` / ``u_last`` as for ON2, ``u_prop`` and ``u_acc`` (T-1, max_trials, M) for the trials,
            ``u`` (T-1, M) for the exact draws.

        Returns what ``backward_sampling_ON2`` returns and sets ``acc_rate`` (T-1,) = (M - nexact) / nprops
        (smoothing.py:422), ``nprops`` (trials made) and ``nexact`` (trajectories drawn exactly) per step.
        The proposals have the law of the reference's ``MultinomialQueue`` draws; its NumPy permutation stream
        is not reproduced.
        """
        if max_trials is None:
            max_trials = M
        max_trials = int(min(max_trials, _lib.REJECT_MAX_TRIALS))
        return self._backward(_lib.BACKWARD_REJECT, M, max_trials, seed, island, replay, return_idx)

    def _backward(self, method, M, nsteps, seed, island, replay, return_idx):
        """``nsteps``: Metropolis steps (MCMC) or max_trials (rejection)."""
        smc = self._smc
        M, nsteps, T = int(M), int(nsteps), smc._n
        if seed is None:
            from .core import _default_seed
            seed = _default_seed()
        replay = dict(replay or {})
        on2, reject = method == _lib.BACKWARD_ON2, method == _lib.BACKWARD_REJECT
        shape = (max(T - 1, 0), M) if on2 else (max(T - 1, 0), nsteps, M)
        names = {"idx_last": ((M,), np.int64), "u_last": ((M,), np.float64),
                 ("u" if on2 else "u_prop"): (shape, np.float64)}
        if not on2:
            names["u_acc"] = (shape, np.float64)
        if reject:
            names["u"] = ((max(T - 1, 0), M), np.float64)
        unknown = set(replay) - set(names)
        if unknown:
            raise ValueError("backward sampling: unknown replay tape(s) %s" % sorted(unknown))
        tapes = {}
        for k, (shp, dt) in names.items():
            if replay.get(k) is None:
                tapes[k] = None
                continue
            a = np.ascontiguousarray(replay[k], dtype=dt)
            if M >= 1 and nsteps >= 1 and a.shape != shp:
                raise ValueError("backward sampling: replay[%r] has shape %s, expected %s" % (k, a.shape, shp))
            tapes[k] = a
        ptr = lambda a, ct: a.ctypes.data_as(_lib.P(ct)) if a is not None else None
        idx = np.empty((T, max(M, 0)), dtype=np.int64)
        paths = np.empty((T, max(M, 0)))
        seed = int(seed) & (2 ** 64 - 1)
        last = (ptr(tapes["idx_last"], _lib.c_i64), ptr(tapes["u_last"], _lib.c_dbl))
        out = (ptr(idx, _lib.c_i64), ptr(paths, _lib.c_dbl))
        try:
            if reject:
                log_bound = np.array([self.fk.upper_bound_trans(s) for s in range(1, T)], dtype=np.float64).reshape(-1)
                nprops, nexact = np.zeros(max(T - 1, 0), dtype=np.int64), np.zeros(max(T - 1, 0), dtype=np.int64)
                _lib.check(_lib.lib().smc_filter_backward_reject(
                    smc._f, int(island), M, nsteps, seed, ptr(log_bound, _lib.c_dbl), *last,
                    ptr(tapes["u_prop"], _lib.c_dbl), ptr(tapes["u_acc"], _lib.c_dbl), ptr(tapes["u"], _lib.c_dbl),
                    *out, ptr(nprops, _lib.c_i64), ptr(nexact, _lib.c_i64)))
                self.nprops, self.nexact = nprops, nexact
                self.acc_rate = (M - nexact) / nprops
            else:
                _lib.check(_lib.lib().smc_filter_backward_sample(
                    smc._f, int(island), method, M, nsteps, seed, *last,
                    ptr(tapes.get("u", tapes.get("u_prop")), _lib.c_dbl), ptr(tapes.get("u_acc"), _lib.c_dbl), *out))
        except ValueError as e:
            if "model kind" in str(e):
                raise NotImplementedError(str(e)) from None
            raise
        out = [paths[t, 0] if M == 1 else paths[t].copy() for t in range(T)]      # (_output_backward_sampling)
        return (out, idx) if return_idx else out


class DeviceRollingParticleHistory:
    """``RollingParticleHistory`` (smoothing.py:186-219) of a fused run: the k most recent
    particle systems stay in a ring of k slots in HBM (``keep_history = k``), the step loop writes
    them there, ``save`` has nothing to do.  ``X``, ``A``, ``wgts`` behave like the reference's
    deques: index 0 is the oldest resident step, -1 the newest."""

    def __init__(self, smc, length):
        self._smc, self.length = smc, int(length)
        self.fk = smc.fk
        self.X = _Window(self, self._X_at)
        self.A = _Window(self, self._A_at)
        self.wgts = _Window(self, self._wgts_at)

    def _X_at(self, t):
        return self._smc._history(_lib.FIELD_X, t)

    def _wgts_at(self, t):
        return DeviceParticleHistory._wgts_at(self, t)

    def _A_at(self, t):
        smc = self._smc
        if t == 0:
            return None                                    # core.py:229: no ancestors at t = 0
        if t - 1 < smc._n - self.length:                   # its parents' step has left the window:
            s = smc._summ()[0, t]                          # the indices themselves are still there
            if not s[4]:
                return np.arange(smc.N)
        return smc._history(_lib.FIELD_A, t)

    @property
    def N(self):
        return self._smc.N

    @property
    def T(self):
        return min(self._smc._n, self.length)

    def save(self, smc):
        pass

    def compute_trajectories(self):
        """(T, N) genealogy of the resident steps (smoothing.py:209-219), on the device."""
        out = np.empty((self.T, self.N), dtype=np.int64)
        _lib.check(_lib.lib().smc_filter_trajectories(self._smc._f, 0, out.ctypes.data_as(_lib.P(_lib.c_i64))))
        return out


class _Window:
    """deque-like view of the resident steps of a rolling device history."""

    def __init__(self, hist, fetch):
        self._h, self._fetch = hist, fetch

    def __len__(self):
        return self._h.T

    def __getitem__(self, i):
        n = len(self)
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(n))]
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("history index out of range")
        return self._fetch(self._h._smc._n - n + i)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class _Frozen:
    pass


def _frozen_weights(w):
    """Copy-on-save: the device double-buffers its arrays, so a saved history
    entry must own host copies (the reference stores references,
    smoothing.py:204-207)."""
    f = _Frozen()
    f.lw, f.W, f.ESS, f.log_mean = w.lw, w.W, w.ESS, w.log_mean
    f.N = w.N
    return f
