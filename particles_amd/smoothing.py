"""Counterpart of ``particles.smoothing``: the history containers the SMC step saves into (smoothing.py:141-255) and the
off-line smoothers on them -- backward sampling (FFBS: exact, MCMC, rejection, QMC; :291-456) and two-filter smoothing
(:487-575).  A fused filter keeps its history in HBM (``DeviceParticleHistory``, ``DeviceRollingParticleHistory``) and
the smoothers run there through ``smc_filter_backward_*`` / ``smc_filter_two_filter``; a history kept on the host takes
the NumPy route.  The on-line smoothers are collectors (``collectors.py``), as in the reference.
"""
import ctypes
from collections import deque

import numpy as np

from . import _lib

# The model kinds the smoothing kernels take: what sm_kind_ok of csrc/smc_filter.hip accepts, restated.
DEVICE_KINDS = (_lib.MODEL_LINGAUSS, _lib.MODEL_STOCHVOL, _lib.MODEL_GORDON, _lib.MODEL_THETALOGISTIC,
                _lib.MODEL_DISCRETECOX)

_ON2_CHUNK_ELEMS = 1 << 22          # host route: the (sources, targets) blocks of an O(N^2) update stay below this


def device_model(fk):
    """The device model of the Feynman-Kac object ``fk`` if the smoothing kernels take its kind, else None."""
    model = fk._device_model() if hasattr(fk, "_device_model") else None
    return model if model is not None and model["kind"] in DEVICE_KINDS else None


def read_tapes(who, replay, spec, subject="replay"):
    """The replay dict of a smoother as what the library reads.  spec: ``{name: (shape or None, dtype)}``.  Returns
    ``{name: C-contiguous array of dtype, or None where the tape is absent or None}``.  ValueError
    "<who>: unknown replay tape(s) [...]" for a name outside spec, "<who>: <subject>[<name>] has shape S, expected E"
    for a wrong shape; a shape of None is not checked."""
    replay = dict(replay or {})
    unknown = set(replay) - set(spec)
    if unknown:
        raise ValueError("%s: unknown replay tape(s) %s" % (who, sorted(unknown)))
    tapes = {}
    for name, (shape, dtype) in spec.items():
        a = replay.get(name)
        if a is not None:
            a = np.ascontiguousarray(a, dtype=dtype)
            if shape is not None and a.shape != shape:
                raise ValueError("%s: %s[%r] has shape %s, expected %s" % (who, subject, name, a.shape, shape))
        tapes[name] = a
    return tapes


def _check_kind(rc):
    """``_lib.check`` of a smoothing call: the library's refusal of a model kind is a NotImplementedError."""
    try:
        _lib.check(rc)
    except ValueError as e:
        if "model kind" in str(e):
            raise NotImplementedError(str(e)) from None
        raise


def _exp_and_normalise_cols(l):
    """Columns of l (sources, targets) as normalised weights; -inf and NaN weigh 0, a column without a finite entry
    is NaN (the reference's exp_and_normalise)."""
    l = np.where(np.isnan(l), -np.inf, l)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.exp(l - l.max(axis=0))
        return w / w.sum(axis=0)


def _all_pairs(sources, targets):
    """Every (source, target) pair as two flat arrays, target-major: model code (``logpt``, ``add_func``) is elementwise
    over particles, not a broadcasting function."""
    return (np.tile(sources, (len(targets),) + (1,) * (sources.ndim - 1)), np.repeat(targets, len(sources), axis=0))


# ---- two-filter smoothing (smoothing.py:487-575) -----------------------------

_TWO_FILTER_T_ERR = "two-filter smoothing: t must be in range 0,...,T-2"
_TWO_FILTER_TAPES = {"u_fwd": np.float64, "u_info": np.float64, "idx_fwd": np.int64, "idx_info": np.int64}


def _two_filter_replay(replay, P):
    """The replay dict of ``two_filter_smoothing`` as contiguous arrays (None where absent)."""
    tapes = read_tapes("two-filter smoothing", replay, {k: ((P,), dt) for k, dt in _TWO_FILTER_TAPES.items()})
    if (tapes["idx_fwd"] is None) != (tapes["idx_info"] is None):
        raise ValueError("two-filter smoothing: replay['idx_fwd'] and replay['idx_info'] are given together")
    return tapes


def _two_filter_phi(phi):
    """``phi(x, xf)`` of a ``QuadAddFunc``: its t >= 1 form, psi_t(xp, x) with xp = x and x = xf."""
    from .state_space_models import QuadAddFunc
    return (lambda x, xf: phi(1, x, xf)) if isinstance(phi, QuadAddFunc) else phi


def _inverse_cdf_draws(W, u):
    """Indices of the uniforms u in the cumulative sums of the weights W; a weightless particle is never drawn."""
    W = np.where(np.isnan(W), 0.0, W)
    cs = np.cumsum(W)
    top = int(np.flatnonzero(W > 0)[-1]) if cs[-1] > 0 else len(W) - 1
    return np.minimum(np.searchsorted(cs, u * cs[-1], side="right"), top).astype(np.int64)


def _two_filter_numpy(hist, t, info, phi, loggamma, linear_cost, return_ess, modif_forward, modif_info, npairs, seed,
                      replay, return_idx):
    """The NumPy route of ``two_filter_smoothing``: the two estimators on arrays read through ``hist.X[...]`` and
    ``hist.wgts[...]``, any callable ``phi(x, xf)`` and ``loggamma(x)``, ``fk.logpt`` on flat pair arrays (model code
    is elementwise over particles).  The O(N^2) form goes over the information filter's particles in chunks of at most
    ``_ON2_CHUNK_ELEMS`` pairs on one running maximum: never an N x N array.  A bound common to all pairs (the
    reference's ``upper_bound_trans``) cancels, so none is asked for."""
    T = hist.T
    if t < 0 or t >= T - 1:
        raise ValueError(_TWO_FILTER_T_ERR)
    ti = T - 2 - t
    fk = hist.fk
    phi = _two_filter_phi(phi)
    X, wf = np.asarray(hist.X[t]), hist.wgts[t]
    Xi = np.asarray(info.hist.X[ti])
    lw = np.asarray(wf.lw, dtype=np.float64)
    lwi = np.asarray(info.hist.wgts[ti].lw, dtype=np.float64) - np.asarray(loggamma(Xi), dtype=np.float64)
    Nf, Ni = len(X), len(Xi)
    if not linear_cost:
        G, A, B = -np.inf, 0.0, 0.0
        step = max(1, _ON2_CHUNK_ELEMS // Nf)
        for m0 in range(0, Ni, step):
            xs = Xi[m0:m0 + step]
            c = len(xs)
            XP, XT = _all_pairs(X, xs)
            l = np.asarray(fk.logpt(t + 1, XP, XT), dtype=np.float64).reshape(c, Nf) + lw[None, :] + lwi[m0:m0 + step, None]
            l = np.where(np.isnan(l), -np.inf, l)
            mx = l.max()
            if not mx > -np.inf:
                continue
            if mx > G:
                sc = np.exp(G - mx) if G > -np.inf else 0.0
                A, B, G = A * sc, B * sc, mx
            e = np.exp(l - G)
            ph = np.asarray(phi(XP, XT), dtype=np.float64)
            ph = ph.reshape((c, Nf) + ph.shape[1:])
            ph = np.where((e > 0).reshape((c, Nf) + (1,) * (ph.ndim - 2)), ph, 0.0)
            A = A + e.sum()
            B = B + np.tensordot(e, ph, axes=([0, 1], [0, 1]))
        with np.errstate(invalid="ignore", divide="ignore"):
            est = np.asarray(B, dtype=np.float64) / A if A > 0 else np.asarray(B, dtype=np.float64) * np.nan
        est = est[()] if np.ndim(est) == 0 else est
        # (the O(N^2) form has no ESS in the reference either: return_ess is the O(N) form's)
        return est
    P = int(Nf if npairs is None else npairs)
    if P < 1:
        raise ValueError("two-filter smoothing: npairs must be at least 1")
    tapes = _two_filter_replay(replay, P)
    mf = None if modif_forward is None else np.asarray(modif_forward, dtype=np.float64)
    mi = None if modif_info is None else np.asarray(modif_info, dtype=np.float64)
    if tapes["idx_fwd"] is not None:
        J, I = tapes["idx_fwd"], tapes["idx_info"]
        if J.min() < 0 or J.max() >= Nf or I.min() < 0 or I.max() >= Ni:
            raise ValueError("two-filter smoothing: pair index out of range")
    else:
        rng = np.random.default_rng(seed)
        u_f = tapes["u_fwd"] if tapes["u_fwd"] is not None else rng.random(P)
        u_i = tapes["u_info"] if tapes["u_info"] is not None else rng.random(P)
        W = np.asarray(wf.W) if mf is None else _exp_and_normalise_cols(lw + mf)
        J = _inverse_cdf_draws(W, u_f)
        I = _inverse_cdf_draws(_exp_and_normalise_cols(lwi if mi is None else lwi + mi), u_i)
    lo = np.asarray(fk.logpt(t + 1, X[J], Xi[I]), dtype=np.float64)
    if mf is not None:
        lo = lo - mf[J]
    if mi is not None:
        lo = lo - mi[I]
    Om = _exp_and_normalise_cols(lo)
    est = np.average(np.asarray(phi(X[J], Xi[I]), dtype=np.float64), axis=0, weights=Om)
    return _two_filter_result(est, 1.0 / np.sum(Om ** 2), J, I, return_ess, return_idx)


def _two_filter_result(est, ess, J, I, return_ess, return_idx):
    """What the O(N) form returns: ``est``, then ``ess`` and the pairs ``(J, I)`` where asked for."""
    out = (est, ess) if return_ess else (est,)
    if return_idx:
        out = out + (J, I)
    return out[0] if len(out) == 1 else out


_TWO_FILTER_DOC = """Two-filter smoothing (smoothing.py:487-575): the smoothing expectation of ``phi(X_t, X_{t+1})`` from this
        (forward) filter's history and the history of ``info``, the information filter -- the same model run on the
        reversed data under the pseudo-prior ``gamma``.  The first eight parameters are the reference's.

        t : 0 <= t <= T - 2
        info : the information filter (an ``SMC`` object run with ``store_history=True``); step ``T - 2 - t`` of it is read
        phi : ``phi(x, xf)`` of the forward particle and the information filter's; a ``QuadAddFunc`` stands for its
            t >= 1 form ``psi_t(xp, x)`` with xp = x and x = xf
        loggamma : ``loggamma(xf)``, the log-density of the pseudo-prior; ``QuadLogGamma`` in closed form
        linear_cost : the O(N) estimator (Fearnhead, Wyncoll & Tawn 2010) instead of the O(N^2) double sum
        return_ess : O(N) form: return ``(est, ess)``, ess = 1 / sum Om^2 of the pairs' weights
        modif_forward, modif_info : (N_f), (N_i) log-modifiers of the two sampling weights, O(N) form only (silently
            unused otherwise, as in the reference)
        npairs : pairs of the O(N) form; None: N of the forward filter (the reference draws N)
        seed, replay, return_idx : the O(N) draws: a key (Philox stream 5, counter (j, t, island, 5) on the device;
            NumPy's generator on the host route), or a dict with uniforms ``u_fwd``, ``u_info`` (npairs,) or given pairs
            ``idx_fwd``, ``idx_info`` (npairs,) int64; ``return_idx`` appends the pairs ``(J, I)`` to the result

        The pairs are iid, in draw order.  The reference draws I and J with ``rs.multinomial``, which returns each
        SORTED, and pairs them position by position: that is another coupling of the same two marginals -- both
        estimators are consistent, their values differ draw by draw.  Unlike the reference no ``upper_bound_log_pt`` is
        needed: a bound common to all pairs cancels.  A -inf or NaN pair weight counts as 0 (in the reference's O(N^2)
        loop a NaN poisons the sum).

        Returns a scalar for a scalar ``phi``, else (K,)."""

# ---- history containers (smoothing.py:141-255) -----------------------------


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


# (the reference's words, smoothing.py:271-276)
_QMC_FFBS_ERR = "QMC FFBS requires particles have been Hilbert ordered during the forward pass"


def _qmc_points(M, T, seed, replay):
    """The (M, T) point set of ``backward_sampling_qmc``: ``replay["u"]``, else ``rqmc.sobol_points(M, T, seed)``."""
    if M < 1:
        raise ValueError("backward sampling: M must be at least 1")
    if T < 1:
        raise ValueError("backward sampling: no step has run yet")
    u = read_tapes("backward sampling", replay, {"u": ((M, T), np.float64)})["u"]
    if u is None:
        from . import rqmc
        u = np.ascontiguousarray(rqmc.sobol_points(M, T, seed))
    return u


class ParticleHistory(RollingParticleHistory):
    def __init__(self, fk, qmc):
        self.X, self.A, self.wgts = [], [], []
        self.fk = fk
        self.qmc = bool(qmc)
        if qmc:
            self.h_orders = []           # h_orders[t] = hilbert_sort(X_t), t < T - 1 (smoothing.py:247-254)

    def save(self, smc):
        RollingParticleHistory.save(self, smc)
        if self.qmc and hasattr(smc, "h_order"):
            self.h_orders.append(smc.h_order)

    def backward_sampling_qmc(self, M, replay=None, seed=None, return_idx=False):
        """QMC backward sampling (smoothing.py:425-456) on a history kept on the host: the NumPy route, the reference's
        method line by line.  Returns its list of T arrays ``paths[t]`` of shape (M,); with ``return_idx`` also the (T, M)
        int64 particle indices.

        replay : ``{"u": (M, T)}`` supplies the points; otherwise ``rqmc.sobol_points(M, T, seed)``."""
        if not hasattr(self, "h_orders"):
            raise ValueError(_QMC_FFBS_ERR)
        from . import hilbert
        M, T = int(M), self.T
        u = _qmc_points(M, T, seed, replay)
        host = lambda a: np.asarray(a.get() if isinstance(a, _lib.DeviceArray) else a)
        X = [host(x) for x in self.X]
        hT = host(hilbert.hilbert_sort(X[-1])).astype(np.int64)
        idx = np.empty((T, M), dtype=np.int64)
        pos = np.searchsorted(np.cumsum(host(self.wgts[-1].W)[hT]), u[:, -1])
        idx[-1] = hT[pos]
        paths = [X[-1][hT][pos]]
        for t in reversed(range(T - 1)):
            h = host(self.h_orders[t]).astype(np.int64)
            lw = host(self.wgts[t].lw)
            pos = np.empty(M, dtype=np.int64)
            for m, xn in enumerate(paths[-1]):
                lwm = lw + host(self.fk.logpt(t + 1, X[t], np.full(X[t].shape, xn)))
                cw = np.cumsum(_exp_and_normalise_cols(lwm[h]))      # use ordered version here
                pos[m] = np.searchsorted(cw, u[m, t])
            idx[t] = h[pos]
            paths.append(X[t][h][pos])
        paths.reverse()
        return (paths, idx) if return_idx else paths

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

    def two_filter_smoothing(self, t, info, phi, loggamma, linear_cost=False, return_ess=False, modif_forward=None,
                             modif_info=None, npairs=None, seed=None, replay=None, return_idx=False):
        return _two_filter_numpy(self, t, info, phi, loggamma, linear_cost, return_ess, modif_forward, modif_info, npairs,
                                 seed, replay, return_idx)

    two_filter_smoothing.__doc__ = _TWO_FILTER_DOC + """
        A history kept on the host takes the NumPy route."""


class _LazySeq:
    """Sequence over steps of a device history whose items are fetched on access.  A subclass says how many steps are
    visible (``__len__``) and which absolute step its index i means (``_step``)."""

    def __init__(self, owner, fetch):
        self._owner, self._fetch = owner, fetch

    def _step(self, i):
        return i

    def __getitem__(self, i):
        n = len(self)
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(n))]
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("history index out of range")
        return self._fetch(self._step(i))

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class _LazySteps(_LazySeq):
    """... over the steps a filter (the owner) has run so far."""

    def __len__(self):
        return self._owner._n


class _LazyOrders(_LazySeq):
    """... over all steps but the last: the reference saves the order of X_t when step t + 1 resamples."""

    def __len__(self):
        return max(self._owner._n - 1, 0)


class _Window(_LazySeq):
    """deque-like view of the resident steps of a rolling device history (the owner)."""

    def __len__(self):
        return self._owner.T

    def _step(self, i):
        return self._owner._smc._n - len(self) + i


def _wgts_at(smc, t):
    """``wgts[t]`` of a device history: the weights of step t of island 0 and their summary."""
    f = _Frozen()
    f.lw = smc._history(_lib.FIELD_LW, t)
    f.W = smc._history(_lib.FIELD_W, t)
    s = smc._summ()[0, t]
    f.ESS, f.log_mean = float(s[0]), float(s[1])
    f.N = smc.N
    return f


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
        if smc.qmc:
            # h_orders[t] = hilbert_sort(X_t), t < T - 1 (smoothing.py:247-254), sorted on the device when read
            self.h_orders = _LazyOrders(smc, self._h_order_at)

    def _X_at(self, t):
        return self._smc._history(_lib.FIELD_X, t)

    def _A_at(self, t):
        return self._smc._history(_lib.FIELD_A, t) if t else None

    def _wgts_at(self, t):
        return _wgts_at(self._smc, t)

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
        _lib.check(_lib.lib().smc_filter_one_trajectory(smc._f, 0, n, _lib.hptr(out, _lib.c_dbl)))
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
        if int(M) == 1 and getattr(self._smc, "_cond_device", False):
            out = self._one_launch(seed, island, replay, return_idx)
            if out is not None:
                return out
        return self._backward(_lib.BACKWARD_ON2, M, 1, seed, island, replay, return_idx)

    def _one_launch(self, seed, island, replay, return_idx):
        """``backward_sampling_ON2(1)`` on a conditional filter (``mcmc.CSMC``): the launch that walks every island's
        history at once (smc_filter_csmc_paths) -- the same indices from the same uniforms.  None: arguments the
        general route takes (or refuses)."""
        smc = self._smc
        C, T = smc.n_islands, smc._n
        if T < 1 or not 0 <= int(island) < C or set(replay or {}) - {"u_last", "u"}:
            return None
        try:
            mine = read_tapes("backward sampling", replay, {"u_last": ((1,), np.float64), "u": ((T - 1, 1), np.float64)})
        except ValueError:
            return None
        tapes = {}
        for k, a in mine.items():
            if a is not None:
                tapes[k] = np.full(a.shape[:-1] + (C,), 0.5)      # (the other islands' draws are not handed out)
                tapes[k][..., int(island)] = a[..., 0]
        from .mcmc import new_paths
        paths, idx = new_paths(smc, True, seed, tapes, True)
        out = [paths[int(island), t] for t in range(T)]
        return (out, idx[int(island)].reshape(T, 1).copy()) if return_idx else out

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

    _GEOMETRIES = {None: 0, "auto": 0, 0: 0, "workgroup": 1, 1: 1, "thread": 2, 2: 2}

    def backward_sampling_qmc(self, M, seed=None, island=0, replay=None, return_idx=False, geometry=None):
        """QMC backward sampling (smoothing.py:425-456) of an SQMC filter, on the device: exact FFBS whose M x T uniforms
        are one randomised Sobol' point set and whose every inverse-CDF lookup is made in the Hilbert order of its
        step's particles (smc_filter_backward_qmc; per step one radix sort and one gather, never T sorted copies).

        Returns the reference's list of T arrays ``paths[t]`` of shape (M,) (not squeezed for M = 1, as the reference's
        method does not); with ``return_idx`` also the (T, M) int64 particle indices.

        seed : of ``rqmc.sobol_points(M, T, seed)``, the host-generated point set; None: a fresh one.
        replay : ``{"u": (M, T)}`` supplies the points, row m the point of trajectory m.
        geometry : None / "auto" picks by M; "workgroup" (1) one workgroup per trajectory, "thread" (2) one thread per
            trajectory -- the same indices either way.
        """
        smc = self._smc
        if not smc.qmc:
            raise ValueError(_QMC_FFBS_ERR)
        if geometry not in self._GEOMETRIES and not isinstance(geometry, int):
            raise ValueError("backward sampling: unknown geometry %r" % (geometry,))
        M, T = int(M), smc._n
        u = _qmc_points(M, T, seed, replay)
        idx = np.empty((T, M), dtype=np.int64)
        paths = np.empty((T, M))
        _check_kind(_lib.lib().smc_filter_backward_qmc(
            smc._f, int(island), M, int(self._GEOMETRIES.get(geometry, geometry)), _lib.hptr(u, _lib.c_dbl),
            _lib.hptr(idx, _lib.c_i64), _lib.hptr(paths, _lib.c_dbl)))
        out = [paths[t].copy() for t in range(T)]
        return (out, idx) if return_idx else out

    def _h_order_at(self, t):
        from . import hilbert
        if t >= self._smc._n - 1:
            raise IndexError("history index out of range")
        h = hilbert.hilbert_sort(_lib.DeviceArray.from_numpy(self._smc._history(_lib.FIELD_X, t)))
        return np.asarray(h.get() if isinstance(h, _lib.DeviceArray) else h, dtype=np.int64)

    def _two_filter_on_device(self, info, phi, loggamma):
        from .state_space_models import QuadAddFunc, QuadLogGamma
        smc, other = self._smc, info
        if not isinstance(getattr(other, "hist", None), DeviceParticleHistory):
            return False
        if smc.qmc or other.qmc or not getattr(smc, "_fused", False) or not getattr(other, "_fused", False):
            return False
        if not isinstance(phi, QuadAddFunc) or not isinstance(loggamma, QuadLogGamma):
            return False
        return device_model(smc.fk) is not None and getattr(other, "_d", 1) == 1

    def two_filter_smoothing(self, t, info, phi, loggamma, linear_cost=False, return_ess=False, modif_forward=None,
                             modif_info=None, npairs=None, seed=None, replay=None, return_idx=False, island=0,
                             island_info=0):
        smc = self._smc
        if t < 0 or t >= smc._n - 1:
            raise ValueError(_TWO_FILTER_T_ERR)
        if not self._two_filter_on_device(info, phi, loggamma):
            self._two_filter_route = "host"
            return _two_filter_numpy(self, t, info, phi, loggamma, linear_cost, return_ess, modif_forward, modif_info,
                                     npairs, seed, replay, return_idx)
        self._two_filter_route = "device"
        ptr = _lib.hptr
        K = phi.K
        est, ess = np.empty(K), _lib.c_dbl(0.0)
        f, g3 = phi._struct(), loggamma._coef()
        P, J, I = 0, None, None
        modif = {"modif_forward": None, "modif_info": None}
        tapes = dict.fromkeys(_TWO_FILTER_TAPES)
        draws = False                                      # does the launch draw from the key?
        if linear_cost:
            P = int(smc.N if npairs is None else npairs)
            if P >= 1:
                tapes = _two_filter_replay(replay, P)
                if return_idx:
                    J, I = np.empty(P, dtype=np.int64), np.empty(P, dtype=np.int64)
            for name, a, n in (("modif_forward", modif_forward, smc.N), ("modif_info", modif_info, info.N)):
                if a is not None:
                    a = np.ascontiguousarray(a, dtype=np.float64)
                    if a.shape != (n,):
                        raise ValueError("two-filter smoothing: %s has shape %s, expected %s" % (name, a.shape, (n,)))
                    modif[name] = a
            draws = tapes["idx_fwd"] is None and (tapes["u_fwd"] is None or tapes["u_info"] is None)
        _lib.check(_lib.lib().smc_filter_two_filter(
            smc._f, int(island), info._f, int(island_info), int(t), _lib.TWOFILTER_ON if linear_cost else _lib.TWOFILTER_ON2,
            ctypes.byref(f), ptr(g3, _lib.c_dbl), ptr(modif["modif_forward"], _lib.c_dbl), ptr(modif["modif_info"], _lib.c_dbl),
            P, _lib.u64_seed(seed if draws else seed or 0),
            ptr(tapes["u_fwd"], _lib.c_dbl), ptr(tapes["u_info"], _lib.c_dbl), ptr(tapes["idx_fwd"], _lib.c_i64),
            ptr(tapes["idx_info"], _lib.c_i64), ptr(J, _lib.c_i64), ptr(I, _lib.c_i64), ptr(est, _lib.c_dbl),
            ctypes.byref(ess)))
        est = est[0] if phi.scalar else est
        if not linear_cost:
            return est
        return _two_filter_result(est, float(ess.value), J, I, return_ess, return_idx)

    two_filter_smoothing.__doc__ = _TWO_FILTER_DOC + """
        On the device (smc_filter_two_filter) when ``info`` keeps a device-resident history too, neither filter is SQMC,
        the forward model is one backward sampling takes, ``phi`` is a ``QuadAddFunc`` and ``loggamma`` a
        ``QuadLogGamma``: the O(N^2) form is one all-pairs launch over the two resident histories, the O(N) form two
        inverse-CDF draws per pair in integer CDFs.  Everything else takes the NumPy route.  ``island`` /
        ``island_info`` pick the island of each filter (device route)."""

    def _backward(self, method, M, nsteps, seed, island, replay, return_idx):
        """``nsteps``: Metropolis steps (MCMC) or max_trials (rejection)."""
        smc = self._smc
        M, nsteps, T = int(M), int(nsteps), smc._n
        seed = _lib.u64_seed(seed)
        on2, reject = method == _lib.BACKWARD_ON2, method == _lib.BACKWARD_REJECT
        steps = (max(T - 1, 0), M) if on2 else (max(T - 1, 0), nsteps, M)
        spec = {"idx_last": ((M,), np.int64), "u_last": ((M,), np.float64),
                ("u" if on2 else "u_prop"): (steps, np.float64)}
        if not on2:
            spec["u_acc"] = (steps, np.float64)
        if reject:
            spec["u"] = ((max(T - 1, 0), M), np.float64)
        if M < 1 or nsteps < 1:           # the library refuses these in its own words: no shape is checked
            spec = {k: (None, dt) for k, (_, dt) in spec.items()}
        tapes = read_tapes("backward sampling", replay, spec)
        ptr = _lib.hptr
        idx = np.empty((T, max(M, 0)), dtype=np.int64)
        paths = np.empty((T, max(M, 0)))
        last = (ptr(tapes["idx_last"], _lib.c_i64), ptr(tapes["u_last"], _lib.c_dbl))
        out = (ptr(idx, _lib.c_i64), ptr(paths, _lib.c_dbl))
        if reject:
            log_bound = np.array([self.fk.upper_bound_trans(s) for s in range(1, T)], dtype=np.float64).reshape(-1)
            nprops, nexact = np.zeros(max(T - 1, 0), dtype=np.int64), np.zeros(max(T - 1, 0), dtype=np.int64)
            _check_kind(_lib.lib().smc_filter_backward_reject(
                smc._f, int(island), M, nsteps, seed, ptr(log_bound, _lib.c_dbl), *last,
                ptr(tapes["u_prop"], _lib.c_dbl), ptr(tapes["u_acc"], _lib.c_dbl), ptr(tapes["u"], _lib.c_dbl),
                *out, ptr(nprops, _lib.c_i64), ptr(nexact, _lib.c_i64)))
            self.nprops, self.nexact = nprops, nexact
            self.acc_rate = (M - nexact) / nprops
        else:
            _check_kind(_lib.lib().smc_filter_backward_sample(
                smc._f, int(island), method, M, nsteps, seed, *last,
                ptr(tapes.get("u", tapes.get("u_prop")), _lib.c_dbl), ptr(tapes.get("u_acc"), _lib.c_dbl), *out))
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
        return _wgts_at(self._smc, t)

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
        _lib.check(_lib.lib().smc_filter_trajectories(self._smc._f, 0, _lib.hptr(out, _lib.c_i64)))
        return out
