"""Counterpart of ``particles.mcmc.CSMC`` (mcmc.py:453-475): the conditional particle filter that updates the states
in Particle Gibbs (mcmc.py:533-619; Andrieu, Doucet & Holenstein 2010), for many chains at once.

``CSMC`` is ``SMC`` with multinomial resampling and a whole history, whose particle 0 follows the retained trajectory
``xstar``.  Bootstrap filters of LinearGauss, StochVol, Gordon_etal, ThetaLogistic and DiscreteCox with N <= 1024 run
conditional ON THE DEVICE: one persistent workgroup per chain, the whole time loop in one launch (``k_csmc_small``,
DESIGN section 6), chains as islands (``n_islands``, or one model per chain through ``fk=[...]``).  ``new_paths`` then
draws the next trajectory of every chain in one more launch (``k_csmc_path``), so a Particle Gibbs state update for C
chains is two launches.  Every other model runs the reference's two overrides on the template-method step.
"""
import numpy as np

from . import _lib
from . import smoothing
from .core import SMC
from ._lib import DeviceArray, check, lib

_MAX_N = 1024


def device_conditional(fk, N):
    """Does ``CSMC(fk, N)`` run conditional on the device (what ``smc_filter_set_conditional`` accepts)?"""
    fks = list(fk) if isinstance(fk, (list, tuple)) else [fk]
    for g in fks:
        if g is None or getattr(g, "_fk_kind", None) != _lib.FK_BOOTSTRAP:
            return False
        model = smoothing.device_model(g)
        if model is None or model.get("params") is None:
            return False
    return (1 <= N <= _MAX_N and not (_lib.path_flags() & _lib.PATH_FLAGS["SMC_NO_SMALL"])
            and SMC._will_fuse(fks[0], False, "multinomial", N=N))


class CSMC(SMC):
    """Conditional SMC (mcmc.py:453-475).

    fk, N, ESSrmin, xstar : as ``particles.mcmc.CSMC``.  ``xstar`` is a length-T sequence, or -- ``n_islands`` chains --
        (n_islands, T), one retained trajectory per chain (a ``DeviceArray`` of that shape is used where it is: what
        ``new_paths`` leaves in ``paths_device``).  ``fk=[...]`` gives every chain its own parameters.
    seed, n_islands, replay : as ``SMC``.  The free ancestors of a resampling step are N - 1 iid draws from the
        weights (Philox stream 6, or slots 1 .. N-1 of the multinomial replay tape); the reference draws N sorted
        indices and overwrites the first -- the same conditional SMC kernel, another coupling of the particles.
    """

    def __init__(self, fk=None, N=100, ESSrmin=0.5, xstar=None, seed=None, n_islands=1, replay=None):
        fks = list(fk) if isinstance(fk, (list, tuple)) else None
        C = len(fks) if fks is not None else int(n_islands)
        fk0 = fks[0] if fks is not None else fk
        self._cond_device = device_conditional(fk, N)
        self._xstar_dev = None
        if self._cond_device:
            if isinstance(xstar, DeviceArray):
                if tuple(xstar.shape) != (C, fk0.T) or xstar.dtype != np.float64:
                    raise ValueError("CSMC: xstar on the device must be float64 of shape (n_islands, T) = %s, got %s"
                                     % ((C, fk0.T), tuple(xstar.shape)))
                self._xstar_dev = xstar
            else:
                xs = np.asarray(xstar, dtype=np.float64)
                if xs.shape == (fk0.T, 1):
                    xs = xs[:, 0]
                if xs.shape not in ((C, fk0.T),) + (((fk0.T,),) if C == 1 else ()):
                    raise ValueError("CSMC: xstar must have shape (T,) or (n_islands, T) = %s, got %s"
                                     % ((C, fk0.T), xs.shape))
                self._xstar_dev = DeviceArray.from_numpy(np.ascontiguousarray(xs.reshape(C, fk0.T)))
        else:
            if C != 1:
                raise ValueError("CSMC: n_islands > 1 needs a conditional filter the device runs (Bootstrap of LinearGauss, "
                                 "StochVol, Gordon_etal, ThetaLogistic or DiscreteCox, N <= %d)" % _MAX_N)
            if xstar is None or len(xstar) != fk0.T:
                raise ValueError("CSMC: xstar must hold one state per time step (T = %d)" % fk0.T)
        self.xstar = xstar
        SMC.__init__(self, fk=fk, N=N, resampling="multinomial", ESSrmin=ESSrmin, store_history=True, collect="off",
                     seed=seed, n_islands=n_islands, replay=replay)
        self.paths_device = None

    # (SMC.__init__ asks through self: a conditional filter the device cannot pin runs the template-method step)
    def _will_fuse(self, fk, qmc=False, resampling="systematic", model=False, N=None):
        return self._cond_device and SMC._will_fuse(fk, qmc, resampling, model, N=N)

    def _create_filter(self, model, replay, use_graph, island_offset, restore=None):
        SMC._create_filter(self, model, replay, use_graph, island_offset, restore)
        check(lib().smc_filter_set_conditional(self._f, self._xstar_dev.ptr))      # (also behind unpickling)

    def __deepcopy__(self, memo):
        if self._xstar_dev is not None:
            memo[id(self._xstar_dev)] = self._xstar_dev         # smc_filter_clone shares the buffer: so do the objects
        return SMC.__deepcopy__(self, memo)

    # ---- the reference's overrides: the template-method step (mcmc.py:468-475)
    def generate_particles(self):
        SMC.generate_particles(self)
        self.X[0] = self.xstar[0]

    def resample_move(self):
        SMC.resample_move(self)
        self.X[0] = self.xstar[self.t]
        self.A[0] = 0

    def new_paths(self, backward_step=False, seed=None, replay=None, return_idx=False):
        """One new trajectory per chain, (n_islands, T): the line of ancestors of a particle drawn from the final
        weights (``extract_one_trajectory``), or -- ``backward_step`` -- exact backward sampling
        (``backward_sampling_ON2(1)``).  On the device all chains in one launch; the paths also stay there, in
        ``paths_device``, ready to be the next ``CSMC``'s ``xstar``.

        seed : Philox key (stream 3, counter (0, t, island, 3), as backward sampling at M = 1); None: a fresh one.
        replay : dict of uniforms instead: ``u_last`` (n_islands,), ``u`` (T-1, n_islands) for the backward steps.
        """
        return new_paths(self, backward_step, seed, replay, return_idx)


def new_paths(pf, backward_step=False, seed=None, replay=None, return_idx=False):
    """``CSMC.new_paths`` for any filter with a whole history (the first update of a Particle Gibbs chain runs an
    unconditional ``SMC(store_history=True)``)."""
    if not getattr(pf, "_fused", False) or getattr(pf, "_keep_history", 0) != 1:
        return _new_paths_host(pf, backward_step, return_idx)
    C, T = pf.n_islands, pf._n
    tapes = smoothing.read_tapes("new_paths", replay, {"u_last": ((C,), np.float64),
                                                       "u": ((max(T - 1, 0), C), np.float64)})
    seed = _lib.u64_seed(seed)
    ptr = _lib.hptr
    idx = np.empty((C, T), dtype=np.int64) if return_idx else None
    paths = np.empty((C, T))
    if T < 1:
        raise ValueError("new_paths: no step has run yet")
    dev = DeviceArray((C, T))
    check(lib().smc_filter_csmc_paths(pf._f, 1 if backward_step else 0, seed,
                                      ptr(tapes["u_last"], _lib.c_dbl), ptr(tapes["u"], _lib.c_dbl),
                                      ptr(idx, _lib.c_i64), ptr(paths, _lib.c_dbl), dev.ptr))
    pf.paths_device = dev
    return (paths, idx) if return_idx else paths


def _new_paths_host(pf, backward_step, return_idx):
    """The template-method route: the history is on the host, one chain."""
    if return_idx:
        raise ValueError("new_paths: return_idx needs the device-resident history")
    if backward_step:
        out = pf.hist.backward_sampling_ON2(1)
    else:
        from . import resampling as rs
        n = rs.multinomial_once(pf.hist.wgts[-1].W)
        out = [pf.hist.X[-1][n]]
        for t in reversed(range(len(pf.hist.X) - 1)):
            n = pf.hist.A[t + 1][n]
            out.append(pf.hist.X[t][n])
        out.reverse()
    return np.asarray(out)[None]
