"""Log-weight stores a resampling step leaves out (StepPlan::lazy_lw of smc_filter.hip): the checks behind
tests/test_lazy_lw_emu.py (emulator build) and tests/test_lazy_lw_gpu.py (MI355X), in the manner of parity_cases.py.

What is promised: whenever a smc_filter_step call has returned, lw of the current step is in memory as ever; only the
steps in the INTERIOR of one call may leave their slot unwritten when they resample, and a later step of the same call
that does not resample forms those values again from X, bit for bit.  So a run in one call, the same run under
SMC_EAGER_LW=1 (every step stores) and the same run one step per call are the same run -- wherever the calls end."""
import copy
import ctypes
import os
import pickle

import numpy as np

import particles_amd as pa
from particles_amd import _lib
from particles_amd import kalman
from particles_amd import resampling as rs_mod
from particles_amd import state_space_models as ssm

T = 40

MODELS = {
    "toy": (lambda: kalman.LinearGauss(rho=0.9, sigmaX=1.0, sigmaY=1.5), "lg_adaptive"),
    "sv": (lambda: ssm.StochVol(), "sv_systematic"),
    "gordon": (lambda: ssm.Gordon_etal(), "gordon_boot"),
    "theta": (lambda: ssm.ThetaLogistic(), "theta_boot"),
    "cox": (lambda: ssm.DiscreteCox(mu=0.5, sigma=0.4, phi=0.9), "cox_boot"),        # (aux_t = gammaln(y_t + 1))
    "svlev": (lambda: ssm.StochVolLeverage(phi=-0.5), "svlev_boot"),
}

# name -> model, N, islands, scheme, ESSrmin, environment.  Sizes: one wide workgroup (2048), two (4096), a ragged
# even and a ragged odd N (k_propagate<.., RAGGED = 1 / 2>), three islands, k_reduce2 + k_ancestors2 in front
# (SMC_TWO_LEVEL_MID), the multinomial scheme (spacings + k_ancestors2).  ESSrmin: where the eager run of the case
# mixes resampling and non-resampling steps (check_coverage holds every case to it).
CASES = {
    "toy_2048": ("toy", 2048, 1, "systematic", 0.5, {}),
    "sv_4096": ("sv", 4096, 1, "systematic", 0.95, {}),
    "gordon_3000": ("gordon", 3000, 1, "systematic", 0.3, {}),
    "theta_1501": ("theta", 1501, 1, "systematic", 0.7, {}),
    "cox_3x2048": ("cox", 2048, 3, "stratified", 0.8, {}),
    "toy_4096_mid": ("toy", 4096, 1, "systematic", 0.5, {"SMC_TWO_LEVEL_MID": "1"}),
    "toy_3000_multinomial": ("toy", 3000, 1, "multinomial", 0.5, {}),
    "sv_1501_stratified": ("sv", 1501, 1, "stratified", 0.95, {}),
}


def data(golden, model, T=T):
    y = np.squeeze(golden(MODELS[model][1])["y"])[:T]
    assert len(y) == T
    return [np.atleast_1d(v) for v in y]


class _Env:
    """Verification switches are read when a filter is created (particles_amd._lib.path_flags)."""

    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def make(golden, case, eager=False, T=T, **kw):
    model, N, islands, scheme, ess, env = CASES[case]
    env = dict(env, **({"SMC_EAGER_LW": "1"} if eager else {}))
    with _Env(env):
        return pa.SMC(fk=ssm.Bootstrap(ssm=MODELS[model][0](), data=data(golden, model, T)), N=N, seed=17, ESSrmin=ess,
                      resampling=scheme, n_islands=islands, collect="off", **kw)


def lazy_steps(pf):
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().smc_filter_lazy_lw_steps(pf._f, ctypes.byref(n)))
    return n.value


def snapshot(pf):
    """X, lw, W, A of every island, the islands' logLt, and the summary rows (ESS, log mean, loglt, logLt, rs_flag)."""
    out = [pf.logLts_islands.copy(), pf._summ().copy()]
    for i in range(pf.n_islands):
        out += [pf._get(f, i).copy() for f in (_lib.FIELD_X, _lib.FIELD_LW, _lib.FIELD_W, _lib.FIELD_A)]
    return out


def same(u, v):
    return len(u) == len(v) and all(np.array_equal(a, b) for a, b in zip(u, v))


_ONE_CALL = {}


def one_call(golden, case, T=T):
    """(snapshot, rs flags (islands, T), lazy-step count) of the case run by ONE step_async(T): computed once."""
    if (case, T) not in _ONE_CALL:
        pf = make(golden, case, T=T)
        assert pf.step_async(T) == T
        snap = snapshot(pf)
        _ONE_CALL[case, T] = (snap, snap[1][:, :, 4] != 0, lazy_steps(pf))
    return _ONE_CALL[case, T]


def expected_lazy(rs, first, last):
    """Steps first .. last run by one call: all but the last are launched lazy, those in which some island resamples
    leave the store out (step 0 never resamples)."""
    return int(np.sum(np.any(rs[:, first:last], axis=0)))


def check_three_runs(golden, case):
    """One call, the same under SMC_EAGER_LW=1, and one step per call: the same run, and the counter says which path ran."""
    a, rs, n_a = one_call(golden, case)
    assert n_a == expected_lazy(rs, 0, T - 1) and n_a > 0, (case, n_a)
    b = make(golden, case, eager=True)
    b.step_async(T)
    assert same(a, snapshot(b)), case
    assert lazy_steps(b) == 0
    c = make(golden, case)
    for _ in range(T):
        next(c)
    assert same(a, snapshot(c)), case
    assert lazy_steps(c) == 0


def check_boundaries(golden, case, T=T):
    """The call boundary moved across every transition: step_async(k), lw and W read, step_async(T - k), every k.
    (A shorter T -- the emulator's -- must still hold the three transitions: check_coverage with the same T.)"""
    a, rs, _ = one_call(golden, case, T)
    for k in range(1, T):
        pf = make(golden, case, T=T)
        pf.step_async(k)
        lw, W = pf.wgts.lw.copy(), pf.W.copy()
        assert np.all(np.isfinite(W)) and abs(W.sum() - 1.0) < 1e-12 and not np.any(np.isnan(lw)), (case, k)
        pf.step_async(T - k)
        assert same(a, snapshot(pf)), (case, k)
        assert lazy_steps(pf) == expected_lazy(rs, 0, k - 1) + expected_lazy(rs, k, T - 1), (case, k)


def check_coverage(golden, case, T=T):
    """The interior steps of the case (1 .. T-2: every one of them launched lazy by the one-call run, step 0 never
    resamples) hold all three transitions; islands do not all decide alike."""
    _, rs, _ = one_call(golden, case, T)
    for isl in range(rs.shape[0]):
        r = rs[isl, 1:T - 1]
        pairs = set(zip(r[:-1].tolist(), r[1:].tolist()))
        assert {(True, False), (False, True), (True, True)} <= pairs, (case, isl, r.astype(int))
    if rs.shape[0] > 1:
        assert np.any(np.any(rs[:, 1:T - 1], axis=0) & ~np.all(rs[:, 1:T - 1], axis=0)), (case, rs.astype(int))


def check_ineligible(golden, T=T):
    """Filters whose steps read lw, or whose weights cannot be formed again from the new particle alone: no step
    ever leaves the store out."""
    y = data(golden, "toy", T)
    lg = lambda: kalman.LinearGauss(rho=0.9, sigmaX=1.0, sigmaY=1.5)
    boot = lambda: ssm.Bootstrap(ssm=lg(), data=y)
    sv_y = data(golden, "sv", T)
    filters = {
        "svlev": dict(fk=ssm.Bootstrap(ssm=MODELS["svlev"][0](), data=data(golden, "svlev", T)), N=2048),
        "guided": dict(fk=ssm.GuidedPF(ssm=lg(), data=y), N=2048),
        "apf": dict(fk=ssm.AuxiliaryPF(ssm=ssm.StochVol(), data=sv_y), N=2048),
        "apf_boot": dict(fk=ssm.AuxiliaryBootstrap(ssm=ssm.StochVol(), data=sv_y), N=2048),
        "strict": dict(fk=boot(), N=2048, strict_ancestors=True),
        "qmc": dict(fk=boot(), N=2048, qmc=True),
        "history": dict(fk=boot(), N=2048, store_history=True),
        "moments": dict(fk=boot(), N=2048, collect=[pa.collectors.Moments()]),
        "graph": dict(fk=boot(), N=2048, use_graph=True),
        "small": dict(fk=boot(), N=1024),
        "one_tile_philox_multinomial": dict(fk=boot(), N=1000, resampling="multinomial"),
    }
    for name, kw in filters.items():
        kw.setdefault("collect", "off")
        mode = _lib.RNG_MODE[0]
        if kw.get("qmc"):
            rs_mod.set_rng("philox")                   # (device-generated points: the fused SQMC step)
        try:
            pf = pa.SMC(seed=17, ESSrmin=0.9, **kw)
        finally:
            rs_mod.set_rng(mode)
        assert pf._fused, name
        pf.step_async(T - 3)
        pf.step_async(3)
        rs = pf._summ()[0][:, 4]
        assert rs.sum() > 0 and lazy_steps(pf) == 0, (name, rs.sum())


def check_state_transport(golden, case, ks=(7, 22)):
    """A filter pickled (smc_filter_save_state / load_state) or deep-copied (smc_filter_clone) between two calls
    continues as the uninterrupted run does."""
    a, rs, _ = one_call(golden, case)
    for k in ks:
        pf = make(golden, case)
        pf.step_async(k)
        with _Env(CASES[case][5]):
            q = pickle.loads(pickle.dumps(pf))
        c = copy.deepcopy(pf)               # (a clone under a key of its own: back to the source's, to compare)
        _lib.check(_lib.lib().smc_filter_reseed(c._f, pf.seed))
        for r in (pf, q, c):
            r.step_async(T - k)
            assert same(a, snapshot(r)), (case, k)
        assert lazy_steps(c) == expected_lazy(rs, k, T - 1)       # (a clone counts what IT enqueues)
