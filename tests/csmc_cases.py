"""Conditional SMC on the device (particles_amd.mcmc.CSMC, smc_filter_set_conditional / smc_filter_csmc_paths,
particles_amd/csrc/smc_csmc.h): the checks behind tests/test_csmc_gpu.py (MI355X) and tests/test_csmc_emu.py (emulator
build), in the manner of smoothing_cases.py.

  pinned      the reference's own mcmc.CSMC run (tests/golden/csmc_lg.npz, written by tests/golden/make_golden_csmc.py)
              replayed through (z, u): X, lw and A[1:] array_equal, A[0] == 0.  No exception: the generator chose a run
              with no uniform within 1e-11 of a step of a CDF.
  restated    every step teacher-forced in NumPy on the device's own previous step: ancestors array_equal to the integer
              CDF contract of smc_smooth.h restated with Python integers, X_t[0] == xstar[t] exactly, A_t[0] == 0,
              X_t[1:] = loc(xp) + scale z and lw_t = scipy's logpdf within 1e-12 (np.allclose, rtol = atol = 1e-12: the
              project's tolerance, parity_cases.RTOL), lw_t[0] the weight of xstar[t], summary rows within 1e-12; at
              t = 0 particles 1 .. N-1 bit-equal to the unconditional filter of the same seed.  Then the paths: the
              genealogy against NumPy tracing of hist.A, the backward mode array_equal to the existing sampler
              (DeviceParticleHistory._backward at M = 1) for every island, with tapes and with a Philox seed.
  philox      Philox mode is replay mode fed with stream 6 (ancestors) and stream 3 (paths).
  invariance  C independent chains started from the exact smoothing law stay there under 20 conditional updates.
  lifecycle   determinism, stepping in several calls, pickling mid-run, cloning, an unconditional filter left alone.
  refusals    what the C entries refuse, and which configurations run the template-method step instead.
"""
import bisect
import copy
import itertools
import math
import pickle

import numpy as np
import pytest
import scipy.stats

import particles_amd as pa
import parity_cases as pc
from oracle import smc_oracle as orc
from particles_amd import _lib
from particles_amd import collectors
from particles_amd import kalman
from particles_amd import mcmc
from particles_amd import resampling as rs_mod
from particles_amd import state_space_models as ssm

T6 = 6
TOL = 1e-12


def _close(a, b):
    return np.allclose(a, b, rtol=TOL, atol=TOL, equal_nan=True)


def _y(golden, name, T):
    y = np.squeeze(golden(name)["y"])[:T]
    assert len(y) == T
    return [np.atleast_1d(v) for v in y]


# kind -> model class, golden with the data, three parameter rows (islands), and the model's three laws in NumPy / scipy:
# x0(th) -> (loc, scale); px(th, t, xp) -> (loc, scale); py(th, y, x) -> log p(y | x)
def _ar1_sd(sigma, rho):
    return sigma / np.sqrt(1.0 - rho ** 2)


KINDS = {
    "lg": dict(cls=kalman.LinearGauss, data="lg_adaptive",
               thetas=[dict(rho=0.9, sigmaX=1.0, sigmaY=1.5), dict(rho=0.5, sigmaX=0.7, sigmaY=0.4),
                       dict(rho=0.95, sigmaX=0.3, sigmaY=2.0)],
               x0=lambda th: (0.0, _ar1_sd(th["sigmaX"], th["rho"])),
               px=lambda th, t, xp: (th["rho"] * xp, th["sigmaX"]),
               py=lambda th, y, x: scipy.stats.norm.logpdf(y, loc=x, scale=th["sigmaY"])),
    "sv": dict(cls=ssm.StochVol, data="sv_systematic",
               thetas=[dict(mu=-1.02, rho=0.9702, sigma=0.178), dict(mu=-0.5, rho=0.9, sigma=0.3),
                       dict(mu=-1.5, rho=0.8, sigma=0.5)],
               x0=lambda th: (th["mu"], _ar1_sd(th["sigma"], th["rho"])),
               px=lambda th, t, xp: (th["mu"] + th["rho"] * (xp - th["mu"]), th["sigma"]),
               py=lambda th, y, x: scipy.stats.norm.logpdf(y, loc=0.0, scale=np.exp(0.5 * x))),
    # (d and e feed the per-step term all islands share: they do not vary)
    "gordon": dict(cls=ssm.Gordon_etal, data="gordon_boot",
                   thetas=[dict(a=0.05, b=0.5, c=25.0, sigmaX=3.162278), dict(a=0.04, b=0.4, c=20.0, sigmaX=2.0),
                           dict(a=0.06, b=0.6, c=25.0, sigmaX=1.0)],
                   x0=lambda th: (0.0, 2.0),
                   px=lambda th, t, xp: (th["b"] * xp + th["c"] * xp / (1.0 + xp ** 2) + 8.0 * np.cos(1.2 * (t - 1)),
                                         th["sigmaX"]),
                   py=lambda th, y, x: scipy.stats.norm.logpdf(y, loc=th["a"] * x ** 2, scale=1.0)),
    "theta": dict(cls=ssm.ThetaLogistic, data="theta_boot",
                  thetas=[dict(tau0=0.15, tau1=0.12, tau2=0.1, sigmaX=0.47, sigmaY=0.39),
                          dict(tau0=0.1, tau1=0.1, tau2=0.2, sigmaX=0.3, sigmaY=0.5),
                          dict(tau0=0.2, tau1=0.15, tau2=0.1, sigmaX=0.6, sigmaY=0.3)],
                  x0=lambda th: (0.0, 1.0),
                  px=lambda th, t, xp: (xp + th["tau0"] - th["tau1"] * np.exp(th["tau2"] * xp), th["sigmaX"]),
                  py=lambda th, y, x: scipy.stats.norm.logpdf(y, loc=x, scale=th["sigmaY"])),
    "cox": dict(cls=ssm.DiscreteCox, data="cox_boot",
                thetas=[dict(mu=0.5, sigma=0.4, phi=0.9), dict(mu=0.3, sigma=0.6, phi=0.8), dict(mu=0.7, sigma=0.2, phi=0.95)],
                x0=lambda th: (th["mu"], _ar1_sd(th["sigma"], th["phi"])),
                px=lambda th, t, xp: (th["mu"] + th["phi"] * (xp - th["mu"]), th["sigma"]),
                py=lambda th, y, x: scipy.stats.poisson.logpmf(y, np.exp(x))),
}

# name -> (kind, N, islands, ESSrmin, what the run must do).  Between them: every N of {2, 5, 64, 255, 256, 257, 1021, 1024}
# (one wave / four waves at 256 | 257, vector / ragged stores at N mod 4), 1 and 3 islands, runs that never resample
# (ESSrmin 0), always (ESS < 1.1 N) and both, all five kinds.
CASES = {
    "lg_2": ("lg", 2, 1, 0.7, None),
    "lg_5x3_always": ("lg", 5, 3, 1.1, "always"),
    "lg_64_never": ("lg", 64, 1, 0.0, "never"),
    "lg_255x3": ("lg", 255, 3, 0.6, "mixed"),
    "lg_256_always": ("lg", 256, 1, 1.1, "always"),
    "lg_257x3": ("lg", 257, 3, 0.6, "mixed"),
    "lg_1021": ("lg", 1021, 1, 0.6, "mixed"),
    "lg_1024x3": ("lg", 1024, 3, 0.6, "mixed"),
    "sv_257x3": ("sv", 257, 3, 0.95, None),
    "sv_1024_always": ("sv", 1024, 1, 1.1, "always"),
    "gordon_255x3": ("gordon", 255, 3, 0.5, None),
    "gordon_5": ("gordon", 5, 1, 0.5, None),
    "theta_1021x3": ("theta", 1021, 3, 0.7, None),
    "theta_64_never": ("theta", 64, 1, 0.0, "never"),
    "cox_64x3": ("cox", 64, 3, 0.8, None),
    "cox_256": ("cox", 256, 1, 0.8, None),
}


def models_of(kind, C):
    k = KINDS[kind]
    return [k["cls"](**th) for th in k["thetas"][:C]], k["thetas"][:C]


def make_fk(golden, kind, C, T=T6):
    models, thetas = models_of(kind, C)
    y = _y(golden, KINDS[kind]["data"], T)
    fks = [ssm.Bootstrap(ssm=m, data=y) for m in models]
    return (fks if C > 1 else fks[0]), thetas, np.array([v[0] for v in y])


def host_history(pf, i):
    T = pf._n
    X = np.array([pf._history(_lib.FIELD_X, t, i) for t in range(T)])
    lw = np.array([pf._history(_lib.FIELD_LW, t, i) for t in range(T)])
    W = np.array([pf._history(_lib.FIELD_W, t, i) for t in range(T)])
    flags = pf._summ()[i, :, 4] != 0
    A = np.array([pf._history(_lib.FIELD_A, t, i) if t and flags[t] else np.arange(pf.N) for t in range(T)])
    return X, lw, W, A, flags


# ---- the integer CDF contract of smc_smooth.h in Python integers
def sm_shift(N):
    c = 0
    while (1 << c) < N:
        c += 1
    return 61 - c


def int_terms(e, N):
    s = sm_shift(N)
    return [int(round(math.ldexp(float(v), s))) if v > 0.0 else 0 for v in e]        # rint: half to even


def int_draw(prefix, u):
    """The first n whose inclusive prefix exceeds floor(u Q), u held to [0, Q - 1]; Q = 0: N - 1."""
    Q = prefix[-1]
    if Q == 0:
        return len(prefix) - 1
    if not u > 0.0:
        thr = 0
    elif u >= 1.0:
        thr = Q - 1
    else:
        num, den = float(u).as_integer_ratio()
        thr = min(num * Q // den, Q - 1)
    return bisect.bisect_right(prefix, thr)                 # (prefix[n - 1] <= thr < prefix[n])


def int_draws(e, us):
    prefix = list(itertools.accumulate(int_terms(e, len(e))))
    return np.array([int_draw(prefix, u) for u in us], dtype=np.int64)


def describe(pf):
    return pc.describe(pf)


def old_backward(pf, island, seed=None, replay=None):
    """backward_sampling_ON2(1) by the sampler that was there before the one-launch route: (T,) indices."""
    return pf.hist._backward(_lib.BACKWARD_ON2, 1, 1, seed, island, replay, True)[1][:, 0]


def stream3_tapes(seed, T, C):
    """The uniforms of the paths launch in Philox mode: counter (0, s, island, 3), word x01 -> [0, 1)."""
    u = np.empty((T, C))
    for s in range(T):
        for i in range(C):
            u[s, i] = orc.u01_halfopen(orc.philox_u64_pair(seed, np.zeros(1, dtype=np.uint32), s, i, 3)[0])[0]
    return u[T - 1].copy(), u[:T - 1].copy()


def stream6_uniforms(seed, N, t, island):
    return orc.u01_halfopen(orc.philox_u64_pair(seed, np.arange(N, dtype=np.uint32), t, island, 6)[0])


# ---------------------------------------------------------------------------------------------------------------- 1
def check_pinned(golden):
    g = golden("csmc_lg")
    N, T = int(g["N"]), int(g["T"])
    model = kalman.LinearGauss(rho=float(g["lg_rho"]), sigmaX=float(g["lg_sigmaX"]), sigmaY=float(g["lg_sigmaY"]))
    y = [np.atleast_1d(v) for v in g["y"]]
    pf = mcmc.CSMC(fk=ssm.Bootstrap(ssm=model, data=y), N=N, ESSrmin=float(g["ESSrmin"]), xstar=g["xstar"],
                   replay=(g["z"].reshape(T, 1, N), g["u"].reshape(T, 1, N)))
    assert pf._fused and describe(pf) == "k_csmc_small"
    pf.run()
    X, lw, W, A, flags = host_history(pf, 0)
    assert np.array_equal(flags, g["rs_flags"])
    assert 0 < flags.sum() < T - 1
    print("pinned: X %d, lw %d, A %d entries differ" % (np.sum(X != g["X"]), np.sum(lw != g["lw"]),
                                                         np.sum(A[:, 1:] != g["A"][:, 1:])))
    assert np.array_equal(X, g["X"])
    assert np.array_equal(lw, g["lw"])
    assert np.array_equal(A[:, 1:], g["A"][:, 1:]) and np.all(A[:, 0] == 0)
    assert abs(pf.logLt - float(g["logLt"])) < 1e-9 * abs(float(g["logLt"]))


# ---------------------------------------------------------------------------------------------------------------- 2, 4, 5
_RUNS = {}


def run_of(golden, case):
    """The case's conditional filter in replay mode, run once: (pf, thetas, y, xstar, z, u)."""
    if case not in _RUNS:
        kind, N, C, ess, _ = CASES[case]
        fk, thetas, y = make_fk(golden, kind, C)
        rng = np.random.default_rng(sum(map(ord, case)))
        xstar = np.array([KINDS[kind]["x0"](th)[0] for th in thetas])[:, None] + 0.5 * rng.standard_normal((C, T6))
        z = rng.standard_normal((T6, C, N))
        u = np.sort(rng.random((T6, C, N)), axis=2)
        pf = mcmc.CSMC(fk=fk, N=N, ESSrmin=ess, xstar=xstar if C > 1 else xstar[0], seed=77, n_islands=C, replay=(z, u))
        assert pf._fused and describe(pf) == "k_csmc_small"
        pf.run()
        _RUNS[case] = (pf, thetas, y, xstar, z, u)
    return _RUNS[case]


def check_restated(golden, case):
    kind, N, C, ess, want = CASES[case]
    pf, thetas, y, xstar, z, u = run_of(golden, case)
    K = KINDS[kind]
    T = T6
    summ = pf._summ()
    unc = pa.SMC(fk=make_fk(golden, kind, C)[0], N=N, resampling="multinomial", ESSrmin=ess, store_history=True, collect="off",
                 seed=77, n_islands=C, replay=(z, u))
    unc.step_async(1)
    nres = 0
    for i in range(C):
        th = thetas[i]
        X, lw, W, A, flags = host_history(pf, i)
        nres += int(flags.sum())
        assert not flags[0]
        assert np.array_equal(X[:, 0], xstar[i]), (case, i, "particle 0 is not the retained trajectory")
        assert np.array_equal(X[0, 1:], unc._history(_lib.FIELD_X, 0, i)[1:]), (case, i, "t = 0 differs from the plain filter")
        logLt, prev_lm = 0.0, None
        for t in range(T):
            if t == 0:
                loc, sc = K["x0"](th)
                loc = np.full(N, loc)
                lw_prev = np.zeros(N)
            else:
                ess_prev = summ[i, t - 1, 0]
                assert bool(flags[t]) == bool(ess_prev < N * ess), (case, i, t, "the decision")
                if flags[t]:
                    want_A = int_draws(W[t - 1], u[t, i])
                    want_A[0] = 0
                    assert np.array_equal(A[t], want_A), (case, i, t, np.flatnonzero(A[t] != want_A)[:5])
                    lw_prev = np.zeros(N)
                else:
                    lw_prev = lw[t - 1]
                loc, sc = K["px"](th, t, X[t - 1][A[t]])
            xo = loc + sc * z[t, i]
            assert _close(X[t, 1:], xo[1:]), (case, i, t, "X", float(np.max(np.abs(X[t, 1:] - xo[1:]))))
            inc = K["py"](th, y[t], X[t])
            lwo = lw_prev + inc
            lwo = np.where(np.isnan(lwo), -np.inf, lwo)
            assert _close(lw[t], lwo), (case, i, t, "lw", float(np.max(np.abs(lw[t] - lwo))))
            # the pinned particle's weight is that of xstar[t], not of the particle the move made
            w0 = lw_prev[0] + K["py"](th, y[t], xstar[i, t])
            assert _close(lw[t, 0], w0), (case, i, t, "lw[0]", lw[t, 0], w0)
            # summary row from the device's own log-weights (resampling.py:217-226, core.py:351-359)
            w = orc.Weights(lw=lw[t].copy())
            lm = w.log_mean
            loglt = lm if (t == 0 or flags[t]) else lm - prev_lm
            logLt += loglt
            row = summ[i, t]
            assert _close(row[0], w.ESS) and _close(row[1], lm) and _close(row[2], loglt) and _close(row[3], logLt), \
                (case, i, t, row[:4], (w.ESS, lm, loglt, logLt))
            prev_lm = lm
    if want == "always":
        assert nres == C * (T - 1)
    elif want == "never":
        assert nres == 0
    elif want == "mixed":
        assert 0 < nres < C * (T - 1), (case, nres)
    check_paths(case, pf)


def check_paths(case, pf):
    """Tests 4 and 5 at the case's N, every island: genealogy against NumPy, backward mode against the old sampler."""
    C, T, N = pf.n_islands, pf._n, pf.N
    rng = np.random.default_rng(5)
    u_last, u = rng.random(C), rng.random((T - 1, C))
    hist = [host_history(pf, i) for i in range(C)]
    # genealogy
    paths, idx = pf.new_paths(replay={"u_last": u_last}, return_idx=True)
    assert paths.shape == (C, T) and idx.shape == (C, T) and idx.dtype == np.int64
    for i in range(C):
        X, lw, W, A, flags = hist[i]
        n = int(int_draws(W[T - 1], [u_last[i]])[0])
        for t in reversed(range(T)):
            assert idx[i, t] == n, (case, i, t, "genealogy")
            n = int(A[t][n])                                  # (A = arange where the step did not resample)
        assert np.array_equal(paths[i], X[np.arange(T), idx[i]])
    # backward, tapes
    paths, idx = pf.new_paths(backward_step=True, replay={"u_last": u_last, "u": u}, return_idx=True)
    assert np.array_equal(pf.paths_device.get(), paths)
    for i in range(C):
        tapes = {"u_last": u_last[i:i + 1], "u": u[:, i:i + 1]}
        assert np.array_equal(idx[i], old_backward(pf, i, replay=tapes)), (case, i, "backward, tapes")
        assert np.array_equal(paths[i], hist[i][0][np.arange(T), idx[i]])
        got = pf.hist.backward_sampling_ON2(1, island=i, replay=tapes, return_idx=True)
        assert np.array_equal(got[1][:, 0], idx[i]) and np.array_equal(np.array(got[0]), paths[i]) and np.ndim(got[0][0]) == 0
    # backward, Philox
    idx = pf.new_paths(backward_step=True, seed=4242, return_idx=True)[1]
    for i in range(C):
        assert np.array_equal(idx[i], old_backward(pf, i, seed=4242)), (case, i, "backward, Philox")


# ---------------------------------------------------------------------------------------------------------------- 3
def check_philox_streams(golden, N=257, C=3, seed=20240607):
    # (a) rho = 0, sigmaX = sigma0 = 1: X_t[n] = 0 + 1 z exactly, so the Philox run's own particles ARE its normals and
    #     the run can be replayed: with stream 6 on the u tape the history must come back bit for bit
    y = _y(golden, "lg_adaptive", T6)
    fk = ssm.Bootstrap(ssm=kalman.LinearGauss(rho=0.0, sigmaX=1.0, sigma0=1.0, sigmaY=0.8), data=y)
    xstar = np.random.default_rng(3).standard_normal((C, T6))
    a = mcmc.CSMC(fk=fk, N=N, ESSrmin=0.55, xstar=xstar, seed=seed, n_islands=C)
    a.run()
    z = np.array([[a._history(_lib.FIELD_X, t, i) for i in range(C)] for t in range(T6)])
    u = np.array([[stream6_uniforms(seed, N, t, i) for i in range(C)] for t in range(T6)])
    b = mcmc.CSMC(fk=fk, N=N, ESSrmin=0.55, xstar=xstar, n_islands=C, replay=(z, u))
    b.run()
    assert np.array_equal(a._summ(), b._summ()) and 0 < a._summ()[:, :, 4].sum() < C * (T6 - 1)
    for i in range(C):
        ha, hb = host_history(a, i), host_history(b, i)
        assert all(np.array_equal(p, q) for p, q in zip(ha, hb)), i
    # (b) any model, teacher-forced: the ancestors of the Philox run are the contract's draws from stream 6
    fk3, thetas, _ = make_fk(golden, "lg", C)
    c = mcmc.CSMC(fk=fk3, N=N, ESSrmin=0.7, xstar=xstar, seed=seed + 1, n_islands=C)
    c.run()
    plain = pa.SMC(fk=fk3, N=N, seed=seed + 1, n_islands=C, collect="off", store_history=True)
    plain.step_async(1)
    n = 0
    for i in range(C):
        X, lw, W, A, flags = host_history(c, i)
        assert np.array_equal(X[0, 1:], plain._history(_lib.FIELD_X, 0, i)[1:]) and X[0, 0] == xstar[i, 0]
        for t in range(1, T6):
            if flags[t]:
                want = int_draws(W[t - 1], stream6_uniforms(seed + 1, N, t, i))
                want[0] = 0
                assert np.array_equal(A[t], want), (i, t)
                n += 1
    assert n > 0
    # (c) the paths: stream 3, counter (0, s, island, 3)
    u_last, up = stream3_tapes(99, T6, C)
    for bw in (False, True):
        p1, i1 = c.new_paths(backward_step=bw, seed=99, return_idx=True)
        p2, i2 = c.new_paths(backward_step=bw, replay={"u_last": u_last, "u": up} if bw else {"u_last": u_last}, return_idx=True)
        assert np.array_equal(i1, i2) and np.array_equal(p1, p2)
        assert not np.array_equal(i1, c.new_paths(backward_step=bw, seed=100, return_idx=True)[1])


# ---------------------------------------------------------------------------------------------------------------- 6
def exact_smoothing(rho, sigmaX, sigmaY, y):
    """Mean and covariance of x_{0:T-1} | y_{0:T-1} for the stationary LinearGauss model, from the joint Gaussian."""
    T = len(y)
    s0 = sigmaX ** 2 / (1.0 - rho ** 2)
    S = s0 * rho ** np.abs(np.subtract.outer(np.arange(T), np.arange(T)))
    P = np.linalg.inv(np.linalg.inv(S) + np.eye(T) / sigmaY ** 2)
    return P @ (np.asarray(y) / sigmaY ** 2), P


def check_invariance(golden, C, backward, K=20, N=4, T=5):
    """Conditional SMC leaves the smoothing law invariant at ANY N >= 2.  C chains start from the exact law; after K
    updates (a fresh CSMC with a fresh seed, then new_paths) the chains are still C independent draws from it: at every
    t the mean of x_t and of x_t^2 over the chains lie within 4.5 standard errors of their exact values (2 modes x 5
    steps x 2 moments: 1.4e-4 that an invariant kernel fails; one mode per call).  N = 4 leaves a kernel that is not invariant far away."""
    th = KINDS["lg"]["thetas"][0]
    fk, _, y = make_fk(golden, "lg", 1, T=T)
    mean, P = exact_smoothing(th["rho"], th["sigmaX"], th["sigmaY"], y)
    var = np.diag(P)
    for bw in (bool(backward),):
        rng = np.random.default_rng(12 + bw)
        x = mean + rng.standard_normal((C, T)) @ np.linalg.cholesky(P).T
        for k in range(K):
            pf = mcmc.CSMC(fk=fk, N=N, xstar=x, seed=1000 * (1 + bw) + k, n_islands=C)
            pf.run()
            x = pf.new_paths(backward_step=bw, seed=5000 * (1 + bw) + k)
            assert x.shape == (C, T)
            if k % 2:                                       # the device buffer serves as the next xstar as well
                x = pf.paths_device
        x = np.asarray(x.get() if isinstance(x, pa.DeviceArray) else x)
        for t in range(T):
            e1, b1 = abs(x[:, t].mean() - mean[t]), 4.5 * np.sqrt(var[t] / C)
            m2 = var[t] + mean[t] ** 2
            v2 = 2.0 * var[t] ** 2 + 4.0 * mean[t] ** 2 * var[t]
            e2, b2 = abs((x[:, t] ** 2).mean() - m2), 4.5 * np.sqrt(v2 / C)
            print("invariance backward=%d t=%d  |mean - exact| %.3e (bound %.3e)  |m2 - exact| %.3e (bound %.3e)"
                  % (bw, t, e1, b1, e2, b2))
            assert e1 < b1 and e2 < b2, (bw, t, e1, b1, e2, b2)


# ---------------------------------------------------------------------------------------------------------------- 7
def _state(pf):
    out = [pf._summ().copy()]
    for i in range(pf.n_islands):
        for t in range(pf._n):
            out += [pf._history(_lib.FIELD_X, t, i), pf._history(_lib.FIELD_LW, t, i)]
            if t:
                out.append(pf._history(_lib.FIELD_A, t, i))
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def check_lifecycle(golden, N=257, C=3):
    fk, thetas, y = make_fk(golden, "sv", C)
    xstar = -1.0 + 0.3 * np.random.default_rng(8).standard_normal((C, T6))
    plain = lambda: pa.SMC(fk=make_fk(golden, "sv", C)[0], N=N, ESSrmin=0.9, seed=9, collect="off", store_history=True)
    before = plain()
    before.run()
    mk = lambda: mcmc.CSMC(fk=fk, N=N, ESSrmin=0.95, xstar=xstar, seed=31, n_islands=C)
    a = mk()
    a.run()
    sa = _state(a)
    b = mk()
    b.run()
    assert _same(sa, _state(b))                                               # same seed, same bits
    c = mk()
    c.step_async(2)
    c.step_async(1)
    q = pickle.loads(pickle.dumps(c))                                         # mid-run
    d = copy.deepcopy(c)
    _lib.check(_lib.lib().smc_filter_reseed(d._f, 31))                        # (a deep copy is re-keyed: undo, to compare)
    for f in (c, q, d):
        assert describe(f) == "k_csmc_small" and f._n == 3
        f.step_async(T6)
        assert f._n == T6
    del c
    assert _same(sa, _state(q)) and _same(sa, _state(d))
    for i in range(C):
        assert np.array_equal(host_history(q, i)[0][:, 0], xstar[i])
    p1 = a.new_paths(backward_step=True, seed=3)
    assert np.array_equal(p1, q.new_paths(backward_step=True, seed=3))
    after = plain()
    after.run()
    assert describe(after) != "k_csmc_small" and _same(_state(before), _state(after))


# ---------------------------------------------------------------------------------------------------------------- 8
def _set_conditional(pf, T=T6):
    buf = pa.DeviceArray.from_numpy(np.zeros((pf.n_islands, T)))
    pf._keep_xstar = buf
    return _lib.lib().smc_filter_set_conditional(pf._f, buf.ptr)


def _paths_call(pf):
    out = np.empty((pf.n_islands, max(pf._n, 1)))
    return _lib.lib().smc_filter_csmc_paths(pf._f, 1, 1, None, None, None, out.ctypes.data_as(_lib.P(_lib.c_dbl)), None)


def check_refusals(golden):
    y = _y(golden, "lg_adaptive", T6)
    lgm = lambda: kalman.LinearGauss(rho=0.9, sigmaX=1.0, sigmaY=1.5)
    boot = lambda: ssm.Bootstrap(ssm=lgm(), data=y)
    kw = dict(N=300, resampling="multinomial", store_history=True, collect="off", seed=3)
    ok = pa.SMC(fk=boot(), **kw)
    assert _set_conditional(ok) == 0 and describe(ok) == "k_csmc_small"
    with pytest.raises(ValueError, match="profiled"):
        _lib.check(_lib.lib().smc_filter_profile(ok._f, 1))
    ok.run()
    assert np.all(ok._history(_lib.FIELD_X, 3)[0] == 0.0)
    with pytest.raises(_lib.SmcError, match="before the first step"):
        _lib.check(_set_conditional(ok))
    lev_y = _y(golden, "svlev_boot", T6)
    mode = _lib.RNG_MODE[0]
    rs_mod.set_rng("philox")
    try:
        sq = pa.SMC(fk=boot(), N=256, qmc=True, seed=3, collect="off")
    finally:
        rs_mod.set_rng(mode)
    assert sq._fused
    refused = {
        "bootstrap": pa.SMC(fk=ssm.GuidedPF(ssm=lgm(), data=y), **kw),
        "bootstrap filters": pa.SMC(fk=ssm.Bootstrap(ssm=ssm.StochVolLeverage(phi=-0.5), data=lev_y), **kw),
        "N <= 1024": pa.SMC(fk=boot(), **dict(kw, N=1025)),
        "multinomial": pa.SMC(fk=boot(), **dict(kw, resampling="systematic")),
        "whole history": pa.SMC(fk=boot(), **dict(kw, store_history=False)),
        "keep_history": pa.SMC(fk=boot(), **dict(kw, store_history=3)),
        "moments": pa.SMC(fk=boot(), **dict(kw, collect=[collectors.Moments()])),
        "STRICT": pa.SMC(fk=boot(), strict_ancestors=True, **kw),
        "SQMC": sq,
        "use_graph": pa.SMC(fk=boot(), use_graph=True, **kw),
    }
    for what, pf in refused.items():
        assert pf._fused, what
        with pytest.raises(ValueError, match=what):
            _lib.check(_set_conditional(pf))
        pf.run()                                            # ... and runs on as the filter it was
        assert describe(pf) != "k_csmc_small"
    with pytest.raises(ValueError, match="null"):
        _lib.check(_lib.lib().smc_filter_set_conditional(pa.SMC(fk=boot(), **kw)._f, None))
    # the paths entry
    for what, key in (("N <= 1024", "N <= 1024"), ("whole history", "whole history"), ("whole history", "keep_history"),
                      ("not supported", "bootstrap filters"), ("SQMC", "SQMC")):
        with pytest.raises(ValueError, match=what):
            _lib.check(_paths_call(refused[key]))
    fresh = pa.SMC(fk=boot(), **kw)
    with pytest.raises(ValueError, match="no step"):
        _lib.check(_paths_call(fresh))
    with pytest.raises(ValueError, match="no output"):
        _lib.check(_lib.lib().smc_filter_csmc_paths(ok._f, 1, 1, None, None, None, None, None))
    assert _paths_call(refused["bootstrap"]) == 0           # a guided filter's history is one backward sampling takes
    with pytest.raises(ValueError, match="shape"):
        mcmc.new_paths(ok, replay={"u_last": np.zeros(2)})
    with pytest.raises(ValueError, match="unknown"):
        mcmc.new_paths(ok, replay={"u_acc": np.zeros(1)})

    # ---- the Python class: what the device does not pin runs the reference's overrides on the template-method step
    xs = np.linspace(-1.0, 1.0, T6)

    class MyLG(kalman.LinearGauss):
        def PY(self, t, xp, x):
            return kalman.LinearGauss.PY(self, t, xp, x)

    g4 = golden("mv4_boot")
    host = {
        "guided": (ssm.GuidedPF(ssm=lgm(), data=y), 200, xs),
        "leverage": (ssm.Bootstrap(ssm=ssm.StochVolLeverage(phi=-0.5), data=lev_y), 200, xs),
        "N > 1024": (boot(), 1025, xs),
        "user model": (ssm.Bootstrap(ssm=MyLG(rho=0.9, sigmaX=1.0, sigmaY=1.5), data=y), 200, xs),
        "multivariate": (ssm.Bootstrap(ssm=kalman.MVLinearGauss_Guarniero_etal(alpha=0.4, dx=4), data=list(g4["y"])[:T6]), 200,
                         np.tile(xs[:, None], (1, 4))),
    }
    for what, (fk, N, xstar) in host.items():
        pf = mcmc.CSMC(fk=fk, N=N, xstar=xstar, ESSrmin=0.9)
        assert not pf._fused, what
        np.random.seed(4)
        pf.run()
        assert pf.t == T6 and len(pf.hist.X) == T6, what
        assert all(np.array_equal(np.asarray(pf.hist.X[t])[0], xstar[t]) for t in range(T6)), what
        assert all(np.asarray(pf.hist.A[t])[0] == 0 for t in range(1, T6)), what
        with pytest.raises(ValueError, match="n_islands"):
            mcmc.CSMC(fk=fk, N=N, xstar=xstar, n_islands=2)
        with pytest.raises(ValueError, match="xstar"):
            mcmc.CSMC(fk=fk, N=N, xstar=xstar[:-1])
    p = mcmc.new_paths(pf)
    assert p.shape[:2] == (1, T6)
    for bad in (np.zeros(T6 - 1), np.zeros((2, T6)), np.zeros((T6, 2))):
        with pytest.raises(ValueError, match="xstar"):
            mcmc.CSMC(fk=boot(), N=100, xstar=bad)
    with pytest.raises(ValueError, match="xstar"):
        mcmc.CSMC(fk=boot(), N=100, xstar=np.zeros((2, T6)), n_islands=3)
    with pytest.raises(ValueError, match="xstar"):
        mcmc.CSMC(fk=boot(), N=100, xstar=pa.DeviceArray.from_numpy(np.zeros((3, T6))), n_islands=2)
