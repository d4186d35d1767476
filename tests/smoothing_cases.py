"""Backward sampling on the device (DeviceParticleHistory.backward_sampling_ON2 / backward_sampling_mcmc,
smc_filter_backward_sample, particles_amd/csrc/smc_smooth.h): the checks behind tests/test_smoothing_gpu.py (MI355X)
and tests/test_smoothing_emu.py (emulator build, smaller M), in the manner of lazy_lw_cases.py.

  pinned      the reference's own backward_sampling_ON2 on the `history` case (tests/golden/ffbs_lg.npz, written by
              tests/golden/make_golden_ffbs.py): the same indices from the same uniforms.
  restated    row t of the device against the reference's expression evaluated in NumPy on the device's own row t + 1
              (teacher forcing): scipy.stats.norm.logpdf, exp_and_normalise, searchsorted(cumsum(W), u), the Metropolis
              rule.  A difference must be a certified near-tie: every step of the fp64 CDF between the two indices within
              1e-11 of the uniform (the integer CDF and a sequential fp64 sum differ by N ulp), or |log u_acc - ratio| <
              1e-9 (device log and logpdf against NumPy's: a few ulp of values of size <= 1e3).  Certified differences
              <= near_tie_allowance(draws); others: none.
  philox      Philox mode is replay mode fed with the documented streams.
  law         means of FFBS trajectories against the exact smoothing marginals of the particle approximation.
  refusals    what the C entry refuses, and that sampling leaves the filter as it was.
"""
import numpy as np
import pytest
import scipy.stats

import particles_amd as pa
import parity_cases as pc
from oracle import smc_oracle as orc
from particles_amd import _lib
from particles_amd import kalman
from particles_amd import resampling as rs_mod
from particles_amd import state_space_models as ssm

LG = dict(rho=0.9, sigmaX=1.0, sigmaY=1.5)


# log p_t(x | xp) of the reference's models (PX(t, xp).logpdf(x), state_space_models.py:341): (loc(t, xp), scale)
def _lg_px(rho=0.9, sigmaX=1.0):
    return lambda t, xp: (rho * xp, sigmaX)                                             # kalman.py:430-431


def _sv_px(mu=-1.02, rho=0.9702, sigma=0.178):
    return lambda t, xp: ((1.0 - rho) * mu + rho * xp, sigma)                           # ssm.py:465-470


def _gordon_px(b=0.5, c=25.0, d=8.0, e=1.2, sigmaX=3.162278):
    return lambda t, xp: (b * xp + c * xp / (1.0 + xp ** 2) + d * np.cos(e * (t - 1)), sigmaX)   # ssm.py:568-574


def _theta_px(tau0=0.15, tau1=0.12, tau2=0.1, sigmaX=0.47):
    return lambda t, xp: (xp + tau0 - tau1 * np.exp(tau2 * xp), sigmaX)                 # ssm.py:677-680


def _cox_px(mu=0.5, sigma=0.4, phi=0.9):
    return lambda t, xp: (mu + phi * (xp - mu), sigma)                                  # ssm.py:626-627


def _y(golden, name, T):
    y = np.squeeze(golden(name)["y"])[:T]
    assert len(y) == T
    return [np.atleast_1d(v) for v in y]


def _boot(model, golden, data, T):
    return ssm.Bootstrap(ssm=model, data=_y(golden, data, T))


# name -> (filter factory(golden), transition)
CASES = {
    "toy_4099": (lambda g: pa.SMC(fk=_boot(kalman.LinearGauss(**LG), g, "lg_adaptive", 6), N=4099, seed=17, ESSrmin=0.5,
                                  store_history=True, collect="off"), _lg_px()),
    "gordon_1501": (lambda g: pa.SMC(fk=_boot(ssm.Gordon_etal(), g, "gordon_boot", 8), N=1501, seed=18, ESSrmin=0.5,
                                     store_history=True, collect="off"), _gordon_px()),
    "sv_2500": (lambda g: pa.SMC(fk=_boot(ssm.StochVol(), g, "sv_systematic", 6), N=2500, seed=19, ESSrmin=0.95,
                                 store_history=True, collect="off"), _sv_px()),
    "theta_2500": (lambda g: pa.SMC(fk=_boot(ssm.ThetaLogistic(), g, "theta_boot", 6), N=2500, seed=20, ESSrmin=0.7,
                                    store_history=True, collect="off"), _theta_px()),
    "cox_2500": (lambda g: pa.SMC(fk=_boot(ssm.DiscreteCox(mu=0.5, sigma=0.4, phi=0.9), g, "cox_boot", 6), N=2500, seed=21,
                                  ESSrmin=0.8, store_history=True, collect="off"), _cox_px()),
    "guided_700": (lambda g: pa.SMC(fk=ssm.GuidedPF(ssm=kalman.LinearGauss(**LG), data=_y(g, "lg_adaptive", 6)), N=700,
                                    seed=22, ESSrmin=0.5, store_history=True, collect="off"), _lg_px()),
    "islands_3x1100": (lambda g: pa.SMC(fk=_boot(kalman.LinearGauss(**LG), g, "lg_adaptive", 6), N=1100, seed=23,
                                        ESSrmin=0.5, n_islands=3, store_history=True, collect="off"), _lg_px()),
    "sharp_1500": (lambda g: pa.SMC(fk=_boot(kalman.LinearGauss(rho=0.9, sigmaX=1.0, sigmaY=1e-3), g, "lg_adaptive", 5),
                                    N=1500, seed=24, ESSrmin=0.5, store_history=True, collect="off"), _lg_px()),
}
ISLAND = {"islands_3x1100": 2}
# (M of the ON2 call, M and nsteps of the MCMC call); between them every M in {1, 65, 257} and nsteps in {1, 3}
SHAPES = {
    "history": [(1, 257, 1), (65, 1, 3), (257, 65, 3)],
    "toy_4099": [(1, 257, 3), (65, 65, 1), (257, 1, 1)],
    "gordon_1501": [(65, 257, 3)],
    "sv_2500": [(65, 65, 3)],
    "theta_2500": [(1, 65, 1)],
    "cox_2500": [(65, 1, 3)],
    "guided_700": [(257, 65, 3)],
    "islands_3x1100": [(65, 257, 1)],
    "sharp_1500": [(65, 65, 3)],
}
# the emulator runs one workgroup at a time: the 257-trajectory ON2 calls stay at the one-tile sizes
SHAPES_EMU = dict(SHAPES, history=[(1, 257, 1), (65, 1, 3)], toy_4099=[(1, 257, 3), (65, 65, 1)],
                  islands_3x1100=[(33, 257, 1)], gordon_1501=[(33, 257, 3)], sv_2500=[(33, 65, 3)], cox_2500=[(33, 1, 3)],
                  sharp_1500=[(33, 65, 3)])

_RUNS = {}


def history_run(golden):
    """The forward pass of parity_cases.check_device_history: the reference's draws replayed, history bit-equal to
    tests/golden/history.npz.  Run once."""
    if "history" not in _RUNS:
        g = golden("history")
        mk_dev, mk_orc = pc.MODELS["lg_adaptive"]
        N, T = int(g["N"]), int(g["T"])
        y = list(g["y"])
        np.random.seed(int(g["run_seed"]))
        rec = orc.RecordingRNG()
        o = orc.run_filter(mk_orc(), y, N, "systematic", 0.5, rng=rec)
        assert o["final_logLt"] == float(g["logLt"])
        z, u = pc.tapes_from_oracle(rec.tape, T, N, "systematic")
        pf = pa.SMC(fk=ssm.Bootstrap(ssm=mk_dev(), data=y), N=N, resampling="systematic", ESSrmin=0.5, replay=(z, u),
                    store_history=True)
        pf.run()
        for t in range(T):
            assert np.array_equal(pf.hist.X[t], g["hist_X"][t]) and np.array_equal(pf.hist.wgts[t].lw, g["hist_lw"][t])
            assert t == 0 or np.array_equal(pf.hist.A[t], g["hist_A"][t - 1])
        _RUNS["history"] = pf
    return _RUNS["history"]


def run_of(golden, case):
    if case == "history":
        return history_run(golden), _lg_px()
    if case not in _RUNS:
        pf = CASES[case][0](golden)
        assert pf._fused and isinstance(pf.hist, pa.collectors.DeviceParticleHistory)
        pf.run()
        _RUNS[case] = pf
    return _RUNS[case], CASES[case][1]


_HOST = {}


def host_history(pf, island=0):
    """X, lw, W (T, N), A (T, N; row 0 unused), rs flags (T,) of one island, downloaded once per filter."""
    key = (id(pf), island)
    if key not in _HOST:
        T = pf._n
        X = np.array([pf._history(_lib.FIELD_X, t, island) for t in range(T)])
        lw = np.array([pf._history(_lib.FIELD_LW, t, island) for t in range(T)])
        W = np.array([pf._history(_lib.FIELD_W, t, island) for t in range(T)])
        flags = pf._summ()[island, :, 4] != 0
        A = np.array([pf._history(_lib.FIELD_A, t, island) if t else np.arange(pf.N) for t in range(T)])
        _HOST[key] = (X, lw, W, A, flags)
    return _HOST[key]


def logpt(px, t, xp, x):
    loc, scale = px(t, xp)
    return scipy.stats.norm.logpdf(x, loc=loc, scale=scale)


def _search(cs, u, W):
    """searchsorted(cumsum(W), u) (resampling.py:596); a uniform beyond the last step: the last positive weight."""
    n = np.searchsorted(cs, u)
    return np.minimum(n, np.flatnonzero(W > 0)[-1])


def _certified_index(cs, u, a, b):
    lo, hi = min(a, b), max(a, b)
    return bool(np.all(np.abs(cs[lo:hi] - u) < 1e-11))


def restate_on2(hist, px, idx, u, where):
    """Row t of idx against the reference's expression on the device's row t + 1.  Returns (certified, draws)."""
    X, lw, W, A, flags = hist
    T, M = idx.shape
    ties = 0
    for t in reversed(range(T - 1)):
        for m in range(M):
            lwm = lw[t] + logpt(px, t + 1, X[t], X[t + 1][idx[t + 1, m]])          # smoothing.py:307-309
            Wb = orc.exp_and_normalise(lwm)
            cs = np.cumsum(Wb)
            want = int(_search(cs, u[t, m], Wb))
            got = int(idx[t, m])
            assert Wb[got] > 0.0, (where, t, m, "a zero-weight particle was drawn")
            if got != want:
                assert _certified_index(cs, u[t, m], got, want), (where, t, m, got, want, u[t, m], cs[min(got, want)])
                ties += 1
    return ties, (T - 1) * M


def restate_mcmc(hist, px, idx, u_prop, u_acc, where):
    X, lw, W, A, flags = hist
    T, M = idx.shape
    nsteps = u_prop.shape[1]
    ties = 0
    for t in reversed(range(T - 1)):
        cs = np.cumsum(W[t])
        nxt = idx[t + 1]
        xn = X[t + 1][nxt]
        cur = A[t + 1][nxt] if flags[t + 1] else nxt.copy()                        # smoothing.py:342 (A = arange: core.py:336)
        near = np.zeros(M, dtype=bool)
        for i in range(nsteps):
            prop = _search(cs, u_prop[t, i], W[t])
            lpr = logpt(px, t + 1, X[t][prop], xn) - logpt(px, t + 1, X[t][cur], xn)   # smoothing.py:346-347
            lu = np.log(u_acc[t, i])
            near |= np.abs(lu - lpr) < 1e-9
            for m in range(M):          # a proposal uniform within 1e-11 of a step of the CDF next to the proposal
                p = int(prop[m])
                near[m] |= abs(cs[p] - u_prop[t, i, m]) < 1e-11 or (p > 0 and abs(cs[p - 1] - u_prop[t, i, m]) < 1e-11)
            cur = np.where(lu < lpr, prop, cur)                                    # smoothing.py:349
        bad = np.flatnonzero(cur != idx[t])
        assert np.all(near[bad]), (where, t, bad[:5], cur[bad][:5], idx[t][bad][:5])
        ties += len(bad)
        assert np.all(W[t][idx[t]] > 0.0) or not flags[t + 1], (where, t, "a zero-weight particle was drawn")
    return ties, (T - 1) * M * nsteps * 2


def check_pinned(golden):
    """The reference's own FFBS run: same last row and uniforms in, the same (T, M) indices and paths out."""
    pf = history_run(golden)
    g, fx = golden("history"), golden("ffbs_lg")
    M = int(fx["M"])
    paths, idx = pf.hist.backward_sampling_ON2(M, replay={"idx_last": fx["idx"][-1], "u": fx["u"]}, return_idx=True)
    assert idx.shape == fx["idx"].shape and idx.dtype == np.int64
    print("pinned: %d of %d indices differ" % (np.sum(idx != fx["idx"]), idx.size))
    assert np.array_equal(idx, fx["idx"])
    assert len(paths) == int(g["T"])
    for t in range(len(paths)):
        assert np.array_equal(paths[t], g["hist_X"][t][idx[t]]) and np.array_equal(paths[t], fx["paths"][t])


def check_restated(golden, case, emu=False):
    pf, px = run_of(golden, case)
    island = ISLAND.get(case, 0)
    hist = host_history(pf, island)
    X, lw, W = hist[0], hist[1], hist[2]
    T, N = X.shape
    rng = np.random.default_rng(11)
    if case == "sharp_1500":
        zero = (W == 0.0).mean(axis=1)
        assert zero.max() >= 0.1, zero
    for M_on2, M_mc, nsteps in (SHAPES_EMU if emu else SHAPES)[case]:
        u_last, u = rng.random(M_on2), rng.random((T - 1, M_on2))
        paths, idx = pf.hist.backward_sampling_ON2(M_on2, island=island, replay={"u_last": u_last, "u": u}, return_idx=True)
        assert idx.shape == (T, M_on2) and idx.min() >= 0 and idx.max() < N and len(paths) == T
        if M_on2 == 1:
            assert all(np.ndim(p) == 0 for p in paths)                              # (_output_backward_sampling)
        assert all(np.array_equal(np.atleast_1d(paths[t]), X[t][idx[t]]) for t in range(T))
        last = _search(np.cumsum(W[-1]), u_last, W[-1])
        d = np.flatnonzero(last != idx[-1])
        ties = len(d)
        assert all(_certified_index(np.cumsum(W[-1]), u_last[m], int(last[m]), int(idx[-1, m])) for m in d), (case, d)
        assert np.all(W[-1][idx[-1]] > 0.0)
        t2, draws = restate_on2(hist, px, idx, u, case)
        pc.log_near_ties("FFBS ON2 %s M=%d" % (case, M_on2), ties + t2, draws + M_on2)
        assert ties + t2 <= pc.near_tie_allowance(draws + M_on2)

        up, ua = rng.random((T - 1, nsteps, M_mc)), rng.random((T - 1, nsteps, M_mc))
        ua = np.maximum(ua, 2.0 ** -53)
        idx_last = rng.integers(0, N, M_mc) if case != "sharp_1500" else idx[-1][rng.integers(0, M_on2, M_mc)]
        paths, idx = pf.hist.backward_sampling_mcmc(M_mc, nsteps=nsteps, island=island, return_idx=True,
                                                    replay={"idx_last": idx_last, "u_prop": up, "u_acc": ua})
        assert idx.shape == (T, M_mc) and np.array_equal(idx[-1], idx_last) and idx.min() >= 0 and idx.max() < N
        assert all(np.array_equal(np.atleast_1d(paths[t]), X[t][idx[t]]) for t in range(T))
        t3, draws = restate_mcmc(hist, px, idx, up, ua, case)
        pc.log_near_ties("FFBS MCMC %s M=%d nsteps=%d" % (case, M_mc, nsteps), t3, draws)
        assert t3 <= pc.near_tie_allowance(draws)


def philox_tapes(seed, T, M, nsteps, island):
    """The documented streams: counter (i M + m, t, island, 3), word x01 -> [0, 1), word x23 -> (0, 1)."""
    u = np.empty((T, nsteps, M))
    ua = np.empty((T, nsteps, M))
    for t in range(T):
        for i in range(nsteps):
            x01, x23 = orc.philox_u64_pair(seed, np.arange(i * M, (i + 1) * M, dtype=np.uint32), t, island, 3)
            u[t, i], ua[t, i] = orc.u01_halfopen(x01), orc.u01_open(x23)
    return u, ua


def check_philox_streams(golden, M=65, nsteps=3, seed=20240607):
    pf, _ = run_of(golden, "toy_4099")
    T = pf._n
    u, ua = philox_tapes(seed, T, M, nsteps, 0)
    a = pf.hist.backward_sampling_ON2(M, seed=seed, return_idx=True)[1]
    b = pf.hist.backward_sampling_ON2(M, replay={"u_last": u[T - 1, 0], "u": u[:T - 1, 0]}, return_idx=True)[1]
    assert np.array_equal(a, b)
    assert not np.array_equal(a, pf.hist.backward_sampling_ON2(M, seed=seed + 1, return_idx=True)[1])
    a = pf.hist.backward_sampling_mcmc(M, nsteps=nsteps, seed=seed, return_idx=True)[1]
    b = pf.hist.backward_sampling_mcmc(M, nsteps=nsteps, return_idx=True,
                                       replay={"u_last": u[T - 1, 0], "u_prop": u[:T - 1], "u_acc": ua[:T - 1]})[1]
    assert np.array_equal(a, b)
    # another island of a filter: its own counter word
    pf3, _ = run_of(golden, "islands_3x1100")
    u, ua = philox_tapes(seed, pf3._n, M, 1, 2)
    a = pf3.hist.backward_sampling_ON2(M, seed=seed, island=2, return_idx=True)[1]
    b = pf3.hist.backward_sampling_ON2(M, island=2, replay={"u_last": u[-1, 0], "u": u[:-1, 0]}, return_idx=True)[1]
    assert np.array_equal(a, b)
    # seed=None: a fresh key per call
    c = pf.hist.backward_sampling_ON2(M, return_idx=True)[1]
    d = pf.hist.backward_sampling_ON2(M, return_idx=True)[1]
    assert not np.array_equal(c, d)


def exact_marginals(X, W, px):
    """The smoothing marginals of the particle approximation by the O(T N^2) backward recursion:
    W_{t|T}[n] = W_t[n] sum_j W_{t+1|T}[j] p(x_{t+1}^j | x_t^n) / sum_k W_t[k] p(x_{t+1}^j | x_t^k)."""
    T, N = X.shape
    S = np.empty((T, N))
    S[-1] = W[-1]
    for t in reversed(range(T - 1)):
        loc, scale = px(t + 1, X[t])
        P = scipy.stats.norm.pdf(X[t + 1][None, :], loc=loc[:, None], scale=scale)     # (n, j)
        den = W[t] @ P
        S[t] = W[t] * (P @ (S[t + 1] / den))
    return S


def check_law(golden, M):
    """FFBS trajectories are iid draws from the smoothing law of the particle approximation: at every t the mean of
    M of them lies within 4.5 standard errors of the exact marginal mean (30 steps: 2e-4 that an exact sampler fails)."""
    pf = history_run(golden)
    X, lw, W = host_history(pf)[:3]
    S = exact_marginals(X, W, _lg_px())
    assert np.allclose(S.sum(axis=1), 1.0, atol=1e-12)
    mean = (S * X).sum(axis=1)
    var = (S * X ** 2).sum(axis=1) - mean ** 2
    paths = pf.hist.backward_sampling_ON2(M, seed=424242)
    for t in range(X.shape[0]):
        err, bound = abs(np.mean(paths[t]) - mean[t]), 4.5 * np.sqrt(var[t] / M)
        print("law t=%2d  |mean - exact| = %.3e  bound %.3e" % (t, err, bound))
        assert err < bound, (t, err, bound)


def _c_call(pf, M=4, nsteps=1, method=0, island=0):
    T = max(pf._n, 1)
    idx = np.empty((T, max(M, 1)), dtype=np.int64)
    return _lib.lib().smc_filter_backward_sample(pf._f, island, method, M, nsteps, 1, None, None, None, None,
                                                 idx.ctypes.data_as(_lib.P(_lib.c_i64)), None)


def check_refusals(golden):
    y = _y(golden, "lg_adaptive", 6)
    lg = lambda: ssm.Bootstrap(ssm=kalman.LinearGauss(**LG), data=y)
    no_hist = pa.SMC(fk=lg(), N=700, seed=3, collect="off")
    no_hist.run()
    assert no_hist.hist is None
    with pytest.raises(ValueError, match="whole history"):
        _lib.check(_c_call(no_hist))
    rolling = pa.SMC(fk=lg(), N=700, seed=3, collect="off", store_history=3)
    rolling.run()
    assert isinstance(rolling.hist, pa.collectors.DeviceRollingParticleHistory)
    assert not hasattr(rolling.hist, "backward_sampling_ON2") and not hasattr(rolling.hist, "backward_sampling_mcmc")
    with pytest.raises(ValueError, match="whole history"):
        _lib.check(_c_call(rolling))
    mode = _lib.RNG_MODE[0]
    rs_mod.set_rng("philox")
    try:
        q = pa.SMC(fk=lg(), N=4096, qmc=True, seed=3, collect="off")
        qh = pa.SMC(fk=lg(), N=4096, qmc=True, seed=3, collect="off", store_history=True)
    finally:
        rs_mod.set_rng(mode)
    assert q._fused
    q.run()
    with pytest.raises(ValueError, match="SQMC"):
        _lib.check(_c_call(q))
    qh.run()
    with pytest.raises(ValueError, match="SQMC"):
        qh.hist.backward_sampling_ON2(4)
    with pytest.raises(ValueError, match="SQMC"):
        qh.hist.backward_sampling_mcmc(4)
    lev = pa.SMC(fk=ssm.Bootstrap(ssm=ssm.StochVolLeverage(phi=-0.5), data=_y(golden, "svlev_boot", 6)), N=700, seed=3,
                 collect="off", store_history=True)
    lev.run()
    assert isinstance(lev.hist, pa.collectors.DeviceParticleHistory)
    with pytest.raises(NotImplementedError, match="SVLEVERAGE"):
        lev.hist.backward_sampling_ON2(4)
    with pytest.raises(NotImplementedError, match="SVLEVERAGE"):
        lev.hist.backward_sampling_mcmc(4)
    g = golden("mv4_boot")
    mv = pa.SMC(fk=ssm.Bootstrap(ssm=kalman.MVLinearGauss_Guarniero_etal(alpha=0.4, dx=4), data=list(g["y"])[:4]), N=700,
                seed=3, collect="off", store_history=True)
    mv.run()
    with pytest.raises(NotImplementedError):
        mv.hist.backward_sampling_ON2(4)
    ok = pa.SMC(fk=lg(), N=700, seed=3, collect="off", store_history=True)
    with pytest.raises(ValueError, match="no step"):
        ok.hist.backward_sampling_ON2(4)
    ok.run()
    for bad in (lambda: ok.hist.backward_sampling_ON2(0), lambda: ok.hist.backward_sampling_mcmc(0),
                lambda: ok.hist.backward_sampling_mcmc(4, nsteps=0), lambda: ok.hist.backward_sampling_ON2(4, island=1),
                lambda: ok.hist.backward_sampling_ON2(4, replay={"u": np.zeros((2, 4))}),
                lambda: ok.hist.backward_sampling_ON2(4, replay={"u_acc": np.zeros((5, 4))}),
                lambda: ok.hist.backward_sampling_ON2(4, replay={"idx_last": np.full(4, 700)})):
        with pytest.raises(ValueError):
            bad()


def _state(pf):
    out = [pf._summ().copy()]
    for f in (_lib.FIELD_X, _lib.FIELD_LW, _lib.FIELD_A):
        out.append(pf._get(f, 0).copy())
    for t in range(pf._n):
        out += [pf._history(_lib.FIELD_X, t), pf._history(_lib.FIELD_LW, t)]
        if t:
            out.append(pf._history(_lib.FIELD_A, t))
    return out


def check_non_interference(golden, N=3000, T=30, k=10):
    """Sampling after k of T steps: k rows out, and the filter finishes as the uninterrupted run does."""
    y = _y(golden, "lg_adaptive", T)
    mk = lambda: pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(**LG), data=y), N=N, seed=31, ESSrmin=0.5, collect="off",
                        store_history=True)
    a = mk()
    a.step_async(T)
    b = mk()
    b.step_async(k)
    before = _state(b)
    p1, i1 = b.hist.backward_sampling_ON2(33, seed=5, return_idx=True)
    p2, i2 = b.hist.backward_sampling_mcmc(33, nsteps=2, seed=5, return_idx=True)
    assert len(p1) == k == len(p2) and i1.shape == (k, 33) == i2.shape
    assert all(np.array_equal(p1[t], b.hist.X[t][i1[t]]) for t in range(k))
    after = _state(b)
    assert len(before) == len(after) and all(np.array_equal(u, v) for u, v in zip(before, after))
    b.step_async(T - k)
    sa, sb = _state(a), _state(b)
    assert len(sa) == len(sb) and all(np.array_equal(u, v) for u, v in zip(sa, sb))
    # one executed step: only the last row is drawn
    c = mk()
    c.step_async(1)
    p, i = c.hist.backward_sampling_mcmc(7, seed=1, return_idx=True)
    assert i.shape == (1, 7) and np.array_equal(p[0], c.hist.X[0][i[0]])
