"""Hybrid rejection backward sampling on the device (DeviceParticleHistory.backward_sampling_reject,
smc_filter_backward_reject, k_sm_reject_* of particles_amd/csrc/smc_smooth.h): the checks behind
tests/test_smoothing_reject_gpu.py (MI355X) and tests/test_smoothing_reject_emu.py (emulator build, smaller M),
built on smoothing_cases.py.

  restated    row t of the device against the contract of DESIGN section 6 evaluated in NumPy on the device's own row
              t + 1 (teacher forcing): trial i proposes searchsorted(cumsum(W_t), u_prop[i]) and is accepted iff
              log(u_acc[i]) < logpdf - logC; the smallest accepted i wins, else the exact draw.  A difference must be a
              certified near-tie (the criteria of smoothing_cases.py); where a step has none, nprops / nexact / acc_rate
              are equal exactly.  Before comparing, the restatement itself must reach the paths a case is there for.
  bounds      +inf / NaN: everything is the exact draw, equal to backward_sampling_ON2's; -inf: every first trial wins;
              a looser bound keeps the fused loop and the contract.
  philox      Philox mode is replay mode fed with the documented streams.
  law         means against the exact smoothing marginals, and against the reference's own sampler (golden file).
  refusals    what the C entry refuses, and that sampling leaves the filter as it was.
"""
import numpy as np
import pytest

import particles_amd as pa
import parity_cases as pc
import smoothing_cases as sc
from oracle import smc_oracle as orc
from particles_amd import _lib
from particles_amd import kalman
from particles_amd import resampling as rs_mod
from particles_amd import state_space_models as ssm

R = 4                 # SM_REJ_SOLO: trials of the one-thread-per-trajectory launch; the wave launch goes on in rounds of 64
WIDE = dict(rho=0.9, sigmaX=1.0, sigmaY=50.0, sigma0=20.0)

# (M, max_trials): max_trials below R, at R + 1 and across one and two rounds of the wave launch; M below, at and across
# a wave and a workgroup
SHAPES = {
    "toy_4099": [(1, 3), (65, 3), (257, 2), (65, 5)],
    "gordon_1501": [(65, 3)],
    "sv_2500": [(257, 2)],
    "guided_700": [(1, 3), (257, 2)],
    "islands_3x1100": [(65, 3)],
    "sharp_1500": [(65, 3)],
    "wide_1500": [(257, 130), (65, 70)],
}
# the emulator runs one workgroup at a time, and every fallback is one workgroup's O(N) draw
SHAPES_EMU = dict(SHAPES, toy_4099=[(1, 3), (65, 3), (65, 5)], sv_2500=[(129, 2)])
TAPE_SEED = {"wide_1500": 25}      # (a seed whose (65, 70) tapes hold an accept at trial 68 or 69: assert_reach)


def _wide(golden):
    return pa.SMC(fk=sc._boot(kalman.LinearGauss(**WIDE), golden, "lg_adaptive", 6), N=1500, seed=25, ESSrmin=0.5,
                  store_history=True, collect="off")


def run_of(golden, case):
    if case == "wide_1500":
        if case not in sc._RUNS:
            pf = _wide(golden)
            assert pf._fused and isinstance(pf.hist, pa.collectors.DeviceParticleHistory)
            pf.run()
            sc._RUNS[case] = pf
        return sc._RUNS[case], sc._lg_px()
    return sc.run_of(golden, case)


def bounds_of(pf):
    return np.array([pf.fk.upper_bound_trans(s) for s in range(1, pf._n)], dtype=np.float64)


def restate(hist, px, idx, logC, u_prop, u_acc, u, where):
    """Rows 0 .. T-2 of idx against the contract, each on the device's own row t + 1.  Returns the certified
    differences, the draws compared, the restated nprops / nexact, which steps had no difference, and the trial index
    every trajectory was resolved at (-1: the exact draw), all from NumPy alone."""
    X, lw, W, A, flags = hist
    T, M = idx.shape
    max_trials = u_prop.shape[1]
    ties = draws = 0
    nprops, nexact = np.zeros(T - 1, dtype=np.int64), np.zeros(T - 1, dtype=np.int64)
    clean = np.ones(T - 1, dtype=bool)
    resolved = np.empty((T - 1, M), dtype=np.int64)
    for t in reversed(range(T - 1)):
        cs = np.cumsum(W[t])
        xn = X[t + 1][idx[t + 1]]                                                   # (M,)
        prop = sc._search(cs, u_prop[t], W[t])                                      # (max_trials, M)
        lpr = sc.logpt(px, t + 1, X[t][prop], xn[None, :]) - logC[t]
        lu = np.log(u_acc[t])
        acc = lu < lpr
        near = np.abs(lu - lpr) < 1e-9
        near |= np.abs(cs[prop] - u_prop[t]) < 1e-11
        near |= (prop > 0) & (np.abs(cs[np.maximum(prop - 1, 0)] - u_prop[t]) < 1e-11)
        first = np.where(acc.any(axis=0), acc.argmax(axis=0), -1)
        resolved[t] = first
        ntrials = np.where(first >= 0, first + 1, max_trials)
        nprops[t], nexact[t] = ntrials.sum(), np.sum(first < 0)
        draws += int(nprops[t] + nexact[t])
        for m in range(M):
            got = int(idx[t, m])
            if first[m] >= 0:
                want, cert = int(prop[first[m], m]), bool(near[:ntrials[m], m].any())
            else:
                lwm = lw[t] + sc.logpt(px, t + 1, X[t], xn[m])                      # smoothing.py:418-421
                Wb = orc.exp_and_normalise(lwm)
                cb = np.cumsum(Wb)
                want = int(sc._search(cb, u[t, m], Wb))
                cert = bool(near[:, m].any()) or sc._certified_index(cb, u[t, m], got, want)
                assert Wb[got] > 0.0 or near[:, m].any(), (where, t, m, "a zero-weight particle was drawn")
            if got != want:
                assert cert, (where, t, m, got, want, int(first[m]))
                ties += 1
                clean[t] = False
    return ties, draws, nprops, nexact, clean, resolved


def assert_reach(case, max_trials, first):
    """The restatement (not the device) must reach what the case is there for: an accept and an exact draw; the
    low-acceptance case also an accept in the first launch, in the first round of the wave launch and in a later one."""
    assert np.any(first >= 0) and np.any(first < 0), (case, "needs an accept and a fallback")
    if case == "wide_1500":
        assert max_trials > 64 + R
        reach = [np.sum(first == 0), np.sum((first >= R) & (first < 64 + R)), np.sum(first >= 64 + R), np.sum(first < 0)]
        print("reach %s max_trials=%d: first trial %d, first round %d, later rounds %d, exact %d"
              % ((case, max_trials) + tuple(reach)))
        assert all(r >= 1 for r in reach), (case, max_trials, reach)


def check_one(pf, px, island, M, max_trials, rng, where, logC=None):
    hist = sc.host_history(pf, island)
    X, lw, W = hist[0], hist[1], hist[2]
    T, N = X.shape
    logC = bounds_of(pf) if logC is None else logC
    u_last, u = rng.random(M), rng.random((T - 1, M))
    up = rng.random((T - 1, max_trials, M))
    ua = np.maximum(rng.random((T - 1, max_trials, M)), 2.0 ** -53)
    paths, idx = pf.hist.backward_sampling_reject(M, max_trials=max_trials, island=island, return_idx=True,
                                                  replay={"u_last": u_last, "u_prop": up, "u_acc": ua, "u": u})
    assert idx.shape == (T, M) and idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < N and len(paths) == T
    if M == 1:
        assert all(np.ndim(p) == 0 for p in paths)                                  # (_output_backward_sampling)
    assert all(np.array_equal(np.atleast_1d(paths[t]), X[t][idx[t]]) for t in range(T))
    h = pf.hist
    assert h.acc_rate.shape == (T - 1,) and h.acc_rate.dtype == np.float64
    assert h.nprops.shape == (T - 1,) == h.nexact.shape and h.nprops.dtype == np.int64 == h.nexact.dtype
    cs_last = np.cumsum(W[-1])
    last = sc._search(cs_last, u_last, W[-1])
    d = np.flatnonzero(last != idx[-1])
    assert all(sc._certified_index(cs_last, u_last[m], int(last[m]), int(idx[-1, m])) for m in d), (where, d)
    assert np.all(W[-1][idx[-1]] > 0.0)
    ties, draws, nprops, nexact, clean, resolved = restate(hist, px, idx, logC, up, ua, u, where)
    pc.log_near_ties("FFBS reject %s M=%d max_trials=%d" % (where, M, max_trials), ties + len(d), draws + M)
    assert ties + len(d) <= pc.near_tie_allowance(draws + M)
    for t in np.flatnonzero(clean):
        assert h.nprops[t] == nprops[t] and h.nexact[t] == nexact[t], (where, t, h.nprops[t], nprops[t], h.nexact[t], nexact[t])
        assert h.acc_rate[t] == (M - nexact[t]) / nprops[t]
    return resolved


def check_restated(golden, case, emu=False):
    pf, px = run_of(golden, case)
    island = sc.ISLAND.get(case, 0)
    rng = np.random.default_rng(TAPE_SEED.get(case, 12))
    if case == "wide_1500":
        assert np.isclose(bounds_of(pf)[0], -0.5 * np.log(2.0 * np.pi))
    seen = []
    for M, max_trials in (SHAPES_EMU if emu else SHAPES)[case]:
        resolved = check_one(pf, px, island, M, max_trials, rng, case).ravel()
        if case == "wide_1500":
            assert_reach(case, max_trials, resolved)
        seen.append(resolved)
    if case != "wide_1500":                                                        # (over the case's shapes together)
        assert_reach(case, 0, np.concatenate(seen))


class _Bound(kalman.LinearGauss):
    BOUND = 0.0

    def upper_bound_log_pt(self, t):
        return self.BOUND


class _PlusInf(_Bound):
    BOUND = np.inf


class _NaN(_Bound):
    BOUND = np.nan


class _MinusInf(_Bound):
    BOUND = -np.inf


class _Loose(kalman.LinearGauss):
    def upper_bound_log_pt(self, t):
        return kalman.LinearGauss.upper_bound_log_pt(self, t) + np.log(4.0)


def _bounded_run(golden, cls, N=700):
    key = "bound_" + cls.__name__
    if key not in sc._RUNS:
        pf = pa.SMC(fk=sc._boot(cls(**sc.LG), golden, "lg_adaptive", 6), N=N, seed=26, ESSrmin=0.5, store_history=True,
                    collect="off")
        assert pf._fused and isinstance(pf.hist, pa.collectors.DeviceParticleHistory)      # the bound is the host's business
        pf.run()
        sc._RUNS[key] = pf
    return sc._RUNS[key]


def check_degenerate_bounds(golden):
    rng = np.random.default_rng(13)
    for cls in (_PlusInf, _NaN):
        pf = _bounded_run(golden, cls)
        T = pf._n
        for M, max_trials in ((65, 3), (33, 70)):
            u_last, u = rng.random(M), rng.random((T - 1, M))
            up, ua = rng.random((T - 1, max_trials, M)), np.maximum(rng.random((T - 1, max_trials, M)), 2.0 ** -53)
            want = pf.hist.backward_sampling_ON2(M, replay={"u_last": u_last, "u": u}, return_idx=True)[1]
            got = pf.hist.backward_sampling_reject(M, max_trials=max_trials, return_idx=True,
                                                   replay={"u_last": u_last, "u": u, "u_prop": up, "u_acc": ua})[1]
            assert np.array_equal(got, want), (cls.__name__, M, max_trials)
            assert np.array_equal(pf.hist.nexact, np.full(T - 1, M))
            assert np.array_equal(pf.hist.nprops, np.full(T - 1, M * max_trials))
            assert np.array_equal(pf.hist.acc_rate, np.zeros(T - 1))
    pf = _bounded_run(golden, _MinusInf)
    X, lw, W = sc.host_history(pf)[:3]
    T, M, max_trials = pf._n, 257, 3
    up, ua = rng.random((T - 1, max_trials, M)), np.maximum(rng.random((T - 1, max_trials, M)), 2.0 ** -53)
    idx = pf.hist.backward_sampling_reject(M, max_trials=max_trials, return_idx=True, replay={"u_prop": up, "u_acc": ua})[1]
    ties = 0
    for t in range(T - 1):
        cs = np.cumsum(W[t])
        want = sc._search(cs, up[t, 0], W[t])
        d = np.flatnonzero(want != idx[t])
        assert all(sc._certified_index(cs, up[t, 0, m], int(want[m]), int(idx[t, m])) for m in d), (t, d)
        ties += len(d)
    assert ties <= pc.near_tie_allowance((T - 1) * M)
    assert np.array_equal(pf.hist.nprops, np.full(T - 1, M)) and np.array_equal(pf.hist.nexact, np.zeros(T - 1, dtype=np.int64))
    assert np.array_equal(pf.hist.acc_rate, np.ones(T - 1))
    # a looser bound: honoured (the host evaluates it), on the fused loop, and still the contract
    pf = _bounded_run(golden, _Loose)
    assert pf._fused
    tight = kalman.LinearGauss(**sc.LG).upper_bound_log_pt(1)
    assert np.array_equal(bounds_of(pf), np.full(pf._n - 1, tight + np.log(4.0)))
    resolved = check_one(pf, sc._lg_px(), 0, 65, 5, rng, "loose")
    assert np.any(resolved >= 0) and np.any(resolved < 0)


def philox_tapes(seed, T, M, max_trials, island):
    """The documented streams: trial i from counter (m, t, island, 4 | i << 8), word x01 -> [0, 1), word x23 -> (0, 1);
    the last row and the exact draws from counter (m, t, island, 3), word x01."""
    m = np.arange(M, dtype=np.uint32)
    up, ua, u = np.empty((T, max_trials, M)), np.empty((T, max_trials, M)), np.empty((T, M))
    for t in range(T):
        u[t] = orc.u01_halfopen(orc.philox_u64_pair(seed, m, t, island, 3)[0])
        for i in range(max_trials):
            x01, x23 = orc.philox_u64_pair(seed, m, t, island, 4 | (i << 8))
            up[t, i], ua[t, i] = orc.u01_halfopen(x01), orc.u01_open(x23)
    return up, ua, u


def check_philox_streams(golden, M=65, seed=20240611):
    for case, max_trials in (("toy_4099", 3), ("islands_3x1100", 6)):      # (6: the wave launch draws from the stream too)
        pf, _ = run_of(golden, case)
        island = sc.ISLAND.get(case, 0)
        T = pf._n
        up, ua, u = philox_tapes(seed, T, M, max_trials, island)
        a = pf.hist.backward_sampling_reject(M, max_trials=max_trials, seed=seed, island=island, return_idx=True)[1]
        stats = (pf.hist.nprops.copy(), pf.hist.nexact.copy())
        print("philox %s: nprops %s nexact %s" % (case, stats[0], stats[1]))
        b = pf.hist.backward_sampling_reject(M, max_trials=max_trials, island=island, return_idx=True,
                                             replay={"u_last": u[T - 1], "u": u[:T - 1], "u_prop": up[:T - 1],
                                                     "u_acc": ua[:T - 1]})[1]
        assert np.array_equal(a, b), case
        assert np.array_equal(stats[0], pf.hist.nprops) and np.array_equal(stats[1], pf.hist.nexact)
        c = pf.hist.backward_sampling_reject(M, max_trials=max_trials, seed=seed + 1, island=island, return_idx=True)[1]
        assert not np.array_equal(a, c)
    # seed=None: a fresh key per call
    pf, _ = run_of(golden, "toy_4099")
    c = pf.hist.backward_sampling_reject(M, return_idx=True)[1]
    d = pf.hist.backward_sampling_reject(M, return_idx=True)[1]
    assert not np.array_equal(c, d)


_MARGINALS = {}


def _marginals(golden):
    if not _MARGINALS:
        pf = sc.history_run(golden)
        X, lw, W = sc.host_history(pf)[:3]
        S = sc.exact_marginals(X, W, sc._lg_px())
        assert np.allclose(S.sum(axis=1), 1.0, atol=1e-12)
        mean = (S * X).sum(axis=1)
        _MARGINALS["mv"] = (mean, (S * X ** 2).sum(axis=1) - mean ** 2)
    return _MARGINALS["mv"]


def check_law(golden, M):
    """The hybrid has exactly the FFBS law, whatever max_trials: at every t the mean of M trajectories lies within 4.5
    standard errors of the exact marginal mean (check_law of smoothing_cases.py: the bound is the marginal variance's)."""
    pf = sc.history_run(golden)
    mean, var = _marginals(golden)
    T = len(mean)
    for max_trials, seed in ((2, 515151), (M, 525252)):
        paths = pf.hist.backward_sampling_reject(M, max_trials=max_trials, seed=seed)
        h = pf.hist
        print("law max_trials=%d  acc_rate %s  nexact %s" % (max_trials, np.round(h.acc_rate, 3), h.nexact))
        assert np.all(h.acc_rate > 0.0) and np.all(h.acc_rate <= 1.0) and np.all(h.nprops >= M)
        for t in range(T):
            err, bound = abs(np.mean(paths[t]) - mean[t]), 4.5 * np.sqrt(var[t] / M)
            print("law max_trials=%d t=%2d  |mean - exact| = %.3e  bound %.3e" % (max_trials, t, err, bound))
            assert err < bound, (max_trials, t, err, bound)


def check_pinned_in_law(golden, M=4096):
    """The reference's own backward_sampling_reject (tests/golden/ffbs_reject_lg.npz, make_golden_reject.py): two
    independent samples of the same law, so the per-step means differ by less than 4.5 sd of their difference."""
    pf = sc.history_run(golden)
    fx = golden("ffbs_reject_lg")
    M_ref = int(fx["M"])
    mean, var = _marginals(golden)
    paths = pf.hist.backward_sampling_reject(M, seed=535353)
    acc = pf.hist.acc_rate
    for t in range(len(mean)):
        err, bound = abs(np.mean(paths[t]) - fx["path_means"][t]), 4.5 * np.sqrt(var[t] * (1.0 / M + 1.0 / M_ref))
        print("pinned t=%2d  |mean - reference's| = %.3e  bound %.3e   acc_rate %s"
              % (t, err, bound, "device %.4f  reference %.4f" % (acc[t], fx["acc_rate"][t]) if t < len(acc) else "-"))
        assert err < bound, (t, err, bound)
    assert acc.shape == fx["acc_rate"].shape
    assert np.all((acc > 0.0) & (acc <= 1.0)) and np.all((fx["acc_rate"] > 0.0) & (fx["acc_rate"] <= 1.0))


def _c_call(pf, M=4, max_trials=3, island=0, bound=True):
    T = max(pf._n, 1)
    idx = np.empty((T, max(M, 1)), dtype=np.int64)
    lb = np.zeros(T)
    return _lib.lib().smc_filter_backward_reject(pf._f, island, M, max_trials, 1,
                                                 lb.ctypes.data_as(_lib.P(_lib.c_dbl)) if bound else None,
                                                 None, None, None, None, None,
                                                 idx.ctypes.data_as(_lib.P(_lib.c_i64)), None, None, None)


def check_refusals(golden):
    y = sc._y(golden, "lg_adaptive", 6)
    lg = lambda: ssm.Bootstrap(ssm=kalman.LinearGauss(**sc.LG), data=y)
    no_hist = pa.SMC(fk=lg(), N=700, seed=3, collect="off")
    no_hist.run()
    with pytest.raises(ValueError, match="whole history"):
        _lib.check(_c_call(no_hist))
    rolling = pa.SMC(fk=lg(), N=700, seed=3, collect="off", store_history=3)
    rolling.run()
    assert not hasattr(rolling.hist, "backward_sampling_reject")
    with pytest.raises(ValueError, match="whole history"):
        _lib.check(_c_call(rolling))
    mode = _lib.RNG_MODE[0]
    rs_mod.set_rng("philox")
    try:
        q = pa.SMC(fk=lg(), N=4096, qmc=True, seed=3, collect="off")
        qh = pa.SMC(fk=lg(), N=4096, qmc=True, seed=3, collect="off", store_history=True)
    finally:
        rs_mod.set_rng(mode)
    q.run()
    with pytest.raises(ValueError, match="SQMC"):
        _lib.check(_c_call(q))
    qh.run()
    with pytest.raises(ValueError, match="SQMC"):
        qh.hist.backward_sampling_reject(4)
    lev = pa.SMC(fk=ssm.Bootstrap(ssm=ssm.StochVolLeverage(phi=-0.5), data=sc._y(golden, "svlev_boot", 6)), N=700, seed=3,
                 collect="off", store_history=True)
    lev.run()
    with pytest.raises(NotImplementedError, match="SVLEVERAGE"):
        lev.hist.backward_sampling_reject(4)
    g = golden("mv4_boot")
    mv = pa.SMC(fk=ssm.Bootstrap(ssm=kalman.MVLinearGauss_Guarniero_etal(alpha=0.4, dx=4), data=list(g["y"])[:4]), N=700,
                seed=3, collect="off", store_history=True)
    mv.run()
    with pytest.raises(NotImplementedError):
        mv.hist.backward_sampling_reject(4)
    with pytest.raises(ValueError, match="MVLINGAUSS"):
        _lib.check(_c_call(mv))
    with pytest.raises(NotImplementedError, match="upper_bound_log_pt"):
        ssm.StateSpaceModel().upper_bound_log_pt(1)
    ok = pa.SMC(fk=lg(), N=700, seed=3, collect="off", store_history=True)
    with pytest.raises(ValueError, match="no step"):
        ok.hist.backward_sampling_reject(4)
    ok.run()
    with pytest.raises(ValueError, match="log_bound"):
        _lib.check(_c_call(ok, bound=False))
    with pytest.raises(ValueError, match="max_trials"):
        _lib.check(_c_call(ok, max_trials=0))
    for bad in (lambda: ok.hist.backward_sampling_reject(0), lambda: ok.hist.backward_sampling_reject(4, max_trials=0),
                lambda: ok.hist.backward_sampling_reject(4, island=1),
                lambda: ok.hist.backward_sampling_reject(4, max_trials=3, replay={"u_prop": np.zeros((5, 4))}),
                lambda: ok.hist.backward_sampling_reject(4, max_trials=3, replay={"u_acc": np.zeros((5, 2, 4))}),
                lambda: ok.hist.backward_sampling_reject(4, replay={"u": np.zeros((2, 4))}),
                lambda: ok.hist.backward_sampling_reject(4, replay={"u_step": np.zeros((5, 4))}),
                lambda: ok.hist.backward_sampling_reject(4, replay={"idx_last": np.full(4, 700)})):
        with pytest.raises(ValueError):
            bad()
    # the cap: "pure rejection" is served as 2^24 - 1 trials, then the exact draw
    paths = ok.hist.backward_sampling_reject(4, max_trials=np.inf, seed=9)
    assert len(paths) == ok._n and np.all(ok.hist.nexact == 0)
    host = pa.collectors.ParticleHistory(lg(), False)
    with pytest.raises(NotImplementedError):
        host.backward_sampling_reject(4)


def check_non_interference(golden, N=3000, T=30, k=10):
    """Sampling after k of T steps: k rows out, and the filter finishes as the uninterrupted run does."""
    y = sc._y(golden, "lg_adaptive", T)
    mk = lambda: pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(**sc.LG), data=y), N=N, seed=31, ESSrmin=0.5,
                        collect="off", store_history=True)
    a = mk()
    a.step_async(T)
    b = mk()
    b.step_async(k)
    before = sc._state(b)
    p1, i1 = b.hist.backward_sampling_reject(33, max_trials=2, seed=5, return_idx=True)
    p2, i2 = b.hist.backward_sampling_reject(33, max_trials=70, seed=5, return_idx=True)
    assert len(p1) == k == len(p2) and i1.shape == (k, 33) == i2.shape and b.hist.acc_rate.shape == (k - 1,)
    assert all(np.array_equal(p1[t], b.hist.X[t][i1[t]]) for t in range(k))
    after = sc._state(b)
    assert len(before) == len(after) and all(np.array_equal(u, v) for u, v in zip(before, after))
    b.step_async(T - k)
    sa, sb = sc._state(a), sc._state(b)
    assert len(sa) == len(sb) and all(np.array_equal(u, v) for u, v in zip(sa, sb))
    # one executed step: only the last row is drawn
    c = mk()
    c.step_async(1)
    p, i = c.hist.backward_sampling_reject(7, seed=1, return_idx=True)
    assert i.shape == (1, 7) and np.array_equal(p[0], c.hist.X[0][i[0]])
    assert c.hist.acc_rate.shape == (0,) and c.hist.nprops.shape == (0,) == c.hist.nexact.shape
