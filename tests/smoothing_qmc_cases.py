"""QMC backward sampling (ParticleHistory / DeviceParticleHistory.backward_sampling_qmc, smc_filter_backward_qmc,
particles_amd/csrc/smc_smooth_qmc.h): the checks behind tests/test_smoothing_qmc_gpu.py (MI355X),
tests/test_smoothing_qmc_emu.py (emulator build, smaller M) and tests/test_smoothing_qmc_host.py (CPU only), in the
manner of smoothing_cases.py.

  restate_qmc  the reference's method (smoothing.py:438-456) in plain NumPy: np.argsort(kind="stable"),
               scipy.stats.norm.logpdf, exp_and_normalise, searchsorted(cumsum(.), u).  On the fixture
               tests/golden/ffbs_qmc_lg.npz (the reference's own run, written by tests/golden/make_golden_ffbs_qmc.py) it
               gives the reference's paths and h_orders exactly; everywhere else it is the reference.
  restated     row t of the device's idx against the restated draw made from the device's own row t + 1 (teacher forcing)
               on the downloaded history.  A difference must be a certified near-tie: every step of the fp64 CDF IN
               SORTED ORDER between the two positions within 1e-11 of the uniform (smoothing_cases._certified_index).
               Certified differences <= near_tie_allowance(draws); others: none.
  geometries   workgroup-per-trajectory and thread-per-trajectory launches return array_equal indices.
  property     the mean of M QMC trajectories against the exact smoothing marginal, within 1.0 iid standard error.
  refusals     what the entry and the method refuse, and that sampling leaves the filter as it was.

Cases: every kind the issue names is taken by the fused SQMC with history; none was swapped.
"""
import numpy as np
import pytest
import scipy.stats

import particles_amd as pa
import parity_cases as pc
import smoothing_cases as sc
from oracle import smc_oracle as orc
from particles_amd import _lib
from particles_amd import kalman
from particles_amd import resampling as rs_mod
from particles_amd import rqmc
from particles_amd import state_space_models as ssm

REF_MSG = "QMC FFBS requires particles have been Hilbert ordered during the forward pass"
T_CASE = 6
MS = (1, 65, 257, 300)


def _philox(make):
    """SQMC runs fused with device-generated points only: construct in Philox mode."""
    mode = _lib.RNG_MODE[0]
    rs_mod.set_rng("philox")
    try:
        return make()
    finally:
        rs_mod.set_rng(mode)


def _sqmc(model, golden, data, N, seed, T=T_CASE, **kw):
    return _philox(lambda: pa.SMC(fk=sc._boot(model, golden, data, T), N=N, qmc=True, seed=seed, store_history=True,
                                  collect="off", **kw))


# name -> (filter factory(golden), transition)
CASES = {
    "lg_2048": (lambda g: _sqmc(kalman.LinearGauss(**sc.LG), g, "lg_adaptive", 2048, 41), sc._lg_px()),
    "lg_4096": (lambda g: _sqmc(kalman.LinearGauss(**sc.LG), g, "lg_adaptive", 4096, 42), sc._lg_px()),
    "sv_2048": (lambda g: _sqmc(ssm.StochVol(), g, "sv_systematic", 2048, 43), sc._sv_px()),
    "gordon_2048": (lambda g: _sqmc(ssm.Gordon_etal(), g, "gordon_boot", 2048, 44), sc._gordon_px()),
    "sharp_2048": (lambda g: _sqmc(kalman.LinearGauss(rho=0.9, sigmaX=1.0, sigmaY=1e-3), g, "lg_adaptive", 2048, 45),
                   sc._lg_px()),
    "islands_2x2048": (lambda g: _sqmc(kalman.LinearGauss(**sc.LG), g, "lg_adaptive", 2048, 46, n_islands=2), sc._lg_px()),
}
ISLAND = {"islands_2x2048": 1}
_RUNS, _HOST = {}, {}


def run_of(golden, case):
    if case not in _RUNS:
        pf = CASES[case][0](golden)
        assert pf._fused and pf.qmc and isinstance(pf.hist, pa.collectors.DeviceParticleHistory)
        pf.run()
        _RUNS[case] = pf
    return _RUNS[case], CASES[case][1]


def host_history(pf, island=0):
    """X, lw, W (T, N) of one island, downloaded once per filter."""
    key = (id(pf), island)
    if key not in _HOST:
        T = pf._n
        _HOST[key] = tuple(np.array([pf._history(f, t, island) for t in range(T)])
                           for f in (_lib.FIELD_X, _lib.FIELD_LW, _lib.FIELD_W))
    return _HOST[key]


def _positions(cw, u, Wb):
    """searchsorted(cumsum(W), u); a uniform beyond the last step: the last positive weight."""
    return np.minimum(np.searchsorted(cw, u), np.flatnonzero(Wb > 0)[-1])


def restate_qmc(X, lw, W, u, px):
    """smoothing.py:438-456 on arrays: X, lw, W (T, N), u (M, T), px the transition (loc, scale).  Returns
    (paths list of T arrays (M,), idx (T, M) particle indices, h_orders (T, N) -- the reference keeps rows 0 .. T - 2)."""
    T, N = X.shape
    M = u.shape[0]
    h = np.array([np.argsort(X[t], kind="stable") for t in range(T)])
    idx = np.empty((T, M), dtype=np.int64)
    pos = np.searchsorted(np.cumsum(W[-1][h[-1]]), u[:, -1])
    idx[-1] = h[-1][pos]
    paths = [X[-1][h[-1]][pos]]
    for t in reversed(range(T - 1)):
        loc, scale = px(t + 1, X[t])
        pos = np.empty(M, dtype=np.int64)
        for m, xn in enumerate(paths[-1]):
            lwm = lw[t] + scipy.stats.norm.logpdf(xn, loc=loc, scale=scale)
            cw = np.cumsum(orc.exp_and_normalise(lwm[h[t]]))
            pos[m] = np.searchsorted(cw, u[m, t])
        idx[t] = h[t][pos]
        paths.append(X[t][h[t]][pos])
    paths.reverse()
    return paths, idx, h


def restate_rows(hist, px, idx, u, where, cols=None):
    """Every row of idx (columns `cols`: all) against the restated draw from the row behind it.  Returns
    (certified, draws)."""
    X, lw, W = hist
    T, M = idx.shape
    N = X.shape[1]
    cols = range(M) if cols is None else cols
    ties = 0
    for t in reversed(range(T)):
        h = np.argsort(X[t], kind="stable")
        inv = np.empty(N, dtype=np.int64)
        inv[h] = np.arange(N)
        if t < T - 1:
            loc, scale = px(t + 1, X[t])
        for m in cols:
            if t == T - 1:
                Wb = W[t][h]
            else:
                lwm = lw[t] + scipy.stats.norm.logpdf(X[t + 1][idx[t + 1, m]], loc=loc, scale=scale)
                Wb = orc.exp_and_normalise(lwm[h])
            cw = np.cumsum(Wb)
            want = int(_positions(cw, u[m, t], Wb))
            got = int(inv[idx[t, m]])
            assert Wb[got] > 0.0, (where, t, m, "a zero-weight particle was drawn")
            if got != want:
                assert sc._certified_index(cw, u[m, t], got, want), (where, t, m, got, want, u[m, t], cw[min(got, want)])
                ties += 1
    return ties, T * len(cols)


def check_fixture(golden):
    """The reference's own run: the restatement gives its paths and its h_orders exactly."""
    g = golden("ffbs_qmc_lg")
    paths, idx, h = restate_qmc(g["X"], g["lw"], g["W"], g["u"], sc._lg_px())
    T = g["X"].shape[0]
    assert g["h_orders"].shape == (T - 1, g["X"].shape[1])
    assert np.array_equal(h[:T - 1], g["h_orders"])
    print("fixture: %d of %d paths differ" % (np.sum(np.array(paths) != g["paths"]), g["paths"].size))
    assert np.array_equal(np.array(paths), g["paths"])
    assert all(np.array_equal(paths[t], g["X"][t][idx[t]]) for t in range(T))


def check_host_route(golden, N=256, T=6, M=64):
    """ParticleHistory.backward_sampling_qmc on an operator-path SQMC run (history on the host) equals the
    restatement on its own saved history, point for point."""
    pf = pa.SMC(fk=sc._boot(kalman.LinearGauss(**sc.LG), golden, "lg_adaptive", T), N=N, qmc=True, store_history=True,
                collect="off")
    assert isinstance(pf.hist, pa.collectors.ParticleHistory)
    pf.run()
    host = lambda a: np.asarray(a.get() if isinstance(a, _lib.DeviceArray) else a)
    X = np.array([host(x) for x in pf.hist.X])
    lw = np.array([host(w.lw) for w in pf.hist.wgts])
    W = np.array([host(w.W) for w in pf.hist.wgts])
    assert X.shape == (T, N) and len(pf.hist.h_orders) == T - 1
    u = rqmc.sobol_points(M, T, seed=9)
    paths, idx = pf.hist.backward_sampling_qmc(M, replay={"u": u}, return_idx=True)
    want_paths, want_idx, h = restate_qmc(X, lw, W, u, sc._lg_px())
    assert all(np.array_equal(host(pf.hist.h_orders[t]), h[t]) for t in range(T - 1))
    assert idx.shape == (T, M) and idx.dtype == np.int64 and len(paths) == T
    print("host route: %d of %d indices differ" % (np.sum(idx != want_idx), idx.size))
    assert np.array_equal(idx, want_idx)
    assert all(np.array_equal(paths[t], want_paths[t]) and paths[t].shape == (M,) for t in range(T))
    # seeded points: reproducible; seed=None: fresh
    a = pf.hist.backward_sampling_qmc(16, seed=3)
    b = pf.hist.backward_sampling_qmc(16, seed=3)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert np.array_equal(rqmc.sobol_points(16, T, 3), rqmc.sobol_points(16, T, 3))
    assert not np.array_equal(rqmc.sobol_points(16, T), rqmc.sobol_points(16, T))
    with pytest.raises(ValueError):
        pf.hist.backward_sampling_qmc(M, replay={"u": u[:, :-1]})
    with pytest.raises(ValueError):
        pf.hist.backward_sampling_qmc(M, replay={"v": u})
    # a history without h_orders: the reference's refusal
    bare = pa.collectors.ParticleHistory(None, False)
    assert not hasattr(bare, "h_orders")
    with pytest.raises(ValueError, match="Hilbert"):
        bare.backward_sampling_qmc(4)


def geometries_of(M, emu):
    """The emulator runs one workgroup at a time: it keeps the workgroup-per-trajectory launch at M <= 65."""
    return (1, 2) if not emu or M <= 65 else (2,)


def check_restated(golden, case, emu=False):
    pf, px = run_of(golden, case)
    island = ISLAND.get(case, 0)
    hist = host_history(pf, island)
    X, lw, W = hist
    T, N = X.shape
    assert T == T_CASE
    if case == "sharp_2048":
        zero = (W == 0.0).mean(axis=1)
        assert zero.max() >= 0.1, zero
    rng = np.random.default_rng(12)
    for M in MS:
        u = rng.random((M, T))
        got = {}
        for geo in geometries_of(M, emu):
            paths, idx = pf.hist.backward_sampling_qmc(M, island=island, replay={"u": u}, return_idx=True, geometry=geo)
            assert idx.shape == (T, M) and idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < N and len(paths) == T
            assert all(p.shape == (M,) for p in paths)                              # (not squeezed for M = 1)
            assert all(np.array_equal(paths[t], X[t][idx[t]]) for t in range(T))
            assert all(np.all(W[t][idx[t]] > 0.0) for t in range(T))
            got[geo] = idx
        if len(got) == 2:
            assert np.array_equal(got[1], got[2]), (case, M, np.argwhere(got[1] != got[2])[:5])
        idx = got[2]
        ties, draws = restate_rows(hist, px, idx, u, case)
        pc.log_near_ties("FFBS QMC %s M=%d" % (case, M), ties, draws)
        assert ties <= pc.near_tie_allowance(draws)


def check_h_orders(golden):
    pf, _ = run_of(golden, "lg_2048")
    X = host_history(pf)[0]
    T = X.shape[0]
    assert len(pf.hist.h_orders) == T - 1
    for t in (0, T - 2):
        h = pf.hist.h_orders[t]
        assert h.dtype == np.int64 and np.array_equal(h, np.argsort(X[t], kind="stable"))
    with pytest.raises(IndexError):
        pf.hist.h_orders[T - 1]
    plain, _ = sc.run_of(golden, "toy_4099")
    assert not hasattr(plain.hist, "h_orders")


def check_edges(golden, emu=False):
    """u = 0, the smallest positive double, u >= 1, in both geometries: a positive weight is drawn, and everything
    between it and the reference's searchsorted position carries no mass (the certificate, with u held to 1: the
    reference draws position 0 for u = 0 even where its weight is 0, the device never does).  Where the end weights of
    the last row are positive in fp64 the ends themselves are drawn."""
    pf, px = run_of(golden, "sharp_2048")
    hist = host_history(pf)
    X, lw, W = hist
    T, N = X.shape
    M = 65
    rng = np.random.default_rng(13)
    u = rng.random((M, T))
    u[0::5] = 0.0
    u[1::5] = 1.0
    u[2::5] = 5e-324
    u[3::5] = 1.5
    got = [pf.hist.backward_sampling_qmc(M, replay={"u": u}, return_idx=True, geometry=g)[1] for g in (1, 2)]
    assert np.array_equal(got[0], got[1])
    idx = got[0]
    assert all(np.all(W[t][idx[t]] > 0.0) for t in range(T))
    ties, draws = restate_rows(hist, px, idx, u, "edges (interior columns)", cols=range(4, M, 5))
    assert ties <= pc.near_tie_allowance(draws)
    restate_rows(hist, px, idx, np.minimum(u, 1.0), "edges", cols=[m for m in range(M) if m % 5 != 4])
    # the last row: every weight outside the drawn ends rounds to 0 in the integer CDF (q = rint(W 2^50) at N = 2048)
    h = np.argsort(X[-1], kind="stable")
    inv = np.empty(N, dtype=np.int64)
    inv[h] = np.arange(N)
    Ws = W[-1][h]
    lo, hi = inv[idx[-1, 0]], inv[idx[-1, 1]]
    assert np.all(idx[-1, 0::5] == h[lo]) and np.all(idx[-1, 2::5] == h[lo])
    assert np.all(idx[-1, 1::5] == h[hi]) and np.all(idx[-1, 3::5] == h[hi])
    assert N == 2048 and Ws[:lo].max(initial=0.0) <= 2.0 ** -51 and Ws[hi + 1:].max(initial=0.0) <= 2.0 ** -51 and lo < hi
    assert Ws[lo] >= 2.0 ** -51 and Ws[hi] >= 2.0 ** -51


_PROPERTY = {}


def property_run(golden, N=2048, T=8):
    if "pf" not in _PROPERTY:
        pf = _sqmc(kalman.LinearGauss(**sc.LG), golden, "lg_adaptive", N, 47, T=T)
        assert pf._fused and isinstance(pf.hist, pa.collectors.DeviceParticleHistory)
        pf.run()
        _PROPERTY["pf"] = pf
    return _PROPERTY["pf"]


def check_qmc_property(golden, M, geometry=None, seed=20241021):
    """The point of the method: with one Sobol' point set per call and every lookup in Hilbert order the mean of M
    trajectories lies within 1.0 iid standard error sqrt(var_t / M) of the exact smoothing marginal mean of the particle
    approximation at every t.  The reference's own sampler measured on the CPU: worst |z| over steps 0.145 (N = 256,
    T = 12, M = 1024, 6 seeds), 0.22 (M = 512, 8 seeds), 0.13 (N = 2048, T = 8, M = 512, 4 seeds) -- 4x room; an iid
    sampler, or one that ignores the order, fails at most seeds."""
    pf = property_run(golden)
    X, lw, W = host_history(pf)
    T = X.shape[0]
    S = sc.exact_marginals(X, W, sc._lg_px())
    assert np.allclose(S.sum(axis=1), 1.0, atol=1e-12)
    mean = (S * X).sum(axis=1)
    var = (S * X ** 2).sum(axis=1) - mean ** 2
    u = rqmc.sobol_points(M, T, seed)
    paths = pf.hist.backward_sampling_qmc(M, replay={"u": u}, geometry=geometry)
    again = pf.hist.backward_sampling_qmc(M, seed=seed, geometry=geometry)
    assert all(np.array_equal(p, q) for p, q in zip(paths, again))                  # seed -> sobol_points(M, T, seed)
    ref = restate_qmc(X, lw, W, u, sc._lg_px())[0]
    z = np.array([(np.mean(paths[t]) - mean[t]) / np.sqrt(var[t] / M) for t in range(T)])
    zr = np.array([(np.mean(ref[t]) - mean[t]) / np.sqrt(var[t] / M) for t in range(T)])
    for t in range(T):
        print("qmc property t=%d  z device %+.3f  z restated %+.3f" % (t, z[t], zr[t]))
    assert np.all(np.abs(z) <= 1.0), z


def _c_call(pf, M=4, island=0, geometry=0):
    T = max(pf._n, 1)
    u = np.full((max(M, 1), T), 0.5)
    idx = np.empty((T, max(M, 1)), dtype=np.int64)
    return _lib.lib().smc_filter_backward_qmc(pf._f, island, M, geometry, u.ctypes.data_as(_lib.P(_lib.c_dbl)),
                                              idx.ctypes.data_as(_lib.P(_lib.c_i64)), None)


def check_refusals(golden):
    y = sc._y(golden, "lg_adaptive", 6)
    lg = lambda: ssm.Bootstrap(ssm=kalman.LinearGauss(**sc.LG), data=y)
    # not SQMC: the reference's words, from the entry and from the method
    plain, _ = sc.run_of(golden, "toy_4099")
    with pytest.raises(ValueError, match=REF_MSG):
        _lib.check(_c_call(plain))
    with pytest.raises(ValueError, match=REF_MSG):
        plain.hist.backward_sampling_qmc(4)
    # SQMC, but no whole history
    q = _philox(lambda: pa.SMC(fk=lg(), N=2048, qmc=True, seed=3, collect="off"))
    rolling = _philox(lambda: pa.SMC(fk=lg(), N=2048, qmc=True, seed=3, collect="off", store_history=3))
    assert q._fused and rolling._fused
    q.run()
    assert q.hist is None
    with pytest.raises(ValueError, match="whole history"):
        _lib.check(_c_call(q))
    rolling.run()
    assert isinstance(rolling.hist, pa.collectors.DeviceRollingParticleHistory)
    assert not hasattr(rolling.hist, "backward_sampling_qmc") and not hasattr(rolling.hist, "h_orders")
    with pytest.raises(ValueError, match="whole history"):
        _lib.check(_c_call(rolling))
    ok = _philox(lambda: pa.SMC(fk=lg(), N=2048, qmc=True, seed=3, collect="off", store_history=True))
    with pytest.raises(ValueError, match="no step"):
        ok.hist.backward_sampling_qmc(4)
    with pytest.raises(ValueError, match="no step"):
        _lib.check(_c_call(ok))
    ok.run()
    T = ok._n
    with pytest.raises(ValueError, match="null"):
        _lib.check(_lib.lib().smc_filter_backward_qmc(ok._f, 0, 4, 0, None, None, None))
    with pytest.raises(ValueError, match="M must"):
        _lib.check(_c_call(ok, M=0))
    with pytest.raises(ValueError, match="island"):
        _lib.check(_c_call(ok, island=1))
    with pytest.raises(ValueError, match="geometry"):
        _lib.check(_c_call(ok, geometry=3))
    for bad in (lambda: ok.hist.backward_sampling_qmc(0), lambda: ok.hist.backward_sampling_qmc(4, island=1),
                lambda: ok.hist.backward_sampling_qmc(4, island=-1),
                lambda: ok.hist.backward_sampling_qmc(4, replay={"u": np.zeros((T, 4))}),
                lambda: ok.hist.backward_sampling_qmc(4, replay={"u": np.zeros((4, T - 1))}),
                lambda: ok.hist.backward_sampling_qmc(4, replay={"u_last": np.zeros(4)}),
                lambda: ok.hist.backward_sampling_qmc(4, geometry=3),
                lambda: ok.hist.backward_sampling_qmc(4, geometry="wave")):
        with pytest.raises(ValueError):
            bad()
    # the existing samplers keep refusing SQMC filters
    with pytest.raises(ValueError, match="SQMC"):
        ok.hist.backward_sampling_ON2(4)


def check_non_interference(golden, N=2048, T=12, k=5):
    """Sampling after k of T steps: k rows out, and the filter finishes as the uninterrupted run does
    (smoothing_cases.check_non_interference's construction; the two filters share their point-set counter)."""
    y = sc._y(golden, "lg_adaptive", T)
    mk = lambda: _philox(lambda: pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(**sc.LG), data=y), N=N, qmc=True, seed=31,
                                        collect="off", store_history=True))
    c0 = _lib._counter
    a = mk()
    c1 = _lib._counter
    _lib._counter = c0
    b = mk()
    assert _lib._counter == c1 and a._sqmc_key == b._sqmc_key
    assert a._fused and b._fused
    a.step_async(T)
    b.step_async(k)
    before = sc._state(b)
    p1, i1 = b.hist.backward_sampling_qmc(32, seed=5, return_idx=True, geometry=1)
    p2, i2 = b.hist.backward_sampling_qmc(32, seed=5, return_idx=True, geometry=2)
    assert len(p1) == k == len(p2) and i1.shape == (k, 32) and np.array_equal(i1, i2)
    assert all(np.array_equal(p1[t], b.hist.X[t][i1[t]]) for t in range(k))
    assert len(b.hist.h_orders) == k - 1
    after = sc._state(b)
    assert len(before) == len(after) and all(np.array_equal(u, v) for u, v in zip(before, after))
    b.step_async(T - k)
    sa, sb = sc._state(a), sc._state(b)
    assert len(sa) == len(sb) and all(np.array_equal(u, v) for u, v in zip(sa, sb))
    # one executed step: only the last row is drawn
    c = mk()
    c.step_async(1)
    p, i = c.hist.backward_sampling_qmc(8, seed=1, return_idx=True)
    assert i.shape == (1, 8) and np.array_equal(p[0], c.hist.X[0][i[0]])
