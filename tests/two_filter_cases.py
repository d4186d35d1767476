"""Two-filter smoothing on the device (DeviceParticleHistory.two_filter_smoothing, smc_filter_two_filter,
particles_amd/csrc/smc_twofilter.h): the checks behind tests/test_two_filter_gpu.py (MI355X), tests/test_two_filter_emu.py
(emulator build) and tests/test_two_filter_host.py (NumPy route), built on smoothing_cases.py.

  restated    ON2 at every t of the run against the double sum restated in NumPy (scipy.stats.norm.logpdf, targets in
              chunks) on the device's own downloaded X, lw of both filters:
                |d est_k| <= 1e-9 sum w |phi_k| / sum w, with max |exponent| < 1e4 asserted
              -- online_smoothing_cases.restate_on2's bound and argument: the two sides differ by a few ulp of the
              exponent and of exp, a relative weight error below 1e-11, while a dropped tile moves the value by >= 1e-2
              of that scale at these sizes.
  slices      forced source splits (SMC_TWOFILTER_SLICES) at 1500 x 700: each within the restated bound, no two bit-equal.
  pairs       ON in replay mode: the returned J, I against searchsorted(cumsum(W), u) (a difference must be a certified
              near-tie); given the returned pairs, est within 1e-9 sum Om |phi_k| and ess within 1e-9 relative of NumPy.
  philox      seed mode = replay mode fed with the documented stream, counter (j, t, island, 5).
  pinned      the reference's own two_filter_smoothing on the `history` case (tests/golden/two_filter_lg.npz).
  law         the mean of 16 seeded ON estimates within 4 standard errors of the ON2 value.
  behaviour   determinism, non-interference, pickling, NumPy route against device route, refusals.
"""
import ctypes
import pickle

import numpy as np
import pytest
import scipy.stats

import particles_amd as pa
import online_smoothing_cases as oc
import parity_cases as pc
import smoothing_cases as sc
from oracle import smc_oracle as orc
from particles_amd import _lib
from particles_amd import collectors as col
from particles_amd import kalman
from particles_amd import state_space_models as ssm

PSI1, PSI3 = oc.PSI1, oc.PSI3


def gauss_loggamma(mean, var):
    """The log-density of N(mean, var) as a QuadLogGamma."""
    return ssm.QuadLogGamma(-0.5 * np.log(2.0 * np.pi * var) - 0.5 * mean ** 2 / var, mean / var, -0.5 / var)


LG_GAMMA = gauss_loggamma(0.0, sc.LG["sigmaX"] ** 2 / (1.0 - sc.LG["rho"] ** 2))
SV_GAMMA = gauss_loggamma(-1.02, 0.178 ** 2 / (1.0 - 0.9702 ** 2))
GORDON_GAMMA = gauss_loggamma(0.0, 100.0)

_lg = lambda: kalman.LinearGauss(**sc.LG)
# name -> (model, Feynman-Kac class, data, T, N_f, forward seed, ESSrmin, N_i, transition, phi, loggamma, islands, island)
SPECS = {
    "lg_4099x1500": (_lg, ssm.Bootstrap, "lg_adaptive", 6, 4099, 17, 0.5, 1500, sc._lg_px(), PSI3, LG_GAMMA, 1, 0),
    # 34 source tiles, the last one ragged (8700 = 33 * 256 + 252), against 3 target blocks: 34 one-tile slices to merge
    "lg_8700x700": (_lg, ssm.Bootstrap, "lg_adaptive", 3, 8700, 17, 0.5, 700, sc._lg_px(), PSI1, LG_GAMMA, 1, 0),
    "gordon_1501x1501": (lambda: ssm.Gordon_etal(), ssm.Bootstrap, "gordon_boot", 8, 1501, 18, 0.5, 1501, sc._gordon_px(),
                         PSI3, GORDON_GAMMA, 1, 0),
    "sv_2500x1100": (lambda: ssm.StochVol(), ssm.Bootstrap, "sv_systematic", 6, 2500, 19, 0.95, 1100, sc._sv_px(), PSI3,
                     SV_GAMMA, 1, 0),
    "guided_700x700": (_lg, ssm.GuidedPF, "lg_adaptive", 6, 700, 22, 0.5, 700, sc._lg_px(), PSI1, LG_GAMMA, 1, 0),
    "islands": (_lg, ssm.Bootstrap, "lg_adaptive", 6, 1100, 23, 0.5, 1100, sc._lg_px(), PSI1, LG_GAMMA, 3, 1),
    "lg_1500x700": (_lg, ssm.Bootstrap, "lg_adaptive", 6, 1500, 17, 0.5, 700, sc._lg_px(), PSI3, LG_GAMMA, 1, 0),
}
GPU_CASES = ["lg_4099x1500", "lg_8700x700", "gordon_1501x1501", "sv_2500x1100", "guided_700x700", "islands"]
EMU_CASES = ["history", "guided_700x700", "lg_1500x700", "gordon_1501x1501"]
EMU_T = {"gordon_1501x1501": 4}
INFO_SEED_OFFSET = 100

_RUNS = {}


def pinned_pair(golden):
    """The `history` forward pass (sc.history_run) and the reference's information filter of two_filter_lg.npz, replayed
    from the oracle's draws under np.random.seed(info_seed) on the reversed data: both bit-equal to their fixtures."""
    if "history" not in _RUNS:
        g, fx = golden("history"), golden("two_filter_lg")
        pf = sc.history_run(golden)
        mk_dev, mk_orc = pc.MODELS["lg_adaptive"]
        N, T = int(g["N"]), int(g["T"])
        y = list(g["y"])[::-1]
        np.random.seed(int(fx["info_seed"]))
        rec = orc.RecordingRNG()
        o = orc.run_filter(mk_orc(), y, N, "systematic", 0.5, rng=rec)
        assert o["final_logLt"] == float(fx["info_logLt"])
        z, u = pc.tapes_from_oracle(rec.tape, T, N, "systematic")
        info = pa.SMC(fk=ssm.Bootstrap(ssm=mk_dev(), data=y), N=N, resampling="systematic", ESSrmin=0.5, replay=(z, u),
                      store_history=True)
        info.run()
        for t in range(T):
            assert np.array_equal(info.hist.X[t], fx["hist_X"][t]) and np.array_equal(info.hist.wgts[t].lw, fx["hist_lw"][t])
        _RUNS["history"] = (pf, info)
    return _RUNS["history"]


def make_pair(golden, case, T=None, steps=None):
    """A fresh (forward, information) pair of SPECS[case]: the information filter is the same Feynman-Kac class on the
    reversed data with another seed.  steps: run only that many steps of each."""
    mk, fk_cls, data, T0, Nf, seed, ess, Ni, px, psi, gam, nisl, isl = SPECS[case]
    y = sc._y(golden, data, T or T0)
    kw = {"n_islands": nisl} if nisl > 1 else {}
    pf = pa.SMC(fk=fk_cls(ssm=mk(), data=y), N=Nf, seed=seed, ESSrmin=ess, store_history=True, collect="off", **kw)
    info = pa.SMC(fk=fk_cls(ssm=mk(), data=y[::-1]), N=Ni, seed=seed + INFO_SEED_OFFSET, ESSrmin=ess, store_history=True,
                  collect="off")
    assert pf._fused and info._fused and isinstance(info.hist, col.DeviceParticleHistory)
    for q in (pf, info):
        if steps is None:
            q.run()
        else:
            for _ in range(steps):
                next(q)
    return pf, info


def pair_of(golden, case, emu=False):
    """(forward, info, transition, phi, loggamma, island), run once per case and T."""
    if case == "history":
        return pinned_pair(golden) + (sc._lg_px(), PSI3, LG_GAMMA, 0)
    T = EMU_T.get(case) if emu else None
    if (case, T) not in _RUNS:
        _RUNS[(case, T)] = make_pair(golden, case, T=T)
    s = SPECS[case]
    return _RUNS[(case, T)] + (s[8], s[9], s[10], s[12])


def particles_at(pf, info, t, island=0):
    """(X_t, lw_t, W_t) of the forward filter's island and (X_ti, lw_ti) of the information filter, downloaded."""
    X, lw, W, _, _ = sc.host_history(pf, island)
    Xi, lwi, _, _, _ = sc.host_history(info, 0)
    ti = pf._n - 2 - t
    return X[t], lw[t], W[t], Xi[ti], lwi[ti]


def phi_of(psi, x, xf):
    """(..., K) phi_k(x, xf) = psi_t(xp = x, x = xf)."""
    x, xf = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(xf, dtype=np.float64))
    return np.asarray(psi(1, x, xf)).reshape(x.shape + (psi.K,))


def restate_on2(px, t, X, lw, Xi, lwinfo, psi, chunk=128):
    """(est, scale) of the double sum in NumPy, targets in chunks: scale_k = sum w |phi_k| / sum w.  Asserts
    max |exponent| < 1e4."""
    G, blocks = -np.inf, []
    for m0 in range(0, len(Xi), chunk):
        xs = Xi[m0:m0 + chunk]
        l = lw[:, None] + lwinfo[None, m0:m0 + chunk] + sc.logpt(px, t + 1, X[:, None], xs[None, :])      # (N_f, c)
        fin = np.isfinite(l)
        assert np.abs(l[fin]).max() < 1e4
        l = np.where(fin, l, -np.inf)
        G = max(G, l.max())
        blocks.append((xs, l))
    A, B, S = 0.0, 0.0, 0.0
    for xs, l in blocks:
        e = np.exp(l - G)
        ph = phi_of(psi, X[:, None], xs[None, :])
        A += e.sum()
        B = B + np.einsum("nm,nmk->k", e, ph)
        S = S + np.einsum("nm,nmk->k", e, np.abs(ph))
    return B / A, S / A


def check_on2_value(est, want, scale, where):
    err = np.abs(np.atleast_1d(est) - want)
    print("%s: err / scale %s" % (where, err / np.maximum(scale, 1e-300)))
    assert np.all(err <= 1e-9 * scale), (where, err, scale)


def check_restated(golden, case, emu=False):
    pf, info, px, psi, gam, isl = pair_of(golden, case, emu)
    assert pf._n >= 3 and info._n == pf._n
    for t in range(pf._n - 1):
        est = pf.hist.two_filter_smoothing(t, info, psi, gam, island=isl)
        assert pf.hist._two_filter_route == "device"
        assert np.shape(est) == (() if psi.scalar else (psi.K,))
        X, lw, _, Xi, lwi = particles_at(pf, info, t, isl)
        want, scale = restate_on2(px, t, X, lw, Xi, lwi - gam(Xi), psi)
        check_on2_value(est, want, scale, "%s ON2 t=%d" % (case, t))


# the geometry of the all-pairs launch (smc_twofilter.h: tf_slices): (slices used, tiles per slice)
def tf_geometry(Ni, Nf, forced=None):
    B, tiles = -(-Ni // 256), -(-Nf // 256)
    s = min(forced if forced else -(-1024 // B), tiles, 1024)
    per = -(-tiles // s)
    return -(-tiles // per), per


def check_slices(golden, monkeypatch, case="lg_1500x700"):
    """The source split is a geometry, not a result: one slice of six tiles, the default (six one-tile slices) and three
    slices of two tiles are each within the restated bound at every t, and no two give the same bits (the split is real)."""
    pf, info, px, psi, gam, isl = pair_of(golden, case)
    Nf, Ni = pf.N, info.N
    assert [tf_geometry(Ni, Nf, f) for f in (1, None, 3)] == [(1, 6), (6, 1), (3, 2)]
    assert tf_geometry(1500, 4099) == (17, 1) and tf_geometry(700, 8700) == (34, 1) and tf_geometry(1 << 14, 1 << 14) == (16, 4)
    ts = range(pf._n - 1)
    want = [restate_on2(px, t, *(lambda X, lw, _, Xi, lwi: (X, lw, Xi, lwi - gam(Xi)))(*particles_at(pf, info, t, isl)), psi)
            for t in ts]
    out = []
    for forced in (1, None, 3):
        if forced is None:
            monkeypatch.delenv("SMC_TWOFILTER_SLICES", raising=False)
        else:
            monkeypatch.setenv("SMC_TWOFILTER_SLICES", str(forced))
        try:
            out.append(np.array([pf.hist.two_filter_smoothing(t, info, psi, gam) for t in ts]))
        finally:
            monkeypatch.delenv("SMC_TWOFILTER_SLICES", raising=False)
        for t in ts:
            check_on2_value(out[-1][t], want[t][0], want[t][1], "%s slices=%s t=%d" % (case, forced, t))
    # (the estimates of every t of the run, as one array per geometry)
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2]) and not np.array_equal(out[0], out[2])


# ---- ON: the pairs

def modif_arrays(pf, info, t, island=0):
    """smoothing_worker's 'two-filter_ON_prop' recipe (smoothing.py:651-661)."""
    X = sc.host_history(pf, island)[0]
    Xi = sc.host_history(info, 0)[0]
    ti = pf._n - 2 - t
    mf = scipy.stats.norm.logpdf(X[t], loc=np.mean(Xi[ti + 1]), scale=np.std(Xi[ti + 1]))
    mi = scipy.stats.norm.logpdf(Xi[ti], loc=np.mean(X[t + 1]), scale=np.std(X[t + 1]))
    return mf, mi


def _audit_draws(W, u, got, where):
    cs = np.cumsum(W)
    want = sc._search(cs, u, W)
    assert np.all(W[got] > 0.0), (where, "a zero-weight particle was drawn")
    ties = 0
    for j in np.flatnonzero(got != want):
        assert sc._certified_index(cs, u[j], int(got[j]), int(want[j])), (where, j, got[j], want[j], u[j])
        ties += 1
    return ties


def check_on_given_pairs(px, psi, t, X, Xi, J, I, mf, mi, est, ess, where):
    """est and ess of the O(N) form in NumPy on the given pairs."""
    lo = sc.logpt(px, t + 1, X[J], Xi[I])
    if mf is not None:
        lo = lo - mf[J] - mi[I]
    Om = orc.exp_and_normalise(lo)
    ph = phi_of(psi, X[J], Xi[I])
    want = (Om[:, None] * ph).sum(axis=0)
    tol = 1e-9 * (Om[:, None] * np.abs(ph)).sum(axis=0)
    err = np.abs(np.atleast_1d(est) - want)
    want_ess = 1.0 / np.sum(Om ** 2)
    print("%s: est err %s tol %s; ess %.6f (NumPy %.6f)" % (where, err, tol, ess, want_ess))
    assert np.all(err <= tol), (where, err, tol)
    assert abs(ess - want_ess) <= 1e-9 * want_ess, (where, ess, want_ess)


def check_pairs(golden, case, P=None, emu=False):
    """Replay mode, with and without the modif_* arrays, at every t."""
    pf, info, px, psi, gam, isl = pair_of(golden, case, emu)
    Nf, Ni = pf.N, info.N
    P = Nf if P is None else P
    rng = np.random.default_rng(14)
    ties = 0
    for t in range(pf._n - 1):
        X, lw, W, Xi, lwi = particles_at(pf, info, t, isl)
        u_f, u_i = rng.random(P), rng.random(P)
        for mf, mi in ((None, None), modif_arrays(pf, info, t, isl)):
            est, ess, J, I = pf.hist.two_filter_smoothing(t, info, psi, gam, linear_cost=True, return_ess=True, modif_forward=mf,
                                                          modif_info=mi, npairs=P, replay={"u_fwd": u_f, "u_info": u_i},
                                                          return_idx=True, island=isl)
            assert pf.hist._two_filter_route == "device"
            assert J.shape == (P,) == I.shape and J.dtype == np.int64 == I.dtype
            assert J.min() >= 0 and J.max() < Nf and I.min() >= 0 and I.max() < Ni
            where = "%s ON t=%d P=%d %s" % (case, t, P, "plain" if mf is None else "prop")
            ties += _audit_draws(W if mf is None else orc.exp_and_normalise(lw + mf), u_f, J, where + " J")
            linfo = lwi - gam(Xi)
            ties += _audit_draws(orc.exp_and_normalise(linfo if mi is None else linfo + mi), u_i, I, where + " I")
            check_on_given_pairs(px, psi, t, X, Xi, J, I, mf, mi, est, ess, where)
    draws = 2 * 2 * P * (pf._n - 1)
    pc.log_near_ties("two-filter ON %s P=%d" % (case, P), ties, draws)
    assert ties <= pc.near_tie_allowance(2 * P)


def philox_tapes(seed, t, P, island):
    """The documented stream: counter (j, t, island, 5), word x01 -> u_fwd, word x23 -> u_info, both [0, 1)."""
    x01, x23 = orc.philox_u64_pair(seed, np.arange(P, dtype=np.uint32), t, island, 5)
    return orc.u01_halfopen(x01), orc.u01_halfopen(x23)


def check_philox(golden, case="lg_1500x700", seed=20240705, P=777):
    pf, info, px, psi, gam, isl = pair_of(golden, case)
    for t in (0, pf._n - 2):
        kw = dict(linear_cost=True, return_ess=True, npairs=P, return_idx=True, island=isl)
        a = pf.hist.two_filter_smoothing(t, info, psi, gam, seed=seed, **kw)
        u_f, u_i = philox_tapes(seed, t, P, isl)
        b = pf.hist.two_filter_smoothing(t, info, psi, gam, replay={"u_fwd": u_f, "u_info": u_i}, **kw)
        c = pf.hist.two_filter_smoothing(t, info, psi, gam, seed=seed + 1, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), t
        assert not np.array_equal(a[2], c[2]) and not np.array_equal(a[3], c[3])
        assert len(np.unique(a[2])) > 10 and len(np.unique(a[3])) > 10


# ---- pinned to the reference

def check_pinned(golden):
    pf, info = pinned_pair(golden)
    fx = golden("two_filter_lg")
    px, gam = sc._lg_px(), ssm.QuadLogGamma(*fx["loggamma3"])
    T = pf._n
    assert fx["on2"].shape == (T - 1, 3)
    for t in range(T - 1):
        est = pf.hist.two_filter_smoothing(t, info, PSI3, gam)
        X, lw, _, Xi, lwi = particles_at(pf, info, t)
        _, scale = restate_on2(px, t, X, lw, Xi, lwi - gam(Xi), PSI3)
        check_on2_value(est, fx["on2"][t], scale, "pinned ON2 t=%d" % t)
    for t in (int(v) for v in fx["on_times"]):
        X, lw, _, Xi, lwi = particles_at(pf, info, t)
        for tag, mf, mi in (("plain", None, None), ("prop", fx["modif_forward_%d" % t], fx["modif_info_%d" % t])):
            J, I = fx["on_%s_J_%d" % (tag, t)], fx["on_%s_I_%d" % (tag, t)]
            est, ess = pf.hist.two_filter_smoothing(t, info, PSI3, gam, linear_cost=True, return_ess=True, modif_forward=mf,
                                                    modif_info=mi, replay={"idx_fwd": J, "idx_info": I})
            Om = orc.exp_and_normalise(sc.logpt(px, t + 1, X[J], Xi[I]) - (0.0 if mf is None else mf[J] + mi[I]))
            tol = 1e-9 * (Om[:, None] * np.abs(phi_of(PSI3, X[J], Xi[I]))).sum(axis=0)
            err = np.abs(est - fx["on_%s_est_%d" % (tag, t)])
            want_ess = float(fx["on_%s_ess_%d" % (tag, t)])
            print("pinned ON %s t=%d: err %s tol %s ess %.6f (%.6f)" % (tag, t, err, tol, ess, want_ess))
            assert np.all(err <= tol), (tag, t, err, tol)
            assert abs(ess - want_ess) <= 1e-9 * want_ess


def check_law(golden, R=16, P=4096):
    """Over R fixed device seeds the mean ON estimate lies within 4 standard errors (from those R runs) of the device's ON2
    value, for each k, at five t.  The check is deterministic."""
    pf, info = pinned_pair(golden)
    for t in (0, 7, 14, 21, 28):
        exact = pf.hist.two_filter_smoothing(t, info, PSI3, LG_GAMMA)
        runs = np.array([pf.hist.two_filter_smoothing(t, info, PSI3, LG_GAMMA, linear_cost=True, npairs=P, seed=880000 + r)
                         for r in range(R)])
        se = runs.std(axis=0, ddof=1) / np.sqrt(R)
        z = (runs.mean(axis=0) - exact) / se
        print("law t=%d: mean %s exact %s z %s" % (t, runs.mean(axis=0), exact, z))
        assert np.all(np.abs(z) < 4.0), (t, z)


# ---- behaviour

def _state(q):
    return [q.X.copy(), q.wgts.lw.copy(), q.logLt] + ([q.A.copy()] if q.t > 0 and q.A is not None else [])


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def _both(pf, info, psi, gam, t, seed=5):
    return (pf.hist.two_filter_smoothing(t, info, psi, gam),
            pf.hist.two_filter_smoothing(t, info, psi, gam, linear_cost=True, return_ess=True, seed=seed, return_idx=True))


def _flat(res):
    return [np.asarray(res[0])] + [np.asarray(v) for v in res[1]]


def check_behaviour(golden, case="guided_700x700", k=4):
    """Twice the same bits; the filters are left as they were and go on stepping; a pickled pair gives the same."""
    psi, gam = SPECS[case][9], SPECS[case][10]
    pf, info = make_pair(golden, case, steps=k)
    before = _state(pf), _state(info)
    a = _both(pf, info, psi, gam, 1)
    b = _both(pf, info, psi, gam, 1)
    assert _same(_flat(a), _flat(b))
    assert _same(before[0], _state(pf)) and _same(before[1], _state(info))
    for t in range(k):
        assert np.array_equal(pf.hist.X[t], sc.host_history(pf)[0][t])
    p2, i2 = pickle.loads(pickle.dumps((pf, info)))
    c = _both(p2, i2, psi, gam, 1)
    assert p2.hist._two_filter_route == "device" and _same(_flat(a), _flat(c))
    # both go on stepping, to what an undisturbed pair reaches
    ref_f, ref_i = make_pair(golden, case)
    pf.run()
    info.run()
    assert _same(_state(pf), _state(ref_f)) and _same(_state(info), _state(ref_i))
    assert np.array_equal(_both(pf, info, psi, gam, 3)[0], _both(ref_f, ref_i, psi, gam, 3)[0])


class _Stand:
    """A stand-in SMC object for a history kept on the host."""

    def __init__(self, hist, N):
        self.hist, self.N, self.qmc = hist, N, False


def _host_history(q, island=0):
    X, lw, W, _, _ = sc.host_history(q, island)
    h = col.ParticleHistory(q.fk, False)
    for t in range(q._n):
        w = col._Frozen()
        w.lw, w.W = lw[t], W[t]
        h.X.append(X[t])
        h.wgts.append(w)
        h.A.append(None)
    return h


def check_numpy_route(golden, case="lg_1500x700", emu=False):
    """The NumPy route on the same particles: a lambda phi, a lambda loggamma and a host ParticleHistory are each within
    the restated bound of the NumPy restatement (as the device route is: check_restated), and within twice that bound
    of the device's value; given pairs give the O(N) form within its bound."""
    pf, info, px, psi, gam, isl = pair_of(golden, case, emu)
    t = 1
    dev = pf.hist.two_filter_smoothing(t, info, psi, gam)
    X, lw, _, Xi, lwi = particles_at(pf, info, t)
    want, scale = restate_on2(px, t, X, lw, Xi, lwi - gam(Xi), psi)
    lam_phi = lambda x, xf: psi(1, x, xf)
    lam_gam = lambda x: gam(x)
    hf, hi = _host_history(pf), _Stand(_host_history(info), info.N)
    routes = {
        "lambda phi": lambda **kw: pf.hist.two_filter_smoothing(t, info, lam_phi, gam, **kw),
        "lambda loggamma": lambda **kw: pf.hist.two_filter_smoothing(t, info, psi, lam_gam, **kw),
        "host info history": lambda **kw: pf.hist.two_filter_smoothing(t, hi, psi, gam, **kw),
        "host ParticleHistory": lambda **kw: hf.two_filter_smoothing(t, hi, psi, gam, **kw),
    }
    rng = np.random.default_rng(3)
    J, I = rng.integers(0, pf.N, 500), rng.integers(0, info.N, 500)
    for name, call in routes.items():
        est = call()
        if name != "host ParticleHistory":
            assert pf.hist._two_filter_route == "host", name
        check_on2_value(est, want, scale, "NumPy route (%s)" % name)
        assert np.all(np.abs(est - dev) <= 2e-9 * scale), name
        e, s = call(linear_cost=True, return_ess=True, npairs=500, replay={"idx_fwd": J, "idx_info": I})
        check_on_given_pairs(px, psi, t, X, Xi, J, I, None, None, e, s, "NumPy route ON (%s)" % name)
        e, s, J2, I2 = call(linear_cost=True, return_ess=True, seed=11, npairs=300, return_idx=True)
        assert J2.shape == (300,) and np.all(sc.host_history(pf)[2][t][J2] > 0.0)
        check_on_given_pairs(px, psi, t, X, Xi, J2, I2, None, None, e, s, "NumPy route ON draws (%s)" % name)
    with pytest.raises(ValueError, match="unknown replay"):
        routes["lambda phi"](linear_cost=True, replay={"bogus": J})
    with pytest.raises(ValueError, match="shape"):
        routes["lambda phi"](linear_cost=True, replay={"idx_fwd": J[:5], "idx_info": I[:5]})


def check_operator_path_filters(golden):
    """Operator-path filters keep their history on the host: ``ParticleHistory.two_filter_smoothing`` is the NumPy route,
    checked against the restatement on those filters' own particles; no upper_bound_log_pt is needed."""
    y = sc._y(golden, "lg_adaptive", 5)
    np.random.seed(4)
    pf = pa.SMC(fk=ssm.Bootstrap(ssm=oc._UserLG(**sc.LG), data=y), N=200, seed=3, store_history=True)
    info = pa.SMC(fk=ssm.Bootstrap(ssm=oc._UserLG(**sc.LG), data=y[::-1]), N=150, seed=4, store_history=True)
    pf.run()
    info.run()
    assert not pf._fused and isinstance(pf.hist, col.ParticleHistory) and isinstance(info.hist, col.ParticleHistory)
    px = sc._lg_px()
    for t in range(4):
        ti = 3 - t
        X, lw = np.asarray(pf.hist.X[t]), np.asarray(pf.hist.wgts[t].lw)
        Xi, lwi = np.asarray(info.hist.X[ti]), np.asarray(info.hist.wgts[ti].lw)
        want, scale = restate_on2(px, t, X, lw, Xi, lwi - LG_GAMMA(Xi), PSI3)
        for phi, gam in ((PSI3, LG_GAMMA), (lambda x, xf: PSI3(1, x, xf), lambda x: LG_GAMMA(x))):
            check_on2_value(pf.hist.two_filter_smoothing(t, info, phi, gam), want, scale, "operator path t=%d" % t)
        est = pf.hist.two_filter_smoothing(t, info, lambda x, xf: (x - xf) ** 2, LG_GAMMA, linear_cost=True, seed=2)
        assert np.ndim(est) == 0 and np.isfinite(est)
    with pytest.raises(ValueError, match="two-filter smoothing: t must be in range 0,...,T-2"):
        pf.hist.two_filter_smoothing(4, info, PSI3, LG_GAMMA)
    with pytest.raises(ValueError, match="two-filter smoothing: t must be in range 0,...,T-2"):
        pf.hist.two_filter_smoothing(-1, info, PSI3, LG_GAMMA)
    g = ssm.QuadLogGamma(0.5, -1.0, 2.0)
    assert np.array_equal(g._coef(), [0.5, -1.0, 2.0]) and np.allclose(g(np.array([0.0, 2.0])), [0.5, 6.5])


def _c_call(pf, info, t=0, method=_lib.TWOFILTER_ON2, K=1, island=0, island_info=0, npairs=8, phi=True, gamma=True, est=True,
            idx=None, f=True, g=True):
    s = PSI1._struct()
    s.K = K
    g3, out = np.zeros(3), np.empty(8)
    P = _lib.P
    ix = None if idx is None else [np.ascontiguousarray(a, dtype=np.int64) for a in idx]
    return _lib.lib().smc_filter_two_filter(
        pf._f if f else None, island, info._f if g else None, island_info, t, method, ctypes.byref(s) if phi else None,
        g3.ctypes.data_as(P(_lib.c_dbl)) if gamma else None, None, None, npairs, 1, None, None,
        ix[0].ctypes.data_as(P(_lib.c_i64)) if ix else None, ix[1].ctypes.data_as(P(_lib.c_i64)) if ix else None, None, None,
        out.ctypes.data_as(P(_lib.c_dbl)) if est else None, None)


def check_refusals(golden, monkeypatch):
    y = sc._y(golden, "lg_adaptive", 6)
    lg = lambda **kw: pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(**sc.LG), data=y), N=700, seed=3, collect="off", **kw)
    pf, info = lg(store_history=True), lg(store_history=True)
    pf.step_async(4)
    info.step_async(2)
    ON = _lib.TWOFILTER_ON
    _lib.check(_c_call(pf, info, t=1))                              # ti = 1: the last step info has run
    for kw, msg in (({"f": False}, "null"), ({"g": False}, "null"), ({"phi": False}, "null"), ({"gamma": False}, "null"),
                    ({"est": False}, "null"), ({"t": -1}, "t must be in range"), ({"t": 3}, "t must be in range"),
                    ({"t": 0}, "information filter has not run"), ({"island": 1, "t": 1}, "island out of range"),
                    ({"island_info": 1, "t": 1}, "island_info out of range"), ({"K": 0, "t": 1}, "K must"),
                    ({"K": 9, "t": 1}, "K must"), ({"method": 2, "t": 1}, "unknown method"),
                    ({"method": ON, "npairs": 0, "t": 1}, "npairs"),
                    ({"method": ON, "t": 1, "idx": (np.full(8, 700), np.zeros(8))}, "index out of range"),
                    ({"method": ON, "t": 1, "idx": (np.zeros(8), np.full(8, -1))}, "index out of range")):
        with pytest.raises(ValueError, match=msg):
            _lib.check(_c_call(pf, info, **kw))
    nohist = lg()
    nohist.step_async(4)
    with pytest.raises(ValueError, match="whole history"):
        _lib.check(_c_call(nohist, info, t=1))
    with pytest.raises(ValueError, match="information filter was created without a whole history"):
        _lib.check(_c_call(pf, nohist, t=1))
    lev = pa.SMC(fk=ssm.Bootstrap(ssm=ssm.StochVolLeverage(phi=-0.5), data=sc._y(golden, "svlev_boot", 6)), N=700, seed=3,
                 store_history=True, collect="off")
    lev.step_async(4)
    with pytest.raises(ValueError, match="SVLEVERAGE"):
        _lib.check(_c_call(lev, info, t=1))
    _lib.check(_c_call(pf, lev, t=1))                               # (only X and lw of the information filter are read)
    g = golden("mv4_boot")
    mv = pa.SMC(fk=ssm.Bootstrap(ssm=kalman.MVLinearGauss_Guarniero_etal(alpha=0.4, dx=4), data=list(g["y"])[:4]), N=700,
                seed=3, store_history=True, collect="off")
    mv.step_async(4)
    with pytest.raises(ValueError, match="MVLINGAUSS"):
        _lib.check(_c_call(mv, info, t=1))
    with pytest.raises(ValueError, match="must be univariate"):
        _lib.check(_c_call(pf, mv, t=1))
    # another context: one stream could not order the call
    other = _lib.Context(_lib.ctx().device, seed=1)
    monkeypatch.setattr(_lib, "_default_ctx", other)
    far = lg(store_history=True)
    monkeypatch.undo()
    far.step_async(4)
    with pytest.raises(ValueError, match="the two filters must share a context"):
        _lib.check(_c_call(pf, far, t=1))
    # the Python method: the reference's message, the replay dict
    with pytest.raises(ValueError, match="two-filter smoothing: t must be in range 0,...,T-2"):
        pf.hist.two_filter_smoothing(3, info, PSI1, LG_GAMMA)
    with pytest.raises(ValueError, match="unknown replay"):
        pf.hist.two_filter_smoothing(1, info, PSI1, LG_GAMMA, linear_cost=True, replay={"u": np.zeros(700)})
    with pytest.raises(ValueError, match="shape"):
        pf.hist.two_filter_smoothing(1, info, PSI1, LG_GAMMA, linear_cost=True, replay={"u_fwd": np.zeros(5)})
    with pytest.raises(ValueError, match="modif_forward has shape"):
        pf.hist.two_filter_smoothing(1, info, PSI1, LG_GAMMA, linear_cost=True, modif_forward=np.zeros(5))
    # modif_* are silently unused without linear_cost, as in the reference
    a = pf.hist.two_filter_smoothing(1, info, PSI1, LG_GAMMA)
    assert a == pf.hist.two_filter_smoothing(1, info, PSI1, LG_GAMMA, modif_forward=np.ones(700), modif_info=np.ones(700))
    far.__del__()                                                   # (the filter goes before its context: an SMC object sits in
    other.close()                                                   #  a reference cycle with its history, `del` would not free it)


def check_sqmc_takes_the_numpy_route(golden):
    from particles_amd import resampling as rs_mod
    y = sc._y(golden, "lg_adaptive", 4)
    mode = _lib.RNG_MODE[0]
    rs_mod.set_rng("philox")
    try:
        q = pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(**sc.LG), data=y), N=4096, qmc=True, seed=3, store_history=True,
                   collect="off")
        q.run()
    finally:
        rs_mod.set_rng(mode)
    info = pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(**sc.LG), data=y[::-1]), N=300, seed=5, store_history=True,
                  collect="off")
    info.run()
    est = q.hist.two_filter_smoothing(1, info, PSI1, LG_GAMMA)       # never refused outright
    assert np.isfinite(est)
    assert q._fused and isinstance(q.hist, col.DeviceParticleHistory) and q.hist._two_filter_route == "host"
    assert np.isfinite(info.hist.two_filter_smoothing(1, q, PSI1, LG_GAMMA)) and info.hist._two_filter_route == "host"
    with pytest.raises(ValueError, match="SQMC"):
        _lib.check(_c_call(q, info, t=1))
    with pytest.raises(ValueError, match="SQMC information"):
        _lib.check(_c_call(info, q, t=1))
