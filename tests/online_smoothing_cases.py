"""On-line smoothing collectors on the device (collectors.Online_smooth_naive / Online_smooth_ON2 / Paris,
smc_filter_online_smooth, particles_amd/csrc/smc_online.h): the checks behind tests/test_online_smoothing_gpu.py
(MI355X) and tests/test_online_smoothing_emu.py (emulator build), built on smoothing_cases.py.

  restated    after every step, Phi_t of the device against the recursion restated in NumPy (scipy.stats.norm.logpdf)
              on the device's own Phi_{t-1}, X_{t-1}, lw_{t-1}, X_t, A_t (teacher forcing).
                ON2    |dPhi[n, k]| <= 1e-9 S_n, S_n = sum_m w_m |Phi_{t-1}[m, k] + psi_k|, w the normalised weights,
                       with max |l| < 1e4 asserted: the two sides differ by a few ulp of |l| in the log-density and a
                       few ulp in exp -- a relative weight error below 1e-11 -- while a wrong index, a dropped tile or
                       a wrong normaliser moves Phi by S_n / N >= 2e-4 S_n at these sizes.
                naive  |d| <= 32 2^-53 sum |terms|: the gather is exact, only the polynomial's rounding order differs.
                est    |d| <= 1e-9 sum_n W_n |Phi_t[n, k]| against np.average of the device's own Phi_t.
  paris       replay mode: As row by row against the contract restated by smoothing_reject_cases.restate (a
              difference must be a certified near-tie; a step without one has nprop equal exactly); given As, Phi_t
              with the naive tolerance; Philox mode = replay mode fed with the documented streams.
  slices      the source split of the all-pairs launch changes form at N = 8192 (above: several tiles per slice) and at
              N = 261 888 (above: one slice).  toy_4099 and toy_8700 restate the default geometry on both sides of the
              first; forced slice counts (SMC_ONLINE_SLICES) at N = 1500 give one slice and slices of two tiles; on
              both sides of the second, and at the sizes the measurements use (2^14, 2^16), the default geometry is
              compared on the device with a forced one -- a geometry, not a result.
  pinned      the reference's own collectors on the `history` case (tests/golden/online_smooth_lg.npz).
  behaviour   determinism, pickling mid-run, non-interference, host route against device route, refusals.
"""
import pickle

import numpy as np
import pytest

import particles_amd as pa
import parity_cases as pc
import smoothing_cases as sc
import smoothing_reject_cases as rc
from oracle import smc_oracle as orc
from particles_amd import _lib
from particles_amd import collectors as col
from particles_amd import kalman
from particles_amd import resampling as rs_mod
from particles_amd import state_space_models as ssm

# (xp - x)^2 with x^2 at t = 0; c[i, j] multiplies xp^i x^j
PSI1 = ssm.QuadAddFunc([0.0, 0.0, 1.0], [[0.0, 0.0, 1.0], [0.0, -2.0, 0.0], [1.0, 0.0, 0.0]])
# (x, x^2, xp x), with (x, x^2, 0) at t = 0: the golden file's function
PSI3 = ssm.QuadAddFunc([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]],
                       [[[0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
                        [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
                        [[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]])


def with_psi(model, psi):
    model.add_func = psi
    return model


# the filters of smoothing_cases.CASES (same model, data, N, seed, ESSrmin), built with collectors; T may be cut
SPECS = {
    "toy_4099": (lambda: kalman.LinearGauss(**sc.LG), ssm.Bootstrap, "lg_adaptive", 6, 4099, 17, 0.5, sc._lg_px(), PSI1),
    # just above OS_N_ONE_TILE = 8192: 34 target blocks, 31 slices asked for, 17 slices of 2 tiles used, the last ragged
    "toy_8700": (lambda: kalman.LinearGauss(**sc.LG), ssm.Bootstrap, "lg_adaptive", 2, 8700, 17, 0.5, sc._lg_px(), PSI1),
    "toy_1500": (lambda: kalman.LinearGauss(**sc.LG), ssm.Bootstrap, "lg_adaptive", 6, 1500, 17, 0.5, sc._lg_px(), PSI3),
    "guided_700": (lambda: kalman.LinearGauss(**sc.LG), ssm.GuidedPF, "lg_adaptive", 6, 700, 22, 0.5, sc._lg_px(), PSI1),
    "gordon_1501": (lambda: ssm.Gordon_etal(), ssm.Bootstrap, "gordon_boot", 8, 1501, 18, 0.5, sc._gordon_px(), PSI3),
    "sv_2500": (lambda: ssm.StochVol(), ssm.Bootstrap, "sv_systematic", 6, 2500, 19, 0.95, sc._sv_px(), PSI3),
    "wide_1500": (lambda: kalman.LinearGauss(**rc.WIDE), ssm.Bootstrap, "lg_adaptive", 6, 1500, 25, 0.5, sc._lg_px(), PSI1),
}
GPU_CASES = ["toy_4099", "toy_8700", "guided_700", "gordon_1501", "sv_2500", "history"]
EMU_CASES = ["history", "guided_700", "toy_1500", "gordon_1501"]
EMU_T = {"gordon_1501": 4}


def make(golden, case, collect, psi=None, T=None, **kw):
    mk, fk_cls, data, T0, N, seed, ess, px, psi0 = SPECS[case]
    psi = psi0 if psi is None else psi
    fk = fk_cls(ssm=with_psi(mk(), psi), data=sc._y(golden, data, T or T0))
    return pa.SMC(fk=fk, N=N, seed=seed, ESSrmin=ess, collect=collect, **kw), px, psi


def history_filter(golden, collect, psi=PSI3):
    """sc.history_run's replayed forward pass (the reference's draws: tests/golden/history.npz), with collectors."""
    g = golden("history")
    mk_dev, mk_orc = pc.MODELS["lg_adaptive"]
    N, T = int(g["N"]), int(g["T"])
    y = list(g["y"])
    np.random.seed(int(g["run_seed"]))
    rec = orc.RecordingRNG()
    orc.run_filter(mk_orc(), y, N, "systematic", 0.5, rng=rec)
    z, u = pc.tapes_from_oracle(rec.tape, T, N, "systematic")
    pf = pa.SMC(fk=ssm.Bootstrap(ssm=with_psi(mk_dev(), psi), data=y), N=N, resampling="systematic", ESSrmin=0.5,
                replay=(z, u), collect=collect)
    return pf, sc._lg_px(), psi


def filter_of(golden, case, collect, **kw):
    if case == "history":
        return history_filter(golden, collect)
    return make(golden, case, collect, **kw)


def collectors_of(pf):
    return [c for c in pf.summaries._collectors if isinstance(c, col._OnlineSmoother)]


def as2d(a):
    a = np.asarray(a, dtype=np.float64)
    return a[:, None] if a.ndim == 1 else a


def psi_terms(psi, xp, x):
    """(..., K) sum over the monomials of |c xp^i x^j|."""
    return sum(np.abs(psi.c[:, i, j]) * np.abs((xp ** i) * (x ** j))[..., None] for i in range(3) for j in range(3))


def psi_of(psi, t, xp, x):
    return as2d(psi(t, xp, x)) if np.ndim(x) == 1 else np.asarray(psi(t, xp, x)).reshape(np.shape(x) + (psi.K,))


def restate_on2(psi, px, t, Phi_prev, Xprev, lwprev, X, chunk=512):
    """(Phi_t, S) of the O(N^2) recursion in NumPy, targets in chunks; asserts max |l| < 1e4."""
    N, K = Phi_prev.shape
    out, S = np.empty((N, K)), np.empty((N, K))
    for n0 in range(0, N, chunk):
        xs = X[n0:n0 + chunk]
        l = lwprev[:, None] + sc.logpt(px, t, Xprev[:, None], xs[None, :])             # (sources, targets)
        fin = np.isfinite(l)
        assert np.abs(l[fin]).max() < 1e4
        e = np.where(fin, np.exp(np.where(fin, l, 0.0) - np.where(fin, l, -np.inf).max(axis=0)), 0.0)
        w = e / e.sum(axis=0)
        v = Phi_prev[:, None, :] + psi_of(psi, t, np.broadcast_to(Xprev[:, None], l.shape), np.broadcast_to(xs[None, :], l.shape))
        out[n0:n0 + chunk] = np.einsum("mn,mnk->nk", w, v)
        S[n0:n0 + chunk] = np.einsum("mn,mnk->nk", w, np.abs(v))
    return out, S


def check_gathered(psi, t, Phi_prev, Xprev, X, As, Phi, where):
    """Phi_t = mean over r of Phi_{t-1}[a] + psi(X_{t-1}[a], X_t[n]), a = As[n, r], with the naive tolerance."""
    R = As.shape[1]
    want = np.zeros_like(Phi)
    terms = np.zeros_like(Phi)
    for r in range(R):
        a = As[:, r]
        want += Phi_prev[a] + as2d(psi(t, Xprev[a], X))
        terms += np.abs(Phi_prev[a]) + psi_terms(psi, Xprev[a], X)
    err = np.abs(Phi - want / R)
    tol = 32.0 * 2.0 ** -53 * terms / R
    print("%s t=%d gather: max err %.3e, max err / tol %.3f" % (where, t, err.max(), (err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol), (where, t, err.max())


def check_estimate(est, Phi, W, where, t):
    want = np.average(Phi, axis=0, weights=W)
    tol = 1e-9 * (W[:, None] * np.abs(Phi)).sum(axis=0)
    err = np.abs(np.atleast_1d(est) - want)
    print("%s t=%d est: err %s tol %s" % (where, t, err, tol))
    assert np.all(err <= tol), (where, t, err, tol)


def check_restated(golden, case, emu=False, store_history=False):
    """Check 1: naive and ON2 on one filter, step by step."""
    kw = {"T": EMU_T[case]} if emu and case in EMU_T else {}
    if store_history:
        kw["store_history"] = True
    pf, px, psi = filter_of(golden, case, [col.Online_smooth_naive(), col.Online_smooth_ON2()], **kw)
    assert pf._fused
    naive, on2 = collectors_of(pf)
    prev = None
    flags = []
    for t in range(pf.fk.T):
        next(pf)
        assert naive._route == "device" == on2._route
        X, lw, W = pf.X.copy(), pf.wgts.lw.copy(), pf.W.copy()
        Pn, Po = as2d(naive.Phi), as2d(on2.Phi)
        assert Pn.shape == (pf.N, psi.K) == Po.shape
        if t == 0:
            want = as2d(psi(0, None, X))
            tol = 32.0 * 2.0 ** -53 * sum(np.abs(psi.c0[:, j]) * np.abs(X ** j)[:, None] for j in range(3))
            assert np.all(np.abs(Pn - want) <= tol) and np.array_equal(Pn, Po)
        else:
            A = pf.A
            flags.append(bool(pf.rs_flag))
            assert pf.rs_flag or np.array_equal(A, np.arange(pf.N))
            check_gathered(psi, t, prev["Pn"], prev["X"], X, A[:, None], Pn, case + " naive")
            want, S = restate_on2(psi, px, t, prev["Po"], prev["X"], prev["lw"], X)
            err = np.abs(Po - want)
            print("%s ON2 t=%d: max err / S %.3e" % (case, t, (err / np.maximum(S, 1e-300)).max()))
            assert np.all(err <= 1e-9 * S), (case, t, (err / S).max())
        check_estimate(pf.summaries.online_smooth_naive[-1], Pn, W, case + " naive", t)
        check_estimate(pf.summaries.online_smooth_ON2[-1], Po, W, case + " ON2", t)
        prev = {"Pn": Pn, "Po": Po, "X": X, "lw": lw}
    if case in ("history", "toy_4099"):
        assert any(flags) and not all(flags), flags                 # resampling and non-resampling steps
    shape = (pf.fk.T,) if psi.scalar else (pf.fk.T, psi.K)
    assert np.shape(pf.summaries.online_smooth_naive) == shape == np.shape(pf.summaries.online_smooth_ON2)


# the geometry of the all-pairs launch as a function of N (smc_online.h: os_slices, OS_TARGET_WGS, OS_N_ONE_TILE, OS_N_SLICED)
OS_N_ONE_TILE, OS_N_SLICED = 8192, 261888


def os_geometry(N, forced=None):
    """(slices used, tiles per slice) of k_os_on2 at N, as the host computes them."""
    B = -(-N // 256)
    s = min(forced if forced else -(-1024 // B), B, 1024)
    per = -(-B // s)
    return -(-B // per), per


def _on2_run(golden, monkeypatch, case, T, slices, N=None):
    if slices is None:
        monkeypatch.delenv("SMC_ONLINE_SLICES", raising=False)
    else:
        monkeypatch.setenv("SMC_ONLINE_SLICES", str(slices))
    try:
        if N is None:
            pf, px, psi = make(golden, case, [col.Online_smooth_ON2()], T=T, psi=PSI1)
        else:
            fk = ssm.Bootstrap(ssm=with_psi(kalman.LinearGauss(**sc.LG), PSI1), data=sc._y(golden, "lg_adaptive", T))
            pf = pa.SMC(fk=fk, N=N, seed=17, ESSrmin=0.5, collect=[col.Online_smooth_ON2()])
        pf.run()
    finally:
        monkeypatch.delenv("SMC_ONLINE_SLICES", raising=False)
    assert collectors_of(pf)[0]._route == "device"
    return as2d(collectors_of(pf)[0].Phi), as2d(np.array(pf.summaries.online_smooth_ON2))


def _agree(a, b, T, where):
    """Each geometry is within 1e-9 S_n of the exact recursion per step (check 1).  These runs use PSI1, whose terms are
    squares: Phi_{t-1} + psi >= 0, so S_n = Phi_t[n] <= max Phi.  Two geometries, compounded linearly over the steps as
    in check_pinned: 2e-9 T max |Phi|."""
    scale = np.abs(a[0]).max(axis=0)
    dP, ds = np.abs(a[0] - b[0]).max(axis=0), np.abs(a[1] - b[1]).max(axis=0)
    print("%s: max |dPhi| %s, max |dest| %s, bound %s" % (where, dP, ds, 2e-9 * T * scale))
    assert np.all(dP <= 2e-9 * T * scale) and np.all(ds <= 2e-9 * T * scale), where


def check_slices(golden, monkeypatch, case="toy_1500", T=3):
    """The source split of k_os_on2 is a geometry, not a result.  At N = 1500 (6 tiles): one slice of 6 tiles, the
    default (6 slices of one tile) and 4 asked for (3 slices of 2 tiles: fewer used than asked) agree within the ON2
    tolerance -- and the default is itself the restated recursion (check_restated)."""
    N = SPECS[case][4]
    assert [os_geometry(N, f) for f in (1, None, 4)] == [(1, 6), (6, 1), (3, 2)]
    one, default, four = (_on2_run(golden, monkeypatch, case, T, f) for f in (1, None, 4))
    _agree(default, one, T, "1 slice")
    _agree(default, four, T, "3 slices of 2 tiles")
    assert not np.array_equal(one[0], default[0]) and not np.array_equal(four[0], default[0])   # (the split is real)


def check_geometry_thresholds(golden, monkeypatch, T=2):
    """Both sides of the two thresholds of os_slices, and the sizes the measurements are taken at.  Just above
    OS_N_ONE_TILE the default geometry is restated in NumPy (check_restated, toy_8700; toy_4099 is below it); around
    OS_N_SLICED, where N^2 is out of NumPy's reach, the default geometry is compared on the device with forced ones
    that check_restated and check_slices tie to the recursion: the same code with another slice count."""
    assert os_geometry(OS_N_ONE_TILE) == (32, 1) and os_geometry(OS_N_ONE_TILE + 1) == (17, 2)
    assert os_geometry(4099) == (17, 1) and os_geometry(8700) == (17, 2)
    assert os_geometry(OS_N_SLICED) == (2, 512) and os_geometry(OS_N_SLICED + 1) == (1, 1024)
    assert os_geometry(1 << 14) == (16, 4) and os_geometry(1 << 16) == (4, 64)
    for N, forced in ((1 << 14, 1), (1 << 16, 7), (OS_N_SLICED, 1), (OS_N_SLICED + 1, 3)):
        assert os_geometry(N, forced) != os_geometry(N)
        a = _on2_run(golden, monkeypatch, None, T, None, N=N)
        b = _on2_run(golden, monkeypatch, None, T, forced, N=N)
        _agree(a, b, T, "N=%d default %s against forced %s" % (N, os_geometry(N), os_geometry(N, forced)))
        assert np.all(np.isfinite(a[0])) and not np.array_equal(a[0], b[0])


# ---- Paris

PARIS_SHAPES = {"toy_4099": [(1, 3), (2, 5)], "wide_1500": [(3, 70)]}
# (the emulator runs one workgroup at a time and the exact launch has one per trajectory: fewer steps, and a smaller N
#  below the wave launch)
PARIS_SHAPES_EMU = {"guided_700": [(1, 3, 3), (2, 5, 3)], "wide_1500": [(3, 70, 2)]}
PARIS_TAPE_SEED = {"wide_1500": 31}


def check_paris_indices(golden, case, Nparis, max_trials, T=None):
    N = SPECS[case][4]
    M = N * Nparis
    rng = np.random.default_rng(PARIS_TAPE_SEED.get(case, 14))
    tapes = {}

    def replay(t):
        if t not in tapes:
            tapes[t] = {"u_prop": rng.random((max_trials, M)), "u": rng.random(M),
                        "u_acc": np.maximum(rng.random((max_trials, M)), 2.0 ** -53)}
        return tapes[t]

    pf, px, psi = make(golden, case, [col.Paris(Nparis=Nparis, max_trials=max_trials, replay=replay, return_idx=True)], T=T)
    paris = collectors_of(pf)[0]
    prev, stats = None, []
    for t in range(pf.fk.T):
        next(pf)
        assert paris._route == "device"
        X, lw, W = pf.X.copy(), pf.wgts.lw.copy(), pf.W.copy()
        Phi = as2d(paris.Phi)
        if t > 0:
            As = paris.As
            assert As.shape == (N, Nparis) and As.dtype == np.int64 and As.min() >= 0 and As.max() < N
            stats.append((t, prev, X, As.copy(), Phi, paris.nprop[-1]))
        check_estimate(pf.summaries.paris[-1], Phi, W, case + " paris", t)
        prev = {"Phi": Phi, "X": X, "lw": lw, "W": W}
    assert len(paris.nprop) == pf.fk.T and paris.nprop[0] == 0.0
    # the restatement, from NumPy alone; it must reach what the shape is there for before anything is compared
    restated, firsts = [], []
    for t, pv, X, As, Phi, nprop in stats:
        hist = (np.array([pv["X"], X]), np.array([pv["lw"], pv["lw"]]), np.array([pv["W"], pv["W"]]), None, None)
        idx = np.array([As.ravel(), np.arange(M) // Nparis])
        logC = np.array([pf.fk.upper_bound_trans(t)])
        tp = tapes[t]
        out = rc.restate(hist, lambda _t, xp, t=t: px(t, xp), idx, logC, tp["u_prop"][None], tp["u_acc"][None], tp["u"][None],
                         "%s t=%d" % (case, t))
        restated.append(out)
        firsts.append(out[5].ravel())
    first = np.concatenate(firsts)
    R = rc.R
    reach = [np.sum((first >= 0) & (first < min(R, max_trials))), np.sum((first >= R) & (first < 64 + R)),
             np.sum(first >= 64 + R), np.sum(first < 0)]
    print("reach %s Nparis=%d max_trials=%d: solo %d, first round %d, later rounds %d, exact %d"
          % ((case, Nparis, max_trials) + tuple(reach)))
    assert reach[0] >= 1 and reach[3] >= 1
    assert max_trials <= R or reach[1] >= 1
    assert max_trials <= 64 + R or reach[2] >= 1
    ties = draws = 0
    for (t, pv, X, As, Phi, nprop), (tt, dd, nprops, nexact, clean, resolved) in zip(stats, restated):
        ties, draws = ties + tt, draws + dd
        if clean[0]:
            assert nprop == nprops[0], (case, t, nprop, nprops[0])
        check_gathered(psi, t, pv["Phi"], pv["X"], X, As, Phi, case + " paris")
    pc.log_near_ties("Paris %s Nparis=%d max_trials=%d" % (case, Nparis, max_trials), ties, draws)
    assert ties <= pc.near_tie_allowance(draws)


def check_paris_philox(golden, case="toy_1500", Nparis=2, max_trials=6, seed=20240619, T=4):
    """Philox mode = replay mode fed with the documented streams: trial i of trajectory j at step t from counter
    (j, t - 1, island, 4 | i << 8), the exact draw from (j, t - 1, island, 3)."""
    N = SPECS[case][4]
    M = N * Nparis
    up, ua, u = rc.philox_tapes(seed, T - 1, M, max_trials, 0)
    a, _, _ = make(golden, case, [col.Paris(Nparis=Nparis, max_trials=max_trials, seed=seed, return_idx=True)], T=T)
    b, _, _ = make(golden, case, [col.Paris(Nparis=Nparis, max_trials=max_trials, return_idx=True,
                                            replay=lambda t: {"u_prop": up[t - 1], "u_acc": ua[t - 1], "u": u[t - 1]})], T=T)
    c, _, _ = make(golden, case, [col.Paris(Nparis=Nparis, max_trials=max_trials, seed=seed + 1, return_idx=True)], T=T)
    for pf in (a, b, c):
        pf.run()
    pa_, pb, pc_ = (collectors_of(pf)[0] for pf in (a, b, c))
    print("philox %s: nprop %s" % (case, pa_.nprop))
    assert np.array_equal(pa_.As, pb.As) and np.array_equal(pa_.Phi, pb.Phi) and pa_.nprop == pb.nprop
    assert np.array_equal(a.summaries.paris, b.summaries.paris)
    assert not np.array_equal(pa_.As, pc_.As)
    assert pa_.nprop[1] > M                                          # (some trajectory needed a second trial)


# ---- pinned to the reference

def check_pinned(golden):
    """The replayed forward pass of the `history` case with the collectors gives the reference's own naive and ON2
    estimates at every t: 1e-9 (t + 1) sum_n W_n |Phi_t[n, k]|, the per-step bound compounded linearly."""
    fx = golden("online_smooth_lg")
    g = golden("history")
    pf, px, psi = history_filter(golden, [col.Online_smooth_naive(), col.Online_smooth_ON2()])
    naive, on2 = collectors_of(pf)
    for t in range(pf.fk.T):
        next(pf)
        assert np.array_equal(pf.X, g["hist_X"][t]) and np.array_equal(pf.wgts.lw, g["hist_lw"][t])
        W = pf.W
        for name, c, est in (("naive", naive, pf.summaries.online_smooth_naive[-1]), ("on2", on2, pf.summaries.online_smooth_ON2[-1])):
            tol = 1e-9 * (t + 1) * (W[:, None] * np.abs(c.Phi)).sum(axis=0)
            err = np.abs(est - fx[name][t])
            print("pinned %s t=%2d err %s tol %s" % (name, t, err, tol))
            assert np.all(err <= tol), (name, t, err, tol)
    assert np.all(np.abs(on2.Phi - fx["on2_Phi"]) <= 1e-9 * pf.fk.T * np.abs(fx["on2_Phi"]).max(axis=0))   # (the same bound, per particle)
    return np.array(pf.summaries.online_smooth_ON2[-1])


def check_paris_law(golden, R=16):
    """Paris is pinned in law: over R device seeds, the mean of the final estimates lies within 4 standard errors
    (from those R runs) of the exact O(N^2) value, in each k.  The seeds are fixed: the check is deterministic."""
    fx = golden("online_smooth_lg")
    exact = fx["on2"][-1]
    finals = []
    for r in range(R):
        pf, _, _ = history_filter(golden, [col.Paris(Nparis=2, seed=777000 + r)])
        pf.run()
        finals.append(pf.summaries.paris[-1])
        assert collectors_of(pf)[0]._route == "device"
    finals = np.array(finals)
    se = finals.std(axis=0, ddof=1) / np.sqrt(R)
    z = (finals.mean(axis=0) - exact) / se
    print("paris law: mean %s exact %s z %s (reference's one run: %s)" % (finals.mean(axis=0), exact, z, fx["paris"][-1]))
    assert np.all(np.abs(z) < 4.0), z


# ---- behaviour

def _three(seed=5):
    return [col.Online_smooth_naive(), col.Online_smooth_ON2(), col.Paris(Nparis=2, seed=seed)]


def _outputs(pf):
    s = pf.summaries
    return [np.array(s.online_smooth_naive), np.array(s.online_smooth_ON2), np.array(s.paris)] + \
           [np.array(c.Phi) for c in collectors_of(pf)] + [np.array(collectors_of(pf)[2].nprop)]


def check_deterministic_and_pickle(golden, case="guided_700", k=3):
    a, _, _ = make(golden, case, _three())
    a.run()
    b, _, _ = make(golden, case, _three())
    b.run()
    oa, ob = _outputs(a), _outputs(b)
    assert all(np.array_equal(u, v) for u, v in zip(oa, ob))
    c, _, _ = make(golden, case, _three())
    for _ in range(k):
        next(c)
    d = pickle.loads(pickle.dumps(c))
    assert all(x._route == "device" for x in collectors_of(d))
    d.run()
    od = _outputs(d)
    assert all(np.array_equal(u, v) for u, v in zip(oa, od))
    # a host-route collector pickles too
    e, _, _ = make(golden, case, [col.Online_smooth_naive()], psi=_python_psi1)
    for _ in range(k):
        next(e)
    e2 = pickle.loads(pickle.dumps(e))
    e2.run()
    e.run()
    assert np.array_equal(e.summaries.online_smooth_naive, e2.summaries.online_smooth_naive)


def check_reads_only(golden, case="toy_1500"):
    """With and without the collectors the filter's X, lw, logLt and A are bit-equal at every step."""
    a, _, _ = make(golden, case, _three())
    b, _, _ = make(golden, case, None)
    for t in range(a.fk.T):
        next(a)
        next(b)
        assert np.array_equal(a.X, b.X) and np.array_equal(a.wgts.lw, b.wgts.lw) and a.logLt == b.logLt
        assert t == 0 or np.array_equal(a.A, b.A)
    assert a.summaries.ESSs == b.summaries.ESSs and a.summaries.logLts == b.summaries.logLts


def _python_psi1(t, xp, x):
    return x ** 2 if t == 0 else (xp - x) ** 2


class _UserLG(kalman.LinearGauss):
    """An operator-path model: PY overridden (same law), so the fused loop is not taken."""

    def PY(self, t, xp, x):
        return kalman.LinearGauss.PY(self, t, xp, x)


class _Feed:
    """A stand-in smc object: the particle system of one step, as the host route reads it."""

    class _W:
        pass

    def __init__(self, fk, N):
        self.fk, self.N, self.qmc, self._fused = fk, N, False, False
        self.wgts = _Feed._W()

    def set(self, t, X, lw, W, A):
        self.t, self.X, self.W, self.A = t, X, W, A
        self.wgts.lw = lw


def check_host_route_agrees(golden, case="guided_700"):
    """A Python add_func, an APF filter and an operator-path model take the host route; on the same particles the host
    route agrees with the device route within the tolerances of check 1."""
    pf, px, psi = make(golden, case, [col.Online_smooth_naive(), col.Online_smooth_ON2()])
    naive, on2 = collectors_of(pf)
    fk_py = type(pf.fk)(ssm=with_psi(kalman.LinearGauss(**sc.LG), _python_psi1), data=pf.fk.data)
    feed = _Feed(fk_py, pf.N)
    hn, ho = col.Online_smooth_naive(), col.Online_smooth_ON2()
    for t in range(pf.fk.T):
        next(pf)
        X, lw, W = pf.X.copy(), pf.wgts.lw.copy(), pf.W.copy()
        A = pf.A.copy() if t else None
        feed.set(t, X, lw, W, A)
        if t:                                                        # teacher forcing: the device's Phi_{t-1}
            hn._host["Phi"], ho._host["Phi"] = prev_n, prev_o
        en, eo = hn.fetch(feed), ho.fetch(feed)
        assert hn._route == "host" == ho._route
        Pn, Po = naive.Phi, on2.Phi
        if t:
            terms = np.abs(prev_n[A]) + psi_terms(psi, Xprev[A], X)[:, 0]
            assert np.all(np.abs(hn.Phi - Pn) <= 32.0 * 2.0 ** -53 * terms), t
            _, S = restate_on2(psi, px, t, as2d(prev_o), Xprev, lwprev, X)
            assert np.all(np.abs(ho.Phi - Po) <= 1e-9 * S[:, 0]), (t, np.abs(ho.Phi - Po).max())
        else:
            assert np.allclose(hn.Phi, Pn, rtol=1e-15) and np.allclose(ho.Phi, Po, rtol=1e-15)
        prev_n, prev_o, Xprev, lwprev = Pn.copy(), Po.copy(), X, lw
    # filters that take the host route end to end
    y = sc._y(golden, "lg_adaptive", 4)
    routes = {
        "python add_func": pa.SMC(fk=ssm.Bootstrap(ssm=with_psi(kalman.LinearGauss(**sc.LG), _python_psi1), data=y), N=200,
                                  seed=3, collect=_three()),
        "APF": pa.SMC(fk=ssm.AuxiliaryBootstrap(ssm=with_psi(kalman.LinearGauss(**sc.LG), PSI1), data=y), N=2048, seed=3,
                      collect=[col.Online_smooth_naive()]),
        "operator path": pa.SMC(fk=ssm.Bootstrap(ssm=with_psi(_UserLG(**sc.LG), PSI3), data=y), N=200, seed=3,
                                collect=_three()),
    }
    assert routes["python add_func"]._fused and routes["APF"]._fused and not routes["operator path"]._fused
    for name, q in routes.items():
        np.random.seed(4)
        q.run()
        cs = collectors_of(q)
        assert all(c._route == "host" for c in cs), name
        for c in cs:
            assert len(c.summary) == 4 and np.all(np.isfinite(c.summary)), name
            assert np.allclose(c.summary[-1], np.average(c.Phi, axis=0, weights=q.W), rtol=1e-12), name
    p = collectors_of(routes["python add_func"])[2]
    assert len(p.nprop) == 4 and p.nprop[0] == 0.0 and all(n >= 400 for n in p.nprop[1:])


def _c_call(pf, method=_lib.ONLINE_ON2, K=1, psi=True, n_paris=2, max_trials=3, island=0, est=True, arrays=True):
    import ctypes
    f = PSI1._struct()
    f.K = K
    N = pf.N
    a = [_lib.DeviceArray((N, 8)), _lib.DeviceArray((N,)), _lib.DeviceArray((N,))]
    out = np.empty(8)
    return _lib.lib().smc_filter_online_smooth(
        pf._f, island, method, ctypes.byref(f) if psi else None, a[0].ptr if arrays else None, a[1].ptr, a[2].ptr, n_paris,
        max_trials, 1, 0.0, None, None, None, None, None, out.ctypes.data_as(_lib.P(_lib.c_dbl)) if est else None)


def check_refusals(golden):
    y = sc._y(golden, "lg_adaptive", 6)
    lg = lambda: ssm.Bootstrap(ssm=with_psi(kalman.LinearGauss(**sc.LG), PSI1), data=y)
    ok = pa.SMC(fk=lg(), N=700, seed=3, collect="off")
    with pytest.raises(ValueError, match="no step"):
        _lib.check(_c_call(ok))
    ok.step_async(2)
    _lib.check(_c_call(ok))                                          # (no history needed)
    for kw, msg in (({"psi": False}, "null"), ({"est": False}, "null"), ({"arrays": False}, "null"), ({"K": 0}, "K must"),
                    ({"K": 9}, "K must"), ({"method": 3}, "unknown method"), ({"island": 1}, "island"),
                    ({"method": _lib.ONLINE_PARIS, "n_paris": 0}, "n_paris"),
                    ({"method": _lib.ONLINE_PARIS, "max_trials": 0}, "max_trials")):
        with pytest.raises(ValueError, match=msg):
            _lib.check(_c_call(ok, **kw))
    mode = _lib.RNG_MODE[0]
    rs_mod.set_rng("philox")
    try:
        q = pa.SMC(fk=lg(), N=4096, qmc=True, seed=3, collect=[col.Online_smooth_naive()])
    finally:
        rs_mod.set_rng(mode)
    assert q._fused
    next(q)
    next(q)
    assert collectors_of(q)[0]._route == "host"                      # never refused outright
    with pytest.raises(ValueError, match="SQMC"):
        _lib.check(_c_call(q))
    lev = pa.SMC(fk=ssm.Bootstrap(ssm=with_psi(ssm.StochVolLeverage(phi=-0.5), PSI1), data=sc._y(golden, "svlev_boot", 6)),
                 N=700, seed=3, collect=[col.Online_smooth_naive()])
    next(lev)
    next(lev)
    assert lev._fused and collectors_of(lev)[0]._route == "host"
    with pytest.raises(ValueError, match="SVLEVERAGE"):
        _lib.check(_c_call(lev))
    g = golden("mv4_boot")
    mv = pa.SMC(fk=ssm.Bootstrap(ssm=kalman.MVLinearGauss_Guarniero_etal(alpha=0.4, dx=4), data=list(g["y"])[:4]), N=700,
                seed=3, collect="off")
    mv.step_async(2)
    with pytest.raises(ValueError, match="MVLINGAUSS"):
        _lib.check(_c_call(mv))
    with pytest.raises(NotImplementedError, match="add_func"):
        ssm.StateSpaceModel().add_func(1, 0.0, 0.0)
    with pytest.raises(ValueError):
        ssm.QuadAddFunc(np.zeros((9, 3)), np.zeros((9, 3, 3)))
    with pytest.raises(ValueError):
        col.Paris(Nparis=2, bogus=1)
    # a collector that misses a step says so
    gap = pa.SMC(fk=lg(), N=700, seed=3, collect=[col.Online_smooth_naive()])
    next(gap)
    gap.step_async(1)
    with pytest.raises(RuntimeError, match="every step"):
        next(gap)
