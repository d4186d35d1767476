"""Backward sampling over a device-resident history (DeviceParticleHistory.backward_sampling_ON2 / _mcmc) against
the host route a user had before: download the history with smc_filter_history and run the reference's NumPy
expression (particles/smoothing.py:291-350) on it.

    python tools/ffbs_perf.py [--quick]            (on a GPU box; the output is profiles/ffbs_perf.txt)
    python tools/ffbs_perf.py --reject [--quick]   (backward_sampling_reject; profiles/ffbs_reject_perf.txt)

Device calls are timed with HIP events around the whole call (history resident, Philox draws, the (T, M) indices and
paths downloaded at its end), after a warm-up call, median of 5.  The host route is timed once with perf_counter; the
exact sampler's host loop is timed on 8 of the trajectories and scaled to M (it is a loop over trajectories).
"""
import ctypes
import os
import sys
import time

import numpy as np
import scipy.stats

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import particles_amd as pa
from particles_amd import _lib, kalman
from particles_amd import state_space_models as ssm

RHO, SX, SY = 0.9, 1.0, 1.5
_hip = ctypes.CDLL("libamdhip64.so")


class Events:
    def __init__(self):
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            assert _hip.hipEventCreate(ctypes.byref(e)) == 0

    def time(self, fn):
        assert _hip.hipEventRecord(self.a, None) == 0
        out = fn()
        assert _hip.hipEventRecord(self.b, None) == 0 and _hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert _hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return ms.value, out


def make_filter(N, T):
    rng = np.random.RandomState(42)
    x = np.cumsum(rng.standard_normal(T)) * 0.3
    y = [np.atleast_1d(v) for v in x + SY * rng.standard_normal(T)]
    pf = pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(rho=RHO, sigmaX=SX, sigmaY=SY), data=y), N=N, seed=7,
                ESSrmin=0.5, store_history=True, collect="off")
    pf.run()
    return pf


def device(ev, call, reps=5):
    call(0)                                        # warm-up: code objects, the pool's blocks
    return float(np.median([ev.time(lambda: call(1 + r))[0] for r in range(reps)]))


def logpt(xp, x):
    return scipy.stats.norm.logpdf(x, loc=RHO * xp, scale=SX)


def host_on2(pf, M, M_timed):
    T = pf._n
    t0 = time.perf_counter()
    X = [pf._history(_lib.FIELD_X, t) for t in range(T)]
    lw = [pf._history(_lib.FIELD_LW, t) for t in range(T)]
    W = pf._history(_lib.FIELD_W, T - 1)
    t_down = time.perf_counter() - t0
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    idx = np.empty((T, M_timed), dtype=np.int64)
    idx[-1] = np.searchsorted(np.cumsum(W), rng.random(M_timed))
    for m in range(M_timed):
        for t in reversed(range(T - 1)):
            lwm = lw[t] + logpt(X[t], X[t + 1][idx[t + 1, m]])
            w = np.exp(lwm - lwm.max())
            idx[t, m] = min(np.searchsorted(np.cumsum(w / w.sum()), rng.random()), pf.N - 1)
    t_loop = (time.perf_counter() - t0) * M / M_timed
    return 1e3 * t_down, 1e3 * t_loop


def host_mcmc(pf, M, nsteps):
    T, N = pf._n, pf.N
    t0 = time.perf_counter()
    X = [pf._history(_lib.FIELD_X, t) for t in range(T)]
    W = [pf._history(_lib.FIELD_W, t) for t in range(T)]
    A = [pf._history(_lib.FIELD_A, t) if t else None for t in range(T)]
    t_down = time.perf_counter() - t0
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    idx = np.empty((T, M), dtype=np.int64)
    idx[-1] = np.minimum(np.searchsorted(np.cumsum(W[-1]), rng.random(M)), N - 1)
    for t in reversed(range(T - 1)):
        xn = X[t + 1][idx[t + 1]]
        idx[t] = A[t + 1][idx[t + 1]]
        cs = np.cumsum(W[t])
        for i in range(nsteps):
            prop = np.minimum(np.searchsorted(cs, rng.random(M)), N - 1)
            lpr = logpt(X[t][prop], xn) - logpt(X[t][idx[t]], xn)
            idx[t] = np.where(np.log(rng.random(M)) < lpr, prop, idx[t])
    return 1e3 * t_down, 1e3 * (time.perf_counter() - t0)


def host_reject(pf, M, max_trials):
    """The hybrid (smoothing.py:352-423) restated in NumPy on the downloaded history: rounds of trials over the
    trajectories still open, then the exact draw for the rest (timed on at most 8 of them, scaled)."""
    T, N = pf._n, pf.N
    t0 = time.perf_counter()
    X = [pf._history(_lib.FIELD_X, t) for t in range(T)]
    lw = [pf._history(_lib.FIELD_LW, t) for t in range(T)]
    W = [pf._history(_lib.FIELD_W, t) for t in range(T)]
    t_down = time.perf_counter() - t0
    logC = pf.fk.upper_bound_trans(1)
    rng = np.random.default_rng(1)
    t_exact = 0.0
    t0 = time.perf_counter()
    idx = np.empty((T, M), dtype=np.int64)
    idx[-1] = np.minimum(np.searchsorted(np.cumsum(W[-1]), rng.random(M)), N - 1)
    for t in reversed(range(T - 1)):
        cs = np.cumsum(W[t])
        open_ = np.arange(M)
        xn = X[t + 1][idx[t + 1]]
        trials = 0
        while len(open_) and trials < max_trials:
            trials += 1
            prop = np.minimum(np.searchsorted(cs, rng.random(len(open_))), N - 1)
            acc = np.log(rng.random(len(open_))) < logpt(X[t][prop], xn[open_]) - logC
            idx[t, open_[acc]] = prop[acc]
            open_ = open_[~acc]
        timed = open_[:8]
        t1 = time.perf_counter()
        for m in timed:
            lwm = lw[t] + logpt(X[t], xn[m])
            w = np.exp(lwm - lwm.max())
            idx[t, m] = min(np.searchsorted(np.cumsum(w / w.sum()), rng.random()), N - 1)
        if len(timed):
            t_exact += (time.perf_counter() - t1) * (len(open_) / len(timed) - 1.0)
            idx[t, open_[8:]] = idx[t, timed[0]]                     # (placeholders: the loop is timed, not its law)
    return 1e3 * t_down, 1e3 * (time.perf_counter() - t0 + t_exact)


def reject_legs(quick):
    """Rejection legs (profiles/ffbs_reject_perf.txt): the hybrid at max_trials = M and 8 against the MCMC sampler, the
    exact sampler and the host route on the same history; then the same on a low-acceptance history, with and without
    the wave-cooperative launch (SMC_REJECT_SOLO_TRIALS >= max_trials leaves it nothing to do)."""
    ev = Events()
    shapes = [(1 << 12, 20, 128), (1 << 14, 20, 1 << 10)] if quick else [(1 << 14, 100, 1024), (1 << 20, 100, 1 << 16)]
    for N, T, M in shapes:
        pf = make_filter(N, T)
        M_on2 = min(M, 1024)
        d_on2 = device(ev, lambda r: pf.hist.backward_sampling_ON2(M_on2, seed=100 + r)) * M / M_on2
        d_mc = device(ev, lambda r: pf.hist.backward_sampling_mcmc(M, nsteps=1, seed=100 + r))
        print("N=2^%d T=%d M=%d: MCMC nsteps=1 %.2f ms, ON2 %.2f ms%s"
              % (int(np.log2(N)), T, M, d_mc, d_on2, "" if M_on2 == M else " (timed at M=%d, scaled)" % M_on2))
        for max_trials in (M, 8):
            d = device(ev, lambda r: pf.hist.backward_sampling_reject(M, max_trials=max_trials, seed=100 + r))
            h = pf.hist
            down, loop = host_reject(pf, M, max_trials)
            print("  reject max_trials=%-6d device %.2f ms (%.1f us per backward step)  mean acc_rate %.4f  sum nexact %d"
                  "  trials per draw %.2f" % (max_trials, d, 1e3 * d / (T - 1), h.acc_rate.mean(), h.nexact.sum(),
                                              h.nprops.sum() / (M * (T - 1.0))))
            print("      host route: download %.1f ms + NumPy %.0f ms = %.0f ms; x%.0f" % (down, loop, down + loop, (down + loop) / d))
        del pf
    N, T, M = shapes[1]
    rng = np.random.RandomState(42)
    y = [np.atleast_1d(v) for v in 50.0 * rng.standard_normal(T)]
    pf = pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(rho=RHO, sigmaX=SX, sigmaY=50.0, sigma0=20.0), data=y), N=N, seed=7,
                ESSrmin=0.5, store_history=True, collect="off")
    pf.run()
    for solo in ("", str(M)):
        if solo:
            os.environ["SMC_REJECT_SOLO_TRIALS"] = solo
        try:
            d = device(ev, lambda r: pf.hist.backward_sampling_reject(M, max_trials=M, seed=100 + r))
        finally:
            os.environ.pop("SMC_REJECT_SOLO_TRIALS", None)
        h = pf.hist
        print("low acceptance (sigmaY=50, sigma0=20) N=2^%d T=%d M=%d max_trials=M, %s: device %.2f ms  mean acc_rate %.4f"
              "  sum nexact %d  trials per draw %.2f"
              % (int(np.log2(N)), T, M, "solo launch only" if solo else "solo (4 trials) + wave launch", d, h.acc_rate.mean(),
                 h.nexact.sum(), h.nprops.sum() / (M * (T - 1.0))))


def main():
    quick = "--quick" in sys.argv
    if "--reject" in sys.argv:
        return reject_legs(quick)
    ev = Events()
    N, T, M = (1 << 12, 20, 128) if quick else (1 << 14, 100, 1024)
    pf = make_filter(N, T)
    d = device(ev, lambda r: pf.hist.backward_sampling_ON2(M, seed=100 + r))
    down, loop = host_on2(pf, M, 8)
    print("ON2   N=2^%d T=%d M=%d: device %.2f ms (%.1f us per backward step, %.2f G particle-trajectory pairs/s)"
          % (int(np.log2(N)), T, M, d, 1e3 * d / (T - 1), 1.0 * N * M * (T - 1) / d / 1e6))
    print("      host route: download %.1f ms + NumPy loop %.0f ms (8 trajectories timed, scaled to M) = %.0f ms; x%.0f"
          % (down, loop, down + loop, (down + loop) / d))
    del pf
    N, T, M = (1 << 14, 20, 1 << 10) if quick else (1 << 20, 100, 1 << 16)
    pf = make_filter(N, T)
    for nsteps in (1, 3):
        d = device(ev, lambda r: pf.hist.backward_sampling_mcmc(M, nsteps=nsteps, seed=100 + r))
        down, loop = host_mcmc(pf, M, nsteps)
        print("MCMC  N=2^%d T=%d M=2^%d nsteps=%d: device %.2f ms (%.1f us per backward step)"
              % (int(np.log2(N)), T, int(np.log2(M)), nsteps, d, 1e3 * d / (T - 1)))
        print("      host route: download %.1f ms + NumPy %.0f ms = %.0f ms; x%.0f" % (down, loop, down + loop, (down + loop) / d))


if __name__ == "__main__":
    main()
