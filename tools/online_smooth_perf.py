"""On-line smoothing collectors (collectors.Online_smooth_naive / Online_smooth_ON2 / Paris) on the device route
(smc_filter_online_smooth) against the NumPy route on the same particles.

    python tools/online_smooth_perf.py [--quick]      (on a GPU box; the output is profiles/online_smooth_perf.txt)

A filter is stepped once with the collector and the collector's device arrays (Phi_0, X_0, lw_0) are copied out; after
the second step they are put back before every timed call, so that each call is the update of step 1 on the real pair
(X_0, X_1) -- what matters for Paris, whose trial count depends on the pair.  HIP events around the whole call (every
launch of the update, its two device-to-device copies and the download of the K estimates), after a warm-up call: median
and range of 20 calls.  The host route is timed once with perf_counter, on the same pair, where it takes under a minute.
"pairs/s" is N^2 over the time of the WHOLE update, not of k_os_on2 alone; it is to be read beside tools/ffbs_perf.py's
figure for backward_sampling_ON2 (N M pairs per backward step, also whole-call time) from the same session.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import particles_amd as pa
from ffbs_perf import RHO, SX, SY, Events
from particles_amd import _lib
from particles_amd import collectors as col
from particles_amd import kalman
from particles_amd import state_space_models as ssm


def psi(K):
    """K components out of x, x^2, xp x, xp^2 (the sufficient statistics of the Gaussian AR(1) family)."""
    c0 = np.zeros((4, 3))
    c = np.zeros((4, 3, 3))
    c0[0, 1] = c0[1, 2] = 1.0
    c[0, 0, 1] = c[1, 0, 2] = c[2, 1, 1] = c[3, 2, 0] = 1.0
    return ssm.QuadAddFunc(c0[:K], c[:K]) if K > 1 else ssm.QuadAddFunc([0.0, 0.0, 1.0], [[0, 0, 1.0], [0, -2.0, 0], [1.0, 0, 0]])


def make_filter(N, collector, K):
    rng = np.random.RandomState(42)
    x = np.cumsum(rng.standard_normal(4)) * 0.3
    y = [np.atleast_1d(v) for v in x + SY * rng.standard_normal(4)]
    model = kalman.LinearGauss(rho=RHO, sigmaX=SX, sigmaY=SY)
    model.add_func = psi(K)
    pf = pa.SMC(fk=ssm.Bootstrap(ssm=model, data=y), N=N, seed=7, ESSrmin=0.5, collect=[collector])
    next(pf)
    c = pf.summaries._collectors[-1]
    assert c._route == "device"
    saved = [a.get() for a in c._dev]              # Phi_0, X_0, lw_0
    next(pf)
    return pf, c, saved


def device(ev, pf, c, saved, reps=20):
    """(median, min, max) ms of the update of step 1, the collector's state put back to step 0 before each call."""
    def call():
        for a, h in zip(c._dev, saved):
            _lib.check(_lib.lib().smc_memcpy_h2d(a.ctx.h, a.ptr, h.ctypes.data_as(_lib.c_vp), h.nbytes))
        pf._ctx.sync()
        pf.t -= 1                                  # (what a collector sees: the index of the step just done)
        try:
            return ev.time(lambda: c._fetch_device(pf))[0]
        finally:
            pf.t += 1
    call()
    ms = [call() for _ in range(reps)]
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


class _Weights:
    pass


class _Smc:
    _fused, qmc = False, False


def host(pf, saved, cls, **kw):
    """One update of the NumPy route on the same pair: step 0 from the saved arrays, then the filter's step 1."""
    h = cls(**kw)
    s = _Smc()
    s.fk, s.N, s.wgts = pf.fk, pf.N, _Weights()
    lw0 = saved[2]
    w = np.exp(lw0 - lw0.max())
    s.t, s.X, s.W, s.A = 0, saved[1], w / w.sum(), None
    s.wgts.lw = lw0
    h.collect(s)
    s.t, s.X, s.W, s.A = 1, np.array(pf.X), np.array(pf.W), np.array(pf.A)
    s.wgts.lw = np.array(pf.wgts.lw)
    t0 = time.perf_counter()
    h.collect(s)
    return 1e3 * (time.perf_counter() - t0)


def main():
    quick = "--quick" in sys.argv
    ev = Events()
    fmt = "%.3f ms per update (%.3f - %.3f)"
    for log2N in ((10, 12) if quick else (12, 14, 16)):
        for K in (1, 4):
            N = 1 << log2N
            pf, c, saved = make_filter(N, col.Online_smooth_ON2(), K)
            d, lo, hi = device(ev, pf, c, saved)
            line = ("ON2    N=2^%d K=%d: device " + fmt + ", %.1f G pairs/s over the whole update") \
                   % (log2N, K, d, lo, hi, 1.0 * N * N / d / 1e6)
            if log2N <= (12 if quick else 14):
                h = host(pf, saved, col.Online_smooth_ON2)
                line += "; host route %.0f ms; x%.0f" % (h, h / d)
            print(line, flush=True)
            del pf, c
    N = 1 << (14 if quick else 20)
    pf, c, saved = make_filter(N, col.Online_smooth_naive(), 1)
    d, lo, hi = device(ev, pf, c, saved)
    h = host(pf, saved, col.Online_smooth_naive)
    print(("naive  N=2^%d K=1: device " + fmt + "; host route %.1f ms; x%.0f") % (int(np.log2(N)), d, lo, hi, h, h / d), flush=True)
    del pf, c
    for log2N in ((12,) if quick else (14, 20)):
        N = 1 << log2N
        pf, c, saved = make_filter(N, col.Paris(Nparis=2, seed=11), 1)
        d, lo, hi = device(ev, pf, c, saved)
        line = ("Paris  N=2^%d K=1 Nparis=2 max_trials=N: device " + fmt + ", %.2f trials per index") \
               % (log2N, d, lo, hi, c.nprop[-1] / (2.0 * N))
        if log2N <= 14:          # (the host route makes one NumPy round per trial: up to N rounds for the slowest index)
            np.random.seed(3)
            h = host(pf, saved, col.Paris, Nparis=2)
            line += "; host route %.0f ms; x%.0f" % (h, h / d)
        print(line, flush=True)
        del pf, c


if __name__ == "__main__":
    main()
