"""QMC backward sampling on the device (DeviceParticleHistory.backward_sampling_qmc, smc_filter_backward_qmc) in its two
launch geometries against the exact sampler of a non-QMC filter of the same shape (backward_sampling_ON2: the comparable
path there was before).

    python tools/ffbs_qmc_perf.py [--quick]        (on a GPU box; the output is profiles/ffbs_qmc_perf.txt)

Every figure is the median of 20 whole calls after a warm-up call per variant, timed with the host clock around the
call: a call ends in its one synchronisation (the download of the (T, M) indices and paths), and includes the upload of
the (M, T) points.  The three variants of a shape -- geometry 1 (workgroup per trajectory), geometry 2 (thread per
trajectory), ON2 -- alternate call by call in one process.  The points are one fixed seeded Sobol' set (generated once,
outside the timing).  G pairs/s = N M (T - 1) / time.  The share of sort + gather is the sum of the HIP-event intervals
around those launches (smc_debug_backward_qmc_timing) over the time of the same call, median over the calls.
"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import particles_amd as pa
from particles_amd import _lib, kalman, rqmc
from particles_amd import resampling as rs_mod
from particles_amd import state_space_models as ssm

RHO, SX, SY = 0.9, 1.0, 1.5
REPS = 20


def make_filter(N, T, qmc):
    rng = np.random.RandomState(42)
    x = np.cumsum(rng.standard_normal(T)) * 0.3
    y = [np.atleast_1d(v) for v in x + SY * rng.standard_normal(T)]
    fk = ssm.Bootstrap(ssm=kalman.LinearGauss(rho=RHO, sigmaX=SX, sigmaY=SY), data=y)
    if qmc:
        pf = pa.SMC(fk=fk, N=N, qmc=True, seed=7, store_history=True, collect="off")
    else:
        pf = pa.SMC(fk=fk, N=N, seed=7, ESSrmin=0.5, store_history=True, collect="off")
    assert pf._fused and isinstance(pf.hist, pa.collectors.DeviceParticleHistory)
    pf.run()
    return pf


def sort_ms():
    ms = ctypes.c_double()
    _lib.check(_lib.lib().smc_debug_backward_qmc_timing(1, ctypes.byref(ms)))
    return ms.value


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def shape(N, T, M, reps):
    q, p = make_filter(N, T, True), make_filter(N, T, False)
    u = rqmc.sobol_points(M, T, seed=1)
    calls = {
        "geometry 1": lambda r: q.hist.backward_sampling_qmc(M, replay={"u": u}, geometry=1),
        "geometry 2": lambda r: q.hist.backward_sampling_qmc(M, replay={"u": u}, geometry=2),
        "ON2": lambda r: p.hist.backward_sampling_ON2(M, seed=100 + r),
    }
    a = q.hist.backward_sampling_qmc(M, replay={"u": u}, geometry=1, return_idx=True)[1]     # (warm-up, and the contract)
    b = q.hist.backward_sampling_qmc(M, replay={"u": u}, geometry=2, return_idx=True)[1]
    assert np.array_equal(a, b)
    calls["ON2"](0)
    ms = {k: [] for k in calls}
    share = {k: [] for k in calls if k != "ON2"}
    for r in range(reps):
        for k, fn in calls.items():
            t = clock(lambda: fn(1 + r))
            ms[k].append(t)
            if k in share:
                share[k].append(sort_ms() / t)
    pairs = 1.0 * N * M * (T - 1)
    print("N=2^%d T=%d M=%d  (%d calls each, alternating)" % (int(np.log2(N)), T, M, reps))
    for k in calls:
        med, lo, hi = np.median(ms[k]), np.min(ms[k]), np.max(ms[k])
        extra = "" if k == "ON2" else "  sort + gather %.1f %% of the call" % (100.0 * np.median(share[k]))
        print("  %-10s %9.2f ms (min %.2f max %.2f)  %7.1f G pairs/s%s" % (k, med, lo, hi, pairs / med / 1e6, extra))
    on2, g1, g2 = (float(np.median(ms[k])) for k in ("ON2", "geometry 1", "geometry 2"))
    print("  geometry 1 / ON2 = %.3f   geometry 2 / geometry 1 = %.3f" % (g1 / on2, g2 / g1))
    return g1, g2


def main():
    quick = "--quick" in sys.argv
    rs_mod.set_rng("philox")                       # device-generated draws for both filters (SQMC fuses in this mode only)
    _lib.check(_lib.lib().smc_debug_backward_qmc_timing(1, None))
    print("smc_version:", _lib.lib().smc_version().decode())
    Ms = (256, 1024) if quick else (256, 1024, 4096, 1 << 14)
    N, T = (1 << 12, 20) if quick else (1 << 14, 100)
    wins = []
    for M in Ms:
        g1, g2 = shape(N, T, M, 3 if quick else REPS)
        if g2 < g1:
            wins.append(M)
    print("geometry 2 wins at N=2^%d for M in %s" % (int(np.log2(N)), wins or "none of the measured M"))
    if not quick:
        shape(1 << 20, 20, 1 << 14, REPS)


if __name__ == "__main__":
    main()
