"""Conditional SMC on the device (particles_amd.mcmc.CSMC: k_csmc_small, k_csmc_path) next to what the tree had before it.

    python tools/csmc_perf.py [--quick]      (on a GPU box; the output is profiles/csmc_perf.txt)

Shape C1: LinearGauss bootstrap, N = 1000, T = 200, n_islands in {1, 64, 1024, 4096}; whole history kept by both filters
(16.5 GB per filter at 4096 islands: where the device has not that much free the size is reported as not measured, and
4096 islands are timed at T = 50 as well).

  filter run   the conditional run (multinomial, Philox: N - 1 draws of stream 6 and a binary search in LDS per resampling
               step) against the unconditional k_filter_small run of the same shape (systematic, Philox).  A filter runs
               once, so every timed run is a fresh filter; its creation is outside the timed region: device sync, T
               steps enqueued in one call, device sync.  The two alternate in one process; median (min - max) of 20.
  paths        new_paths(backward_step=True) -- one launch for all islands -- against the route the tree offered before:
               one backward_sampling_ON2(1, island=i) per island, T - 1 dependent launches each (the general sampler,
               DeviceParticleHistory._backward).  The old route is timed on 3 calls and left out beyond 1024 islands.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import particles_amd as pa
from particles_amd import _lib
from particles_amd import kalman
from particles_amd import mcmc
from particles_amd import state_space_models as ssm

RHO, SX, SY = 0.9, 1.0, 1.5
N = 1000


def describe(pf):
    import ctypes
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().smc_filter_describe(pf._f, buf, 256))
    return buf.value.decode()


def wall(fn):
    """Milliseconds of fn() with a device synchronisation on both sides."""
    _lib.ctx().sync()
    t0 = time.perf_counter()
    out = fn()
    _lib.ctx().sync()
    return 1e3 * (time.perf_counter() - t0), out


def stats(ms):
    return "%.3f ms (%.3f - %.3f)" % (float(np.median(ms)), float(np.min(ms)), float(np.max(ms)))


def main():
    quick = "--quick" in sys.argv
    for C, T in (((1, 200), (64, 200)) if quick else ((1, 200), (64, 200), (1024, 200), (4096, 50), (4096, 200))):
        try:
            measure(C, T, 5 if quick else 20)
        except MemoryError as e:
            print("islands=%4d T=%d: not measured (%s)" % (C, T, e), flush=True)


def measure(C, T, reps):
    rng = np.random.RandomState(42)
    x = np.cumsum(rng.standard_normal(T)) * 0.3
    y = [np.atleast_1d(v) for v in x + SY * rng.standard_normal(T)]
    fk = ssm.Bootstrap(ssm=kalman.LinearGauss(rho=RHO, sigmaX=SX, sigmaY=SY), data=y)
    print("conditional SMC, LinearGauss bootstrap, N = %d, T = %d, ESSrmin = 0.5, median (min - max) of %d" % (N, T, reps))
    xstar = np.tile(x, (C, 1))
    cond = lambda s: mcmc.CSMC(fk=fk, N=N, xstar=xstar, seed=s, n_islands=C)
    plain = lambda s: pa.SMC(fk=fk, N=N, seed=s, n_islands=C, store_history=True, collect="off")
    tc, tp, nres = [], [], 0
    for r in range(reps + 1):                            # (round 0: warm-up -- code objects, the pool's blocks)
        for mk, out in ((cond, tc), (plain, tp)):
            pf = mk(100 + r)
            if r == 0:
                assert describe(pf) == ("k_csmc_small" if mk is cond else "k_filter_small"), describe(pf)
            ms, _ = wall(lambda: pf.step_async(T))
            if r:
                out.append(ms)
            if mk is cond and r == 0:
                nres = pf._summ()[:, :, 4].sum() / C
            del pf                                       # (one filter at a time: 16 GB of history at 4096 islands)
    ratio = float(np.median(tc) / np.median(tp))
    print("filter run  islands=%4d: k_csmc_small %s | k_filter_small %s | ratio %.2f  (%.0f of %d steps resample)"
          % (C, stats(tc), stats(tp), ratio, nres, T), flush=True)
    # ---- the new trajectories of all islands
    pf = cond(100)
    pf.run()
    tn = [wall(lambda: pf.new_paths(backward_step=True, seed=7 + r))[0] for r in range(reps + 1)][1:]
    tg = [wall(lambda: pf.new_paths(backward_step=False, seed=7 + r))[0] for r in range(reps + 1)][1:]
    line = "paths       islands=%4d: one launch, backward %s | genealogy %s" % (C, stats(tn), stats(tg))
    if C <= 1024:
        old = lambda: [pf.hist._backward(_lib.BACKWARD_ON2, 1, 1, 7, i, None, True) for i in range(C)]
        to = [wall(old)[0] for r in range(1 + (1 if C > 64 else 3))][1:]
        line += " | %d calls of backward_sampling_ON2(1, island=i) %s: x%.0f" % (C, stats(to), np.median(to) / np.median(tn))
        a = pf.new_paths(backward_step=True, seed=7, return_idx=True)[1]
        assert all(np.array_equal(a[i], pf.hist._backward(_lib.BACKWARD_ON2, 1, 1, 7, i, None, True)[1][:, 0])
                   for i in range(min(C, 4)))
    print(line, flush=True)
    del pf


if __name__ == "__main__":
    main()

