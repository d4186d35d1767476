"""Two-filter smoothing (DeviceParticleHistory.two_filter_smoothing) on the device route (smc_filter_two_filter) against
the NumPy route on the same two histories, and next to the all-pairs on-line collector at the same N.

    python tools/two_filter_perf.py [--quick]      (on a GPU box; the output is profiles/two_filter_perf.txt)

A forward filter and an information filter (the same model on the reversed data) of N particles each are run for four
steps with a whole history; every timed call is two_filter_smoothing(t = 1).  HIP events around the whole call (every
launch, the uploads and the download of the estimates), after a warm-up call: median and range of 20 calls.  The NumPy
route is timed once with perf_counter, where it takes under a minute.  "pairs/s" is N_f N_i over the time of the WHOLE
call, not of k_tf_on2 alone.  For K = 1 the update of Online_smooth_ON2 (tools/online_smooth_perf.py: N^2 pairs, whole
update) is timed in the same process, the two alternating, four rounds of 20 calls each.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import particles_amd as pa
import online_smooth_perf as osp
from ffbs_perf import RHO, SX, SY, Events
from particles_amd import collectors as col
from particles_amd import kalman
from particles_amd import state_space_models as ssm

VAR = SX ** 2 / (1.0 - RHO ** 2)
GAMMA = ssm.QuadLogGamma(-0.5 * np.log(2.0 * np.pi * VAR), 0.0, -0.5 / VAR)


def make_pair(N):
    rng = np.random.RandomState(42)
    x = np.cumsum(rng.standard_normal(4)) * 0.3
    y = [np.atleast_1d(v) for v in x + SY * rng.standard_normal(4)]
    mk = lambda data, seed: pa.SMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(rho=RHO, sigmaX=SX, sigmaY=SY), data=data), N=N,
                                   seed=seed, ESSrmin=0.5, store_history=True, collect="off")
    pf, info = mk(y, 7), mk(y[::-1], 8)
    pf.run()
    info.run()
    return pf, info


def timed(ev, call, reps=20):
    call()
    ms = [ev.time(call)[0] for _ in range(reps)]
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


class _Host:
    """The same histories behind objects the device route does not take."""

    def __init__(self, q):
        self.N, self.qmc = q.N, False
        self.hist = col.ParticleHistory(q.fk, False)
        for t in range(q._n):
            self.hist.X.append(q.hist.X[t])
            self.hist.wgts.append(q.hist.wgts[t])
            self.hist.A.append(None)


def main():
    quick = "--quick" in sys.argv
    ev = Events()
    fmt = "%.3f ms per call (%.3f - %.3f)"
    for log2N in ((10,) if quick else (12, 14, 16)):
        N = 1 << log2N
        pf, info = make_pair(N)
        for K in (1, 4):
            phi = osp.psi(K)
            d, lo, hi = timed(ev, lambda: pf.hist.two_filter_smoothing(1, info, phi, GAMMA))
            assert pf.hist._two_filter_route == "device"
            line = ("ON2  N_f=N_i=2^%d K=%d: device " + fmt + ", %.1f G pairs/s over the whole call") \
                   % (log2N, K, d, lo, hi, 1.0 * N * N / d / 1e6)
            if log2N <= (10 if quick else 14) and K == 1:
                hf, hi_ = _Host(pf), _Host(info)
                t0 = time.perf_counter()
                hf.hist.two_filter_smoothing(1, hi_, phi, GAMMA)
                h = 1e3 * (time.perf_counter() - t0)
                line += "; NumPy route %.0f ms; x%.0f" % (h, h / d)
            print(line, flush=True)
        # the all-pairs collector at the same N, K = 1, alternating with the two-filter call
        phi = osp.psi(1)
        qf, c, saved = osp.make_filter(N, col.Online_smooth_ON2(), 1)
        for r in range(4):
            a = timed(ev, lambda: pf.hist.two_filter_smoothing(1, info, phi, GAMMA))
            b = osp.device(ev, qf, c, saved)
            print(("     round %d N=2^%d K=1: two-filter ON2 " + fmt + " = %.1f G pairs/s | Online_smooth_ON2 " + fmt
                   + " = %.1f G pairs/s") % ((r, log2N) + a + (1.0 * N * N / a[0] / 1e6,) + b + (1.0 * N * N / b[0] / 1e6,)),
                  flush=True)
        del pf, info, qf, c
    log2N = 14 if quick else 20
    N = 1 << log2N
    pf, info = make_pair(N)
    phi = osp.psi(1)
    d, lo, hi = timed(ev, lambda: pf.hist.two_filter_smoothing(1, info, phi, GAMMA, linear_cost=True, npairs=N, seed=11))
    hf, hi_ = _Host(pf), _Host(info)
    t0 = time.perf_counter()
    hf.hist.two_filter_smoothing(1, hi_, phi, GAMMA, linear_cost=True, npairs=N, seed=11)
    h = 1e3 * (time.perf_counter() - t0)
    print(("ON   N=2^%d npairs=2^%d K=1: device " + fmt + ", %.0f M pairs/s; NumPy route %.0f ms; x%.0f")
          % (log2N, log2N, d, lo, hi, N / d / 1e3, h, h / d), flush=True)


if __name__ == "__main__":
    main()
