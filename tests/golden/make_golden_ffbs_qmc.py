"""Generate tests/golden/ffbs_qmc_lg.npz by RUNNING THE REFERENCE's QMC backward sampler
(particles/smoothing.py:425-456 backward_sampling_qmc) behind its own SQMC forward pass.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ffbs_qmc.py

LinearGauss(rho=0.9, sigmaX=1, sigmaY=1.5), T = 6 observations simulated under np.random.seed(DATA_SEED), then
SMC(qmc=True, store_history=True) with N = 128 and backward_sampling_qmc(64) with rqmc.sobol wrapped so that the
(M, T) point set of the backward pass is recorded.  scipy's Sobol' engine seeds itself: the file is the record of
ONE run, not a reproducible one -- a second run writes another history and other paths.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle", "numba_shim"), "/root/reference"]

import numpy as np  # noqa: E402
import particles  # noqa: E402
from particles import kalman  # noqa: E402
from particles import rqmc  # noqa: E402
from particles import state_space_models as ssm  # noqa: E402

N, T, M, DATA_SEED = 128, 6, 64, 2024


def main():
    np.random.seed(DATA_SEED)
    model = kalman.LinearGauss(rho=0.9, sigmaX=1.0, sigmaY=1.5)
    x, y = model.simulate(T)
    pf = particles.SMC(fk=ssm.Bootstrap(ssm=model, data=y), N=N, qmc=True, store_history=True)
    pf.run()
    assert len(pf.hist.X) == T and len(pf.hist.h_orders) == T - 1

    calls = []
    sobol0 = rqmc.sobol

    def sobol(n, d):
        u = sobol0(n, d)
        calls.append(np.array(u))
        return u

    rqmc.sobol = sobol
    try:
        paths = pf.hist.backward_sampling_qmc(M)
    finally:
        rqmc.sobol = sobol0
    assert len(calls) == 1 and calls[0].shape == (M, T)
    X = np.array([np.squeeze(v) for v in pf.hist.X])
    np.savez_compressed(os.path.join(HERE, "ffbs_qmc_lg.npz"), y=np.squeeze(np.array(y)), X=X,
                        lw=np.array([w.lw for w in pf.hist.wgts]), W=np.array([w.W for w in pf.hist.wgts]),
                        h_orders=np.array(pf.hist.h_orders, dtype=np.int64), u=calls[0], paths=np.array(paths),
                        N=N, T=T, M=M, data_seed=DATA_SEED)
    print("ffbs_qmc_lg.npz: X", X.shape, "u", calls[0].shape, "paths", np.array(paths).shape)


if __name__ == "__main__":
    main()
