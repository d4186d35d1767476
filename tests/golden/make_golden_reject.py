"""Generate tests/golden/ffbs_reject_lg.npz by RUNNING THE REFERENCE's hybrid rejection backward sampler
(particles/smoothing.py:352-423 backward_sampling_reject) on the `history` case of make_golden.py.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_reject.py

The forward pass is run again and must equal history.npz.  The reference leaves the bound of the transition
density to the user: the model here is its LinearGauss with upper_bound_log_pt = -log(sigmaX) - log(2 pi) / 2,
the largest value of the Gaussian transition density.  Under np.random.seed(11), 4096 trajectories are drawn
(max_trials = M, the reference's default); the file keeps their per-step means and the acceptance rates --
the device draws other uniforms, so it is pinned to these in law, not index by index.
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
from particles import state_space_models as ssm  # noqa: E402

M, REJECT_SEED = 4096, 11


class BoundedLinearGauss(kalman.LinearGauss):
    def upper_bound_log_pt(self, t):
        return -np.log(self.sigmaX) - 0.5 * np.log(2.0 * np.pi)


def main():
    g = np.load(os.path.join(HERE, "history.npz"))
    T, N = int(g["T"]), int(g["N"])
    np.random.seed(int(g["data_seed"]))
    model = BoundedLinearGauss(rho=0.9, sigmaX=1.0, sigmaY=1.5)
    x, y = model.simulate(T)
    np.random.seed(int(g["run_seed"]))
    pf = particles.SMC(fk=ssm.Bootstrap(ssm=model, data=y), N=N, resampling="systematic", ESSrmin=0.5,
                       store_history=True)
    pf.run()
    assert np.array_equal(np.array(pf.hist.X), g["hist_X"]) and np.array_equal(np.array(pf.hist.A[1:]), g["hist_A"])
    assert np.array_equal(np.array([w.lw for w in pf.hist.wgts]), g["hist_lw"]) and pf.logLt == float(g["logLt"])

    np.random.seed(REJECT_SEED)
    paths = pf.hist.backward_sampling_reject(M)
    means = np.array([np.mean(p) for p in paths])
    acc = np.array(pf.hist.acc_rate, dtype=np.float64)
    assert means.shape == (T,) and acc.shape == (T - 1,) and np.all(acc > 0.0) and np.all(acc <= 1.0)
    np.savez_compressed(os.path.join(HERE, "ffbs_reject_lg.npz"), path_means=means, acc_rate=acc, M=M,
                        reject_seed=REJECT_SEED, data_seed=int(g["data_seed"]), run_seed=int(g["run_seed"]))
    print("ffbs_reject_lg.npz: path_means", means.shape, "acc_rate", np.round(acc, 3))


if __name__ == "__main__":
    main()
