"""Generate tests/golden/online_smooth_lg.npz by RUNNING THE REFERENCE's on-line smoothing collectors
(particles/collectors.py:345-449 Online_smooth_naive, Online_smooth_ON2, Paris) on the `history` case of make_golden.py.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_online.py

The additive function has K = 3 components: (x, x^2, 0) at t = 0 and (x, x^2, xp x) afterwards.  Neither the naive nor
the O(N^2) collector draws random numbers, so the forward pass with them must still equal history.npz (asserted).  The
file keeps both (T, 3) arrays of estimates and the final Phi of the O(N^2) recursion.  A second run under
np.random.seed(PARIS_SEED) adds Paris(Nparis=2): its draws move NumPy's stream, so that forward pass is another one; its
estimates and nprop are kept for a comparison in law.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle", "numba_shim"), "/root/reference"]

import numpy as np  # noqa: E402
import particles  # noqa: E402
from particles import collectors as col  # noqa: E402
from particles import kalman  # noqa: E402
from particles import state_space_models as ssm  # noqa: E402

PARIS_SEED = 12


class LinearGaussStats(kalman.LinearGauss):
    def upper_bound_log_pt(self, t):
        return -np.log(self.sigmaX) - 0.5 * np.log(2.0 * np.pi)

    def add_func(self, t, xp, x):
        if t == 0:
            x = np.asarray(x, dtype=np.float64)
            return np.stack([x, x ** 2, np.zeros_like(x)], axis=-1)
        xp, x = np.broadcast_arrays(np.asarray(xp, dtype=np.float64), np.asarray(x, dtype=np.float64))
        return np.stack([x, x ** 2, xp * x], axis=-1)


def main():
    g = np.load(os.path.join(HERE, "history.npz"))
    T, N = int(g["T"]), int(g["N"])
    np.random.seed(int(g["data_seed"]))
    model = LinearGaussStats(rho=0.9, sigmaX=1.0, sigmaY=1.5)
    x, y = model.simulate(T)
    np.random.seed(int(g["run_seed"]))
    pf = particles.SMC(fk=ssm.Bootstrap(ssm=model, data=y), N=N, resampling="systematic", ESSrmin=0.5,
                       store_history=True, collect=[col.Online_smooth_naive(), col.Online_smooth_ON2()])
    pf.run()
    assert np.array_equal(np.array(pf.hist.X), g["hist_X"]) and np.array_equal(np.array(pf.hist.A[1:]), g["hist_A"])
    assert np.array_equal(np.array([w.lw for w in pf.hist.wgts]), g["hist_lw"]) and pf.logLt == float(g["logLt"])
    naive = np.array(pf.summaries.online_smooth_naive)
    on2 = np.array(pf.summaries.online_smooth_ON2)
    phi = np.array([c for c in pf.summaries._collectors if isinstance(c, col.Online_smooth_ON2)][0].Phi)
    assert naive.shape == (T, 3) == on2.shape and phi.shape == (N, 3)

    np.random.seed(PARIS_SEED)
    pp = particles.SMC(fk=ssm.Bootstrap(ssm=model, data=y), N=N, resampling="systematic", ESSrmin=0.5,
                       collect=[col.Paris(Nparis=2)])
    pp.run()
    paris = np.array(pp.summaries.paris)
    nprop = np.array([c for c in pp.summaries._collectors if isinstance(c, col.Paris)][0].nprop, dtype=np.float64)
    assert paris.shape == (T, 3) and nprop.shape == (T,)
    np.savez_compressed(os.path.join(HERE, "online_smooth_lg.npz"), naive=naive, on2=on2, on2_Phi=phi, paris=paris,
                        paris_nprop=nprop, paris_seed=PARIS_SEED, data_seed=int(g["data_seed"]), run_seed=int(g["run_seed"]))
    print("online_smooth_lg.npz: last ON2 row", on2[-1], "last naive row", naive[-1], "last Paris row", paris[-1])


if __name__ == "__main__":
    main()
