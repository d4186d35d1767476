"""Generate tests/golden/two_filter_lg.npz by RUNNING THE REFERENCE's two-filter smoothing
(particles/smoothing.py:487-575, ParticleHistory.two_filter_smoothing) on the `history` case of make_golden.py.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_two_filter.py

The forward pass is the `history` case (asserted equal to history.npz).  The information filter is the same bootstrap
filter on the reversed data under np.random.seed(INFO_SEED); its history is kept, (T, N) each.  The test function has
K = 3 components phi = (xf, xf^2, x xf) -- the t >= 1 form of make_golden_online.py's additive function -- and loggamma
is the log-density of the stationary law N(0, sigmaX^2 / (1 - rho^2)), kept as its three coefficients.

  on2 (T - 1, 3)      the O(N^2) estimate at every t
  on_*                t in ON_TIMES: the O(N) estimate and ESS without and with the modif_* arrays of smoothing_worker's
                      'two-filter_ON_prop', those arrays, and the pairs I, J the reference drew.  The method does not
                      return its draws: NumPy is seeded, the method called, then NumPy is seeded again and rs.multinomial
                      called twice in the method's order; the estimate recomputed from those pairs must equal the
                      method's (asserted).
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
from particles import resampling as rs  # noqa: E402
from particles import state_space_models as ssm  # noqa: E402
from scipy import stats  # noqa: E402

INFO_SEED = 77
ON_TIMES = (0, 14, 28)
ON_SEED = 500


class LinearGaussBound(kalman.LinearGauss):
    def upper_bound_log_pt(self, t):
        return -np.log(self.sigmaX) - 0.5 * np.log(2.0 * np.pi)


def phi_k(k):
    return [lambda x, xf: xf + 0.0 * x, lambda x, xf: xf ** 2 + 0.0 * x, lambda x, xf: x * xf][k]


def phi3(x, xf):
    return np.stack([phi_k(k)(x, xf) for k in range(3)], axis=-1)


def main():
    g = np.load(os.path.join(HERE, "history.npz"))
    T, N = int(g["T"]), int(g["N"])
    np.random.seed(int(g["data_seed"]))
    model = LinearGaussBound(rho=0.9, sigmaX=1.0, sigmaY=1.5)
    x, y = model.simulate(T)
    np.random.seed(int(g["run_seed"]))
    pf = particles.SMC(fk=ssm.Bootstrap(ssm=model, data=y), N=N, resampling="systematic", ESSrmin=0.5, store_history=True)
    pf.run()
    assert np.array_equal(np.array(pf.hist.X), g["hist_X"]) and np.array_equal(np.array(pf.hist.A[1:]), g["hist_A"])
    assert np.array_equal(np.array([w.lw for w in pf.hist.wgts]), g["hist_lw"]) and pf.logLt == float(g["logLt"])

    np.random.seed(INFO_SEED)
    info = particles.SMC(fk=ssm.Bootstrap(ssm=model, data=y[::-1]), N=N, resampling="systematic", ESSrmin=0.5,
                         store_history=True)
    info.run()
    info_X = np.array(info.hist.X)
    info_lw = np.array([w.lw for w in info.hist.wgts])
    assert info_X.shape == (T, N) == info_lw.shape

    var = model.sigmaX ** 2 / (1.0 - model.rho ** 2)
    loggamma3 = np.array([-0.5 * np.log(2.0 * np.pi * var), 0.0, -0.5 / var])
    loggamma = lambda xx: stats.norm.logpdf(xx, loc=0.0, scale=np.sqrt(var))
    assert np.allclose(loggamma(info_X[3]), loggamma3[0] + loggamma3[2] * info_X[3] ** 2, rtol=1e-13, atol=1e-13)

    on2 = np.array([[pf.hist.two_filter_smoothing(t, info, phi_k(k), loggamma) for k in range(3)] for t in range(T - 1)])
    assert on2.shape == (T - 1, 3) and np.all(np.isfinite(on2))

    out = {}
    for t in ON_TIMES:
        ti = T - 2 - t
        mf = stats.norm.logpdf(pf.hist.X[t], loc=np.mean(info.hist.X[ti + 1]), scale=np.std(info.hist.X[ti + 1]))
        mi = stats.norm.logpdf(info.hist.X[ti], loc=np.mean(pf.hist.X[t + 1]), scale=np.std(pf.hist.X[t + 1]))
        for tag, a, b in (("plain", None, None), ("prop", mf, mi)):
            np.random.seed(ON_SEED + t)
            est, ess = pf.hist.two_filter_smoothing(t, info, phi3, loggamma, linear_cost=True, return_ess=True,
                                                    modif_forward=a, modif_info=b)
            # the method's draws again, in its order (smoothing.py:555-564)
            np.random.seed(ON_SEED + t)
            lwinfo = info.hist.wgts[ti].lw - loggamma(info.hist.X[ti])
            if b is not None:
                lwinfo = lwinfo + b
            I = rs.multinomial(rs.exp_and_normalise(lwinfo))
            W = pf.hist.wgts[t].W if a is None else rs.exp_and_normalise(pf.hist.wgts[t].lw + a)
            J = rs.multinomial(W)
            lo = pf.fk.logpt(t + 1, pf.hist.X[t][J], info.hist.X[ti][I])
            if a is not None:
                lo = lo - a[J]
            if b is not None:
                lo = lo - b[I]
            Om = rs.exp_and_normalise(lo)
            again = np.average(phi3(pf.hist.X[t][J], info.hist.X[ti][I]), axis=0, weights=Om)
            assert np.array_equal(again, est) and 1.0 / np.sum(Om ** 2) == ess
            out["on_%s_est_%d" % (tag, t)] = est
            out["on_%s_ess_%d" % (tag, t)] = ess
            out["on_%s_I_%d" % (tag, t)] = np.asarray(I, dtype=np.int64)
            out["on_%s_J_%d" % (tag, t)] = np.asarray(J, dtype=np.int64)
        out["modif_forward_%d" % t] = mf
        out["modif_info_%d" % t] = mi
    np.savez_compressed(os.path.join(HERE, "two_filter_lg.npz"), hist_X=info_X, hist_lw=info_lw, info_seed=INFO_SEED,
                        info_logLt=info.logLt, on2=on2, loggamma3=loggamma3, on_times=np.array(ON_TIMES), on_seed=ON_SEED,
                        data_seed=int(g["data_seed"]), run_seed=int(g["run_seed"]), **out)
    print("two_filter_lg.npz: info logLt", info.logLt, "on2[0]", on2[0], "on2[-1]", on2[-1])


if __name__ == "__main__":
    main()
