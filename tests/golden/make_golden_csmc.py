"""Generate tests/golden/csmc_lg.npz by RUNNING THE REFERENCE's conditional particle filter (particles/mcmc.py:453-475,
CSMC) on a LinearGauss bootstrap model: N = 50, T = 20, ESSrmin = 0.5, xstar a simulated path.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_csmc.py

The reference's draws are recorded by patching the two functions it draws with: rs.random.rand (rs.multinomial's
uniform spacings: one rand(N + 1) call per resampling step) and the normal draw of distributions.Normal.rvs
(random.normal(loc, scale, size) = loc + scale * standard_normal(size), checked against an unpatched run).  The
fixture holds the data, xstar, the tapes (z (T, N) normals; u (T, N) the SORTED uniforms of the resampling steps) and
the reference's history X, lw, A (T, N; row 0 of A is arange, like the rows of the steps that do not resample) with its
resampling flags.

The device inverts every uniform in an exact integer CDF, the reference in a sequential fp64 one: the two can differ
where a uniform lies within rounding of a step of the CDF.  RUN_SEED is chosen so that no uniform of the run is within
1e-11 of any step (asserted below): the test then allows no exception at all.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle", "numba_shim"), "/root/reference"]

import numpy as np  # noqa: E402
from particles import distributions as dists  # noqa: E402
from particles import kalman  # noqa: E402
from particles import mcmc  # noqa: E402
from particles import resampling as rs  # noqa: E402
from particles import state_space_models as ssm  # noqa: E402

N, T, ESSRMIN = 50, 20, 0.5
DATA_SEED, RUN_SEED = 2024, 11
LG = dict(rho=0.9, sigmaX=1.0, sigmaY=1.5)


def run(y, xstar, record):
    calls_u, calls_z = [], []
    rand0, normal0 = rs.random.rand, dists.random.normal

    def rand(*shape):
        v = rand0(*shape)
        calls_u.append(np.atleast_1d(v).copy())
        return v

    def normal(loc=0.0, scale=1.0, size=None):
        z = np.random.standard_normal(size)
        calls_z.append(np.array(z))
        return loc + scale * z

    if record:
        rs.random.rand, dists.random.normal = rand, normal
    try:
        np.random.seed(RUN_SEED)
        pf = mcmc.CSMC(fk=ssm.Bootstrap(ssm=kalman.LinearGauss(**LG), data=y), N=N, ESSrmin=ESSRMIN, xstar=xstar)
        pf.run()
    finally:
        rs.random.rand, dists.random.normal = rand0, normal0
    return pf, calls_u, calls_z


def main():
    np.random.seed(DATA_SEED)
    model = kalman.LinearGauss(**LG)
    _, y = model.simulate(T)
    xs, _ = model.simulate(T)
    xstar = np.array(xs, dtype=np.float64).reshape(T)
    plain, _, _ = run(y, xstar, False)
    pf, calls_u, calls_z = run(y, xstar, True)
    X = np.array(pf.hist.X)
    lw = np.array([w.lw for w in pf.hist.wgts])
    W = np.array([w.W for w in pf.hist.wgts])
    A = np.array([np.arange(N)] + [np.asarray(a) for a in pf.hist.A[1:]])     # (row 0: no ancestors, hist.A[0] is None)
    assert np.array_equal(X, np.array(plain.hist.X)) and np.array_equal(lw, np.array([w.lw for w in plain.hist.wgts]))
    assert all(np.array_equal(a, b) for a, b in zip(pf.hist.A[1:], plain.hist.A[1:])) and pf.logLt == plain.logLt
    flags = np.array([False] + [not np.array_equal(A[t][1:], np.arange(1, N)) for t in range(1, T)])
    assert len(calls_z) == T and all(z.shape == (N,) for z in calls_z)
    assert len(calls_u) == flags.sum() and all(c.shape == (N + 1,) for c in calls_u)
    assert 3 <= flags.sum() < T - 3                      # steps of both kinds
    z = np.array(calls_z)
    u = np.zeros((T, N))
    margin, k = np.inf, 0
    for t in range(1, T):
        if flags[t]:
            sp = np.cumsum(-np.log(calls_u[k]))
            u[t] = sp[:-1] / sp[-1]                      # resampling.py:536-537
            k += 1
            assert np.array_equal(rs.inverse_cdf(u[t], W[t - 1])[1:], A[t][1:])
            cs = np.cumsum(W[t - 1])
            margin = min(margin, np.abs(cs[None, :] - u[t][1:, None]).min())
    assert margin > 1e-11, margin                        # no uniform within 1e-11 of a step of a CDF
    assert np.all(X[:, 0] == xstar) and np.all(A[:, 0] == 0)
    np.savez_compressed(os.path.join(HERE, "csmc_lg.npz"), y=np.array(y).reshape(T), xstar=xstar, z=z, u=u, X=X, lw=lw, A=A,
                        rs_flags=flags, N=N, T=T, ESSrmin=ESSRMIN, logLt=float(pf.logLt), data_seed=DATA_SEED,
                        run_seed=RUN_SEED, margin=margin, **{"lg_" + k_: v for k_, v in LG.items()})
    print("csmc_lg.npz: %d of %d steps resample, closest uniform to a CDF step %.3e" % (flags.sum(), T, margin))


if __name__ == "__main__":
    main()
