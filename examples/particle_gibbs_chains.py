"""C chains of Particle Gibbs state updates on the ToySSM model, all chains in two launches per update.

    python examples/particle_gibbs_chains.py [C] [N] [T] [sweeps]

Every chain holds a trajectory x_{0:T-1}.  One update runs a conditional particle filter around it
(``particles_amd.mcmc.CSMC``: particle 0 is the retained trajectory, chains are islands of one grid) and draws the
chain's new trajectory from the filter's history by backward sampling (``new_paths``).  The trajectories stay on the
device from one update to the next: ``paths_device`` of one filter is the ``xstar`` of the next.  The conditional
update leaves the smoothing law p(x_{0:T-1} | y_{0:T-1}) invariant at any N >= 2, so the average over chains approaches
the Kalman smoother's mean; the first sweep is an ordinary (unconditional) filter, as in the reference's
``ParticleGibbs.update_states``.
"""
import sys
import time

import numpy as np

import particles_amd as pa
from particles_amd import kalman
from particles_amd import mcmc
from particles_amd import state_space_models as ssm


def smoothing_mean(model, y):
    """E[x_t | y_{0:T-1}] of the stationary LinearGauss model, from the joint Gaussian."""
    T = len(y)
    s0 = model.sigma0 ** 2
    S = np.empty((T, T))
    for s in range(T):
        for t in range(T):
            lo, hi = min(s, t), max(s, t)
            var_lo = model.rho ** (2 * lo) * s0 + model.sigmaX ** 2 * sum(model.rho ** (2 * k) for k in range(lo))
            S[s, t] = model.rho ** (hi - lo) * var_lo
    P = np.linalg.inv(np.linalg.inv(S) + np.eye(T) / model.sigmaY ** 2)
    return P @ (np.asarray(y) / model.sigmaY ** 2)


def main():
    C, N, T, sweeps = (int(v) for v in (sys.argv[1:5] + ["256", "64", "50", "30"][len(sys.argv) - 1:]))
    np.random.seed(1)
    model = kalman.ToySSM(0.2)
    _, y = model.simulate(T)
    fk = ssm.Bootstrap(ssm=model, data=y)
    t0 = time.perf_counter()
    # sweep 0: an unconditional filter per chain, then one trajectory each
    pf = pa.SMC(fk=fk, N=N, n_islands=C, store_history=True, collect="off", seed=100)
    pf.run()
    x = mcmc.new_paths(pf, backward_step=True, seed=200)
    x_dev = pf.paths_device
    mean = np.zeros(T)
    for k in range(1, sweeps):
        cpf = mcmc.CSMC(fk=fk, N=N, xstar=x_dev, n_islands=C, seed=100 + k)
        cpf.run()
        x = cpf.new_paths(backward_step=True, seed=200 + k)
        x_dev = cpf.paths_device
        if k >= sweeps // 2:
            mean += x.mean(axis=0) / (sweeps - sweeps // 2)
    dt = time.perf_counter() - t0
    exact = smoothing_mean(model, np.ravel(y))
    print("%d chains x %d sweeps (N = %d, T = %d) in %.3f s" % (C, sweeps, N, T, dt))
    print("largest |mean over chains and sweeps - smoothing mean| = %.4f" % np.max(np.abs(mean - exact)))


if __name__ == "__main__":
    main()
