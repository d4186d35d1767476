"""The host side of conditional SMC: the Python restatement of the integer CDF contract the device tests compare
against, checked on its own against fractions; and particles_amd.adapter against the REAL reference package (build
container only, the kernels run through the emulator there): the reference's ParticleGibbs, unchanged, under
``install()`` builds device filters for both branches of ``update_states``."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import csmc_cases as cc
from conftest import ROOT

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "particles")),
                                     reason="the reference package is not on this box")


def test_integer_cdf_restatement_is_the_contract():
    """int_draws: q_n = rint(e_n 2^s), thr = floor(u Q), the first prefix above thr -- against exact rationals."""
    rng = np.random.default_rng(0)
    for N in (2, 5, 64, 257, 1024):
        e = rng.random(N) ** 4
        e[rng.random(N) < 0.2] = 0.0
        e[0], e[-1] = 0.5, 0.0                             # a dead last particle is never drawn
        us = np.concatenate([rng.random(200), [0.0, 1.0, 1.0 - 2.0 ** -53, 2.0 ** -1074]])
        got = cc.int_draws(e, us)
        s = cc.sm_shift(N)
        assert (1 << (61 - s)) >= N > (1 << (61 - s)) // 2 or N == 1
        q = [Fraction(int(round(v * 2.0 ** s))) for v in e]
        Q = sum(q)
        pre = np.cumsum(q)
        for u, n in zip(us, got):
            thr = min(Fraction(float(u)) * Q // 1, Q - 1)
            assert pre[n] > thr and (n == 0 or pre[n - 1] <= thr) and e[n] > 0.0
    assert cc.int_draws(np.zeros(7), [0.3])[0] == 6         # no weight at all: the last particle


def test_exact_smoothing_law_of_the_invariance_test():
    """exact_smoothing against the Kalman smoother of the same model (particles_amd.kalman has none: two-step case by
    hand)."""
    rho, sx, sy = 0.9, 1.0, 1.5
    y = np.array([0.3, -1.2])
    mean, P = cc.exact_smoothing(rho, sx, sy, y)
    s0 = sx ** 2 / (1 - rho ** 2)
    S = np.array([[s0, rho * s0], [rho * s0, s0]])           # stationary AR(1): Var x_1 = rho^2 s0 + sx^2 = s0
    K = S @ np.linalg.inv(S + sy ** 2 * np.eye(2))
    assert np.allclose(mean, K @ y, atol=1e-13) and np.allclose(P, S - K @ S, atol=1e-13)


@pytest.fixture(scope="module")
def ref():
    sys.dont_write_bytecode = True
    for p in (REF, os.path.join(ROOT, "oracle", "numba_shim")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import particles
    from particles import distributions, kalman, mcmc, state_space_models
    return dict(particles=particles, dists=distributions, kalman=kalman, mcmc=mcmc, ssm=state_space_models)


@needs_reference
def test_particle_gibbs_runs_both_filters_on_the_device_under_install(ref, monkeypatch):
    import particles_amd as pa
    from particles_amd import adapter
    from particles_amd import mcmc as dmcmc
    particles, rmcmc, rk, dists = ref["particles"], ref["mcmc"], ref["kalman"], ref["dists"]
    orig_smc, orig_csmc = particles.SMC, rmcmc.CSMC
    np.random.seed(3)
    _, y = rk.LinearGauss(rho=0.9, sigmaX=1.0, sigmaY=0.5).simulate(12)
    made = []
    init0 = dmcmc.CSMC.__init__
    smc0 = pa.core.SMC.__init__

    def csmc_init(self, *a, **kw):
        init0(self, *a, **kw)
        made.append(("csmc", self._fused, self.N))

    def smc_init(self, *a, **kw):
        smc0(self, *a, **kw)
        if type(self) is pa.core.SMC:
            made.append(("smc", self._fused, self.N))

    monkeypatch.setattr(dmcmc.CSMC, "__init__", csmc_init)
    monkeypatch.setattr(pa.core.SMC, "__init__", smc_init)

    class PG(rmcmc.ParticleGibbs):
        def update_theta(self, theta, x):
            return theta                                     # the states are what this test is about

    prior = dists.StructDist({"rho": dists.Uniform(0.5, 0.99)})
    theta0 = np.array([(0.9,)], dtype=[("rho", float)])
    adapter.install()
    try:
        assert rmcmc.CSMC is adapter.HipCSMC() and issubclass(rmcmc.CSMC, orig_csmc)
        for backward in (False, True):
            del made[:]
            pg = PG(niter=4, ssm_cls=rk.LinearGauss, prior=prior, data=y, theta0=theta0[0], Nx=50, backward_step=backward,
                    store_x=True)
            np.random.seed(5)
            pg.run()
            assert [m[0] for m in made] == ["smc", "csmc", "csmc", "csmc"], made
            assert all(fused and N == 50 for _, fused, N in made), made
            x = np.array(pg.chain.x)
            assert x.shape == (4, 12) and np.all(np.isfinite(x)) and len(np.unique(x[:, -1])) > 1
        # a configuration the device does not pin stays the reference's own class
        g = rmcmc.CSMC(fk=ref["ssm"].GuidedPF(ssm=rk.LinearGauss(), data=y), N=20, xstar=list(np.zeros(12)))
        assert type(g) is adapter.HipCSMC() and isinstance(g, orig_csmc)
    finally:
        adapter.uninstall()
    assert particles.SMC is orig_smc and rmcmc.CSMC is orig_csmc
    assert not hasattr(rmcmc, "_csmc_before_hip")
