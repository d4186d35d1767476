"""The NumPy route of the on-line smoothing collectors (particles_amd.collectors), without a device: fed the rows of
tests/golden/history.npz through a stand-in smc object, it gives the reference's own estimates
(tests/golden/online_smooth_lg.npz, written by tests/golden/make_golden_online.py) within 1e-12 relative."""
import numpy as np
import scipy.stats

from particles_amd import collectors as col
from particles_amd import state_space_models as ssm

PSI3 = ssm.QuadAddFunc([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]],
                       [[[0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
                        [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
                        [[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]])


def _python_psi3(t, xp, x):
    x = np.asarray(x, dtype=np.float64)
    return np.stack([x, x ** 2, np.zeros_like(x) if t == 0 else xp * x], axis=-1)


class _FK:
    """The Feynman-Kac side the host route reads: the LinearGauss transition of the `history` case in NumPy."""

    def __init__(self, add_func):
        self.add_func = add_func

    def logpt(self, t, xp, x):
        return scipy.stats.norm.logpdf(x, loc=0.9 * xp, scale=1.0)

    def upper_bound_trans(self, t):
        return -0.5 * np.log(2.0 * np.pi)


class _Weights:
    pass


class _Smc:
    _fused, qmc = False, False

    def __init__(self, fk, N):
        self.fk, self.N, self.wgts = fk, N, _Weights()


def _feed(golden, collectors, add_func):
    g = golden("history")
    T, N = int(g["T"]), int(g["N"])
    smc = _Smc(_FK(add_func), N)
    for t in range(T):
        lw = g["hist_lw"][t]
        w = np.exp(lw - lw.max())
        smc.t, smc.X, smc.W = t, g["hist_X"][t], w / w.sum()
        smc.wgts.lw = lw
        smc.A = g["hist_A"][t - 1] if t else None
        for c in collectors:
            c.collect(smc)
    return T, N


def test_quad_add_func_is_the_polynomial():
    rng = np.random.default_rng(1)
    xp, x = rng.normal(size=50), rng.normal(size=50)
    assert np.allclose(PSI3(3, xp, x), _python_psi3(3, xp, x), rtol=1e-15, atol=0)
    assert np.allclose(PSI3(0, None, x), _python_psi3(0, None, x), rtol=1e-15, atol=0)
    assert PSI3(2, xp, 0.5).shape == (50, 3) and PSI3(2, xp[:, None], x[None, :7]).shape == (50, 7, 3)
    one = ssm.QuadAddFunc([0.0, 0.0, 1.0], [[0.0, 0.0, 1.0], [0.0, -2.0, 0.0], [1.0, 0.0, 0.0]])
    assert one.K == 1 and one(1, xp, x).shape == (50,) and np.allclose(one(1, xp, x), (xp - x) ** 2, rtol=1e-13, atol=1e-15)
    assert np.array_equal(one(0, None, x), x ** 2)


def test_host_route_gives_the_references_estimates(golden):
    fx = golden("online_smooth_lg")
    for add_func in (PSI3, _python_psi3):
        naive, on2 = col.Online_smooth_naive(), col.Online_smooth_ON2()
        T, N = _feed(golden, [naive, on2], add_func)
        assert naive._route == "host" == on2._route
        assert np.shape(naive.summary) == (T, 3) == np.shape(on2.summary) and on2.Phi.shape == (N, 3)
        for got, want in ((naive.summary, fx["naive"]), (on2.summary, fx["on2"]), (on2.Phi, fx["on2_Phi"])):
            err = np.abs(np.array(got) - want) / np.maximum(np.abs(want), 1e-300)
            print("max relative error", err.max())
            assert np.all(np.abs(np.array(got) - want) <= 1e-12 * np.abs(want))


def test_host_paris_has_the_law_of_the_on2_smoother(golden):
    """Paris on the host route draws from np.random: over 16 seeded runs the mean of the final estimates lies within 4
    standard errors of the exact O(N^2) value; nprop counts at least one trial per index."""
    fx = golden("online_smooth_lg")
    finals = []
    for r in range(16):
        np.random.seed(900 + r)
        p = col.Paris(Nparis=2)
        T, N = _feed(golden, [p], PSI3)
        finals.append(p.summary[-1])
        assert len(p.nprop) == T and p.nprop[0] == 0.0 and all(n >= 2 * N for n in p.nprop[1:])
    finals = np.array(finals)
    z = (finals.mean(axis=0) - fx["on2"][-1]) / (finals.std(axis=0, ddof=1) / 4.0)
    print("host paris z", z)
    assert np.all(np.abs(z) < 4.0)
