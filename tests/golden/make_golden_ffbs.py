"""Generate tests/golden/ffbs_lg.npz by RUNNING THE REFERENCE's exact backward sampler
(particles/smoothing.py:291-311 backward_sampling_ON2) on the `history` case of make_golden.py.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ffbs.py

The forward pass is run again and must equal history.npz; then, under np.random.seed(7), 64 trajectories
are drawn with the reference's uniforms recorded: one rand(65) call (rs.multinomial's uniform spacings of the
last row) and then 64 x 29 scalar draws (rs.multinomial_once), trajectory m the outer loop, t reversed the
inner one.  The (T, M) index array is taken from _output_backward_sampling's argument.
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
from particles import smoothing  # noqa: E402
from particles import state_space_models as ssm  # noqa: E402

M, FFBS_SEED = 64, 7


def main():
    g = np.load(os.path.join(HERE, "history.npz"))
    T, N = int(g["T"]), int(g["N"])
    np.random.seed(int(g["data_seed"]))
    model = kalman.LinearGauss(rho=0.9, sigmaX=1.0, sigmaY=1.5)
    x, y = model.simulate(T)
    np.random.seed(int(g["run_seed"]))
    pf = particles.SMC(fk=ssm.Bootstrap(ssm=model, data=y), N=N, resampling="systematic", ESSrmin=0.5,
                       store_history=True)
    pf.run()
    assert np.array_equal(np.array(pf.hist.X), g["hist_X"]) and np.array_equal(np.array(pf.hist.A[1:]), g["hist_A"])
    assert np.array_equal(np.array([w.lw for w in pf.hist.wgts]), g["hist_lw"]) and pf.logLt == float(g["logLt"])

    calls, seen = [], {}
    rand0 = rs.random.rand
    out0 = smoothing.ParticleHistory._output_backward_sampling

    def rand(*shape):
        v = rand0(*shape)
        calls.append(np.atleast_1d(v).copy())
        return v

    def output(self, idx):
        seen["idx"] = np.array(idx)
        return out0(self, idx)

    rs.random.rand = rand
    smoothing.ParticleHistory._output_backward_sampling = output
    try:
        np.random.seed(FFBS_SEED)
        paths = pf.hist.backward_sampling_ON2(M)
    finally:
        rs.random.rand = rand0
        smoothing.ParticleHistory._output_backward_sampling = out0
    assert len(calls) == 1 + M * (T - 1) and calls[0].shape == (M + 1,) and all(c.shape == (1,) for c in calls[1:])
    # draw (m, t) is call 1 + m (T - 1) + (T - 2 - t): rows of u are time steps, columns trajectories
    u = np.array([c[0] for c in calls[1:]]).reshape(M, T - 1)[:, ::-1].T.copy()
    idx = seen["idx"]
    assert idx.shape == (T, M) and u.shape == (T - 1, M)
    assert all(np.array_equal(paths[t], g["hist_X"][t][idx[t]]) for t in range(T))
    np.savez_compressed(os.path.join(HERE, "ffbs_lg.npz"), idx=idx.astype(np.int64), u=u, paths=np.array(paths),
                        u_spacings=calls[0], M=M, ffbs_seed=FFBS_SEED, data_seed=int(g["data_seed"]),
                        run_seed=int(g["run_seed"]))
    print("ffbs_lg.npz: idx", idx.shape, "u", u.shape)


if __name__ == "__main__":
    main()
