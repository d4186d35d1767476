"""Every univariate model kind that runs only as a bootstrap filter (Gordon et al., ThetaLogistic, StochVolLeverage,
DiscreteCox) on every step form the plan chooses, against the oracle: the checks behind tests/test_model_matrix_emu.py
(emulator build) and tests/test_model_matrix_gpu.py (MI355X), in the manner of lazy_lw_cases.py.

One dispatch turns (kind, Feynman-Kac kind, slots, record shape) into a kernel instance, so every kind reaches every
form; a wrong time index or a wrong aux slot in ONE (kind, form) cell is self-consistent across the forms the other
tests compare with each other, and stays inside a z-test on the evidence.  Here every cell is a teacher-forced audit
(parity_cases.audit_history / audit_sqmc_history: every particle, every step, ancestors bit for bit), on the first T
observations of the model's own fixture -- DiscreteCox gets real counts.

No bound is set here: every tolerance is the audits' own, the strict cells and the history / no-history pairs use
equality."""
import numpy as np

import particles_amd as pa
import parity_cases as pc
from lazy_lw_cases import _Env
from oracle import smc_oracle as orc
from particles_amd import _lib
from particles_amd import resampling as rs
from particles_amd import state_space_models as ssm

T = 6
SEED = 5
MODELS = ("gordon", "theta", "svlev", "cox")

# cell -> N, scheme, ESSrmin, verification switches, replayed draws?, islands, audited island, smc_filter_describe.
# The smallest N that reaches each form: the one-workgroup filter (one wave; 1000 threads), the flat step (closed-form
# and multinomial), the two-level step wide and tile (SMC_NO_WIDE), the ragged tile at an odd N (k_propagate<.., RAGGED
# = 2>), the ragged wide step (RAGGED = 1, general counts), k_reduce2 in front, the one-pass spacings, islands, and the
# flat CDF above two tiles.
CELLS = {
    1: (100, "systematic", 0.5, {}, True, 1, 0, "k_filter_small"),
    2: (1000, "stratified", 0.9, {}, False, 1, 0, "k_filter_small"),
    3: (1000, "systematic", 0.9, {"SMC_NO_SMALL": "1"}, True, 1, 0, "k_ancestors<fused>+k_propagate"),
    4: (1000, "multinomial", 0.9, {"SMC_NO_SMALL": "1"}, False, 1, 0,
        "k_f_spacing_sums+k_f_spacing_scan+k_f_spacing_write+k_ancestors<fused>+k_propagate"),
    5: (2048, "systematic", 0.9, {}, True, 1, 0, "k_ancestors2w+k_propagate"),
    6: (4096, "systematic", 0.9, {"SMC_NO_WIDE": "1"}, False, 1, 0, "k_ancestors2+k_propagate"),
    7: (3001, "stratified", 0.9, {}, False, 1, 0, "k_ancestors2+k_propagate"),
    8: (3000, "systematic", 0.5, {}, True, 1, 0, "k_ancestors2w+k_propagate"),
    9: (2048, "stratified", 0.9, {"SMC_TWO_LEVEL_MID": "1"}, False, 1, 0, "k_reduce2+k_ancestors2+k_propagate"),
    10: (3000, "multinomial", 0.9, {}, False, 1, 0, "k_f_spacing_onepass<with k_reduce2>+k_ancestors2+k_propagate"),
    11: (2048, "systematic", 0.9, {}, False, 3, 2, "k_ancestors2w+k_propagate"),
    12: (3000, "systematic", 0.9, {"SMC_FLAT_CDF": "1"}, True, 1, 0, "k_ancestors<fused>+k_propagate"),
}
SKIP_CELLS = (1, 8)              # (ESSrmin 0.5: the cells that must hold a step which does not resample)
DEGENERATE_CELLS = (2, 5, 7, 10)            # one-workgroup, wide, ragged tile, multinomial

STRICT_SIZES = {1000: "k_strict_W+k_sqx_classify+k_sqx_fill+k_strict_search_S+k_propagate",
                3000: "k_strict_classify+k_strict_search+k_propagate"}
SQMC_TWO_LEVEL = "k_rs_sort+k_sq_permute+k_reduce2+k_ancestors2+k_propagate"
SQMC_FLAT = "k_rs_sort+k_sobol+k_sqmv_tapes+k_ancestors<fused>+k_sqmv_compose+k_propagate"

# model, y[2]: one particle keeps all the weight (ESS exactly 1.0, an evidence of -5e7 / -3e12) ...
ONE_SURVIVOR = (("gordon", 1e4), ("theta", 1e6))
# ... or none does: a count outside the support, a squared residual that overflows, a missing value
DEAD = (("cox", 2.5), ("gordon", 1e200), ("gordon", float("nan")))


def data(golden, model, T=T):
    y = np.squeeze(golden(model + "_boot")["y"])[:T]
    assert len(y) == T
    return [np.atleast_1d(np.asarray(v, dtype=float)) for v in y]


def skipped_then_resumed(r):
    """A step t >= 1 that does not resample, and a later one that does."""
    r = [bool(v) for v in r]
    return any(not r[t] and any(r[t + 1:]) for t in range(1, len(r)))


_RS = {}                # (model, cell) -> rs flags of the audited island


def numpy_tapes(N, T, scheme, seed):
    """Dense replay tapes (z, u) of one island, drawn as parity_cases.check_oracle_at_size draws them."""
    np.random.seed(seed)
    z = np.random.standard_normal((T, 1, N))
    u = np.random.rand(T, 1, 1 if scheme == "systematic" else N)
    if scheme == "multinomial":
        for t in range(T):
            u[t, 0] = orc.uniform_spacings_from(np.random.rand(N + 1))
    return z, u


def audit_moves(pf, mk_orc, y, scheme, ESSrmin, steps, z=None, u=None, exact=False, strict=False, tol=1e-12):
    """The steps of a history-keeping bootstrap run that parity_cases.audit_history cannot take, by its own rules and
    tolerances: the decision from the device's ESS, then
    strict: A_t equal to the reference's sequential fp64 CDF on exp_and_normalise(lw_{t-1}) -- no integer contract, no
    near-tie -- X, lw of every particle, and the summaries;
    otherwise (a step that kills every particle: ESS and evidence are NaN on both sides, which `abs(a / b - 1) < tol`
    cannot express): A_t bit for bit on the integer contract, X and lw; the caller checks the summaries."""
    N = pf.N
    model = mk_orc()
    ctx = orc.StepCtx(model, "bootstrap", y[0])
    two_level = "k_ancestors2" in pc.describe(pf)
    summ = pf._summ()[0]
    for t in steps:
        X, lw = pf._history(_lib.FIELD_X, t), pf._history(_lib.FIELD_LW, t)
        rs_flag = bool(summ[t, 4])
        Xp = lw_prev = None
        if t > 0:
            X_prev, lw_prev = pf._history(_lib.FIELD_X, t - 1), pf._history(_lib.FIELD_LW, t - 1)
            assert abs(summ[t - 1, 0] / orc.Weights(lw=lw_prev.copy()).ESS - 1) < 1e-11, t
            assert rs_flag == bool(summ[t - 1, 0] < N * ESSrmin), t
            Xp = X_prev
            if rs_flag:
                A = pf._history(_lib.FIELD_A, t)
                ut = np.asarray(u[t, 0]) if u is not None else (
                    pf._spacings(t, 0) if scheme == "multinomial" else orc.philox_resample_uniforms(pf.seed, scheme, N, t, 0))
                su = ut if scheme == "multinomial" else orc.sorted_uniforms(scheme, N, ut)
                if strict:
                    A_want = orc.inverse_cdf(su, orc.exp_and_normalise(lw_prev))
                elif two_level:
                    A_want, _ = orc.inverse_cdf_2level_c(scheme, ut, lw_prev)
                else:
                    A_want = orc.inverse_cdf_q62(su, pf._history(_lib.FIELD_W, t - 1))
                assert np.array_equal(A, A_want), (t, "A", int(np.sum(A != A_want)))
                Xp = X_prev[A]
        zt = np.asarray(z[t, 0]) if z is not None else orc.philox_normals(pf.seed, N, t, 0)
        Xo, inc = orc.propagate(model, "bootstrap", t, np.asarray(y[t]), Xp, zt, ctx)
        lwo = inc if (t == 0 or rs_flag) else lw_prev + inc
        lwo = np.where(np.isnan(lwo), -np.inf, lwo)
        if exact and z is not None:
            assert np.array_equal(X, Xo) and np.array_equal(lw, lwo), t
        else:
            assert np.allclose(X, Xo, rtol=tol, atol=tol), (t, "X", float(np.max(np.abs(X - Xo))))
            assert np.allclose(lw, lwo, rtol=100 * tol, atol=100 * tol), (t, "lw")
        if strict:
            w = orc.Weights(lw=lw.copy())
            assert abs(summ[t, 0] / w.ESS - 1) < 1e-10, (t, "ESS")
            assert abs(summ[t, 1] - w.log_mean) < 1e-11 * max(1.0, abs(w.log_mean)), (t, "log_mean")
            loglt = w.log_mean if (t == 0 or rs_flag) else w.log_mean - orc.Weights(lw=lw_prev.copy()).log_mean
            assert abs(summ[t, 2] - loglt) < 1e-10 * max(1.0, abs(loglt)), (t, "loglt")
            logLt = float(np.sum(summ[:t + 1, 2]))
            assert abs(summ[t, 3] - logLt) < 1e-10 * max(1.0, abs(logLt)), (t, "logLt")


def check_cell(golden, model, cell, y=None, inspect=None, tag=""):
    """What parity_cases.check_oracle_at_size does, on the fixture's data: the history-keeping run audited step by step
    (audit_history), the run without history (parity-slot launches, log-weight stores left out) pinned to it bit for
    bit."""
    N, scheme, ess, env, replay, n_islands, isl, want = CELLS[cell]
    mk_dev, mk_orc = pc.MODELS[model]
    y = data(golden, model) if y is None else y
    z, u = numpy_tapes(N, len(y), scheme, SEED) if replay else (None, None)
    with _Env(env):
        mk = lambda hist: pa.SMC(fk=ssm.Bootstrap(ssm=mk_dev(), data=y), N=N, resampling=scheme, ESSrmin=ess,
                                 replay=None if z is None else (z, u), store_history=hist, n_islands=n_islands,
                                 seed=SEED, collect="off")
        ph, pf = mk(True), mk(False)
    ph.run()
    assert pc.describe(ph) == want, (model, cell, pc.describe(ph))
    r = ph._summ()[isl, :, 4] != 0
    assert r[1:].any(), (model, cell, r.astype(int))
    if not tag:
        _RS[model, cell] = r
    if inspect is not None:
        inspect(ph)
    ties = pc.audit_history(ph, mk_orc, "bootstrap", y, scheme, ess, z=z, u=u, exact=model in pc.EXACT_MODELS, island=isl)
    pc.log_near_ties("%s cell %d%s N=%d %s %s" % (model, cell, tag, N, scheme, "replay" if replay else "philox"), ties,
                     int(np.sum(r)) * N)
    assert ties <= pc.near_tie_allowance(len(y) * N), ties
    pf.run()
    assert np.array_equal(pf._get(_lib.FIELD_X, isl), ph._get(_lib.FIELD_X, isl))
    assert np.array_equal(pf._get(_lib.FIELD_LW, isl), ph._get(_lib.FIELD_LW, isl))
    if ph._summ()[isl, -1, 4]:
        assert np.array_equal(pf._get(_lib.FIELD_A, isl), ph._get(_lib.FIELD_A, isl))
    assert np.array_equal(pf._summ(), ph._summ())
    return ties


def check_skipped_resampling(golden, model):
    """Per model, one of the ESSrmin = 0.5 cells has a step that does not resample followed by one that does: the
    evidence increment across a skipped resampling (log_mean_t - log_mean_{t-1}) is among what the cells audit."""
    for cell in SKIP_CELLS:
        if (model, cell) not in _RS:
            check_cell(golden, model, cell)
    assert any(skipped_then_resumed(_RS[model, c]) for c in SKIP_CELLS), \
        (model, [_RS[model, c].astype(int).tolist() for c in SKIP_CELLS])


def check_strict(golden, model, N):
    """strict_ancestors=True: at every resampling step A_t IS the reference's sequential fp64 CDF on
    exp_and_normalise(lw_{t-1}) -- equality, no near-tie allowance -- and X, lw of every particle as in the cells."""
    mk_dev, mk_orc = pc.MODELS[model]
    y = data(golden, model)
    pf = pa.SMC(fk=ssm.Bootstrap(ssm=mk_dev(), data=y), N=N, resampling="systematic", ESSrmin=0.9, seed=SEED,
                store_history=True, strict_ancestors=True, collect="off")
    pf.run()
    assert pc.describe(pf) == STRICT_SIZES[N], (model, N, pc.describe(pf))
    nres = int(np.sum(pf._summ()[0, :, 4] != 0))
    assert nres >= 1, (model, N)
    audit_moves(pf, mk_orc, y, "systematic", 0.9, range(T), strict=True)
    pc.log_near_ties("STRICT %s systematic N=%d philox: literal equality" % (model, N), 0, nres * N)


def _sqmc_run(model, y, N, hist, seed=47):
    pa.seed(seed)
    c0 = _lib._counter + 1
    pf = pa.SMC(fk=ssm.Bootstrap(ssm=pc.MODELS[model][0](), data=y), N=N, qmc=True, collect="off", store_history=hist)
    assert pf._fused and pc.describe(pf) == SQMC_TWO_LEVEL, (model, pc.describe(pf))
    pf.run()
    return pf, c0


def _sqmc_end(pf):
    return [np.asarray(pf.X).copy(), np.asarray(pf.A).copy(), np.asarray(pf.wgts.lw).copy(), pf._summ().copy()]


_SQMC_END = {}          # model -> end state of the run without history, default plan: computed once


def check_sqmc(golden, model, gather, N=2048):
    """The fused SQMC step (k_sq_permute<KIND, RECOMPUTE>): audit_sqmc_history on a history-keeping run, the run without
    history ends in the same state.  gather: the same with the sorted weights gathered through the permutation
    (SMC_SQ_GATHER: the other value of RECOMPUTE), and the same end state as the default plan's.  StochVolLeverage's
    weight needs the parent, so its plan never recomputes: both settings are one path, held to agree."""
    y = data(golden, model)
    mk_orc = pc.MODELS[model][1]
    mode = _lib.RNG_MODE[0]
    rs.set_rng("philox")
    try:
        if gather and model not in _SQMC_END:
            _SQMC_END[model] = _sqmc_end(_sqmc_run(model, y, N, False)[0])
        with _Env({"SMC_SQ_GATHER": "1"} if gather else {}):
            pf, c0 = _sqmc_run(model, y, N, True)
            pq, _ = _sqmc_run(model, y, N, False)
        if not (gather and model == "svlev"):
            ties = pc.audit_sqmc_history(pf, mk_orc, "bootstrap", y, 47, c0)
            assert ties <= pc.near_tie_allowance(T * N), ties
        assert np.array_equal(np.asarray(pq.X), np.asarray(pf.X)) and pq.logLt == pf.logLt, (model, gather)
        if gather:
            assert all(np.array_equal(a, b) for a, b in zip(_sqmc_end(pq), _SQMC_END[model])), model
        else:
            _SQMC_END[model] = _sqmc_end(pq)
    finally:
        rs.set_rng(mode)


def check_sqmc_flat(golden, model, N=256):
    """Below two tiles the flat step runs SQMC (no history slots): as parity_cases.check_sqmc_fused_small, the SAME run
    as the operator path on the same points -- both form the flat Q62 CDF of the sorted weights, so the ancestors are
    identical wherever the weights are; X bit for bit."""
    y = data(golden, model)
    mode = _lib.RNG_MODE[0]
    rs.set_rng("philox")
    try:
        runs = []
        for fused in (True, False):
            _lib.FUSED_SQMC[0] = fused
            pa.seed(31)
            pf = pa.SMC(fk=ssm.Bootstrap(ssm=pc.MODELS[model][0](), data=y), N=N, qmc=True, collect="off")
            assert pf._fused == fused
            if fused:
                assert pc.describe(pf) == SQMC_FLAT, pc.describe(pf)
            steps = []
            for t in range(T):
                next(pf)
                assert pf.rs_flag == (t > 0)
                steps.append((np.asarray(pf.X).copy(), None if t == 0 else np.asarray(pf.A).copy(),
                              np.asarray(pf.wgts.lw).copy(), float(pf.logLt)))
            runs.append(steps)
    finally:
        _lib.FUSED_SQMC[0] = True
        rs.set_rng(mode)
    for t in range(T):
        (Xa, Aa, la, La), (Xb, Ab, lb, Lb) = runs[0][t], runs[1][t]
        if model not in pc.EXACT_MODELS and Aa is not None and not np.array_equal(Aa, Ab):
            break                  # (weights that differ in their last bits move a near-tie: as for StochVol there)
        assert Aa is None or np.array_equal(Aa, Ab), (model, t)
        assert np.array_equal(Xa, Xb), (model, t)
        # (the fused kernels and the operators form the observation density by different expressions)
        assert np.array_equal(la, lb) if model in pc.EXACT_MODELS else np.allclose(la, lb, rtol=1e-13, atol=1e-13), (model, t)
        assert abs(La - Lb) < 1e-12 * max(1.0, abs(La)), (model, t)
    else:
        t = T
    assert t >= 2, (model, t)


def check_one_survivor(golden, model, bad, cell):
    """An observation that leaves ONE particle with all the weight: the next step gives every offspring to one parent
    (the heavy-parent list; the two-level CDF with all its mass in one tile).  The unchanged audit."""
    y = data(golden, model)
    y[2] = np.array([bad])

    def look(ph):
        isl = CELLS[cell][6]
        assert ph._summ()[isl, 2, 0] == 1.0, ph._summ()[isl, 2]
        assert ph._summ()[isl, 3, 4] != 0
        A = ph._history(_lib.FIELD_A, 3, isl)
        assert np.all(A == A[0]), np.unique(A)

    check_cell(golden, model, cell, y=y, inspect=look, tag=" y[2]=%g" % bad)


def check_dead_population(golden, model, bad, cell):
    """An observation that kills every particle.  The reference's semantics (core.py:181-183): every weight is -inf,
    ESS and log_mean are NaN, `ESS < N * ESSrmin` is False from then on: no later step resamples, logLt stays NaN,
    and the particles go on moving."""
    N, scheme, ess, env, replay, n_islands, isl, want = CELLS[cell]
    assert n_islands == 1
    mk_dev, mk_orc = pc.MODELS[model]
    y = data(golden, model)
    y[2] = np.array([bad])
    z, u = numpy_tapes(N, T, scheme, SEED) if replay else (None, None)
    with _Env(env):
        mk = lambda hist: pa.SMC(fk=ssm.Bootstrap(ssm=mk_dev(), data=y), N=N, resampling=scheme, ESSrmin=ess,
                                 replay=None if z is None else (z, u), store_history=hist, seed=SEED, collect="off")
        ph, pf = mk(True), mk(False)
    ph.run()
    assert pc.describe(ph) == want, pc.describe(ph)
    exact = model in pc.EXACT_MODELS
    ties = pc.audit_history(ph, mk_orc, "bootstrap", y, scheme, ess, z=z, u=u, exact=exact, steps=range(2))
    summ = ph._summ()[0]
    assert summ[2, 4] != 0, summ[:, 4]                    # (step 2 resamples the living; its weights then die)
    with np.errstate(over="ignore", invalid="ignore"):    # (the oracle's own (y - loc)^2 overflows at 1e200)
        audit_moves(ph, mk_orc, y, scheme, ess, range(2, 3), z=z, u=u, exact=exact)
    pc.log_near_ties("%s cell %d y[2]=%g: dead population" % (model, cell, bad), ties, int(np.sum(summ[:, 4])) * N)
    assert ties <= pc.near_tie_allowance(T * N), ties
    model_o = mk_orc()
    ctx = orc.StepCtx(model_o, "bootstrap", y[0])
    for t in range(2, T):
        assert np.all(np.isneginf(ph._history(_lib.FIELD_LW, t))), t
        assert np.all(np.isnan(summ[t, [0, 1, 3]])), (t, summ[t])
        if t == 2:
            continue
        assert summ[t, 4] == 0, (t, summ[:, 4])
        X, X_prev = ph._history(_lib.FIELD_X, t), ph._history(_lib.FIELD_X, t - 1)
        zt = np.asarray(z[t, 0]) if z is not None else orc.philox_normals(ph.seed, N, t, 0)
        Xo, _ = orc.propagate(model_o, "bootstrap", t, y[t], X_prev, zt, ctx)
        assert np.all(np.isfinite(X)), t
        if exact and z is not None:
            assert np.array_equal(X, Xo), (t, "X")
        else:
            assert np.allclose(X, Xo, rtol=1e-12, atol=1e-12), (t, "X", float(np.max(np.abs(X - Xo))))
    pf.run()
    assert np.array_equal(pf._get(_lib.FIELD_X), ph._get(_lib.FIELD_X))
    assert np.array_equal(pf._get(_lib.FIELD_LW), ph._get(_lib.FIELD_LW))
    assert np.array_equal(pf._summ(), ph._summ(), equal_nan=True)
