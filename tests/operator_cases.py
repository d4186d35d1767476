"""The operator path against NumPy: DeviceArray arithmetic (smc_elementwise), the distributions classes on device
arrays, X[A], X @ M (smc_rows_matmul), column / stack_columns (smc_copy_strided) and the Weights they feed -- every
op code, every operand form, and the refusals.  Written once and run twice: on an MI355X by tests/test_operators_gpu.py
and through the emulator build of the same kernel sources by tests/test_operators_emu.py, at the same sizes.

The spec is NumPy: in the reference these arrays are ndarrays.  IEEE operations (+ - * / neg abs sqrt square min max)
are compared bit for bit, signs of zero included (the sign of a NaN is left open: IEEE 754 does not define it for
arithmetic results).  The one documented difference: where minimum / maximum tie on +0 and -0 the device returns the
zero fmin / fmax pick, NumPy its first argument; those elements are compared by value (DESIGN, "What DeviceArray
broadcasts and what it refuses").

exp log cos sin arctan pow go through the device libm and are judged in ulps of a wider reference rounded to double:
numpy.longdouble where it is wider than double (x87: 64-bit significand), mpmath at 113 bits elsewhere, and mpmath
always for pow.  sin / cos: |x| <= 1e5, ulps where |want| >= 2^-10, absolute error in units of spacing(2^-10) closer to
a zero.  pow: base in (0, 1e3], exponent in [-20, 20].  Nobody had measured the device libm's fp64 error here, so the
bounds were not fixed in advance: LIBM_MEASURED is the largest error seen on an MI355X over libm_inputs() (seed
LIBM_SEED), LIBM_BOUND that value rounded up to a whole ulp plus one ulp.  The emulator run evaluates the same bounds
against the host libm.

    function   measured on MI355X (ulp)   asserted (ulp)
    exp        0.808                      2
    log        0.621                      2
    cos        0.730                      2
    sin        0.712                      2
    arctan     1.298                      3
    pow        1.164                      3

(All far inside the rtol = 1e-14, about 45 ulp, that check_resident_user_model asserts of the same functions.)

X @ M is one fma chain of length d per output, so its bound is derived, not measured:
|err_ij| <= gamma_d * sum_l |x_il m_lj| with gamma_d = d 2^-53 / (1 - d 2^-53) (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., section 3.1; an fma chain satisfies the bound of the plain recursive sum of products).
"""
import math

import mpmath
import numpy as np
import pytest
import scipy.special as sps

import particles_amd as pa
from oracle import smc_oracle as orc
from particles_amd import _lib
from particles_amd._lib import DeviceArray as DA
from particles_amd import distributions as dists
from particles_amd import resampling as rs

SIZES_1D = (1, 2, 255, 256, 257, 513, 1000)
SHAPES_2D = ((1, 1), (3, 3), (100, 7), (257, 5), (64, 64))

LIBM_SEED = 20240611
LIBM_MEASURED = {"exp": 0.808, "log": 0.621, "cos": 0.730, "sin": 0.712, "arctan": 1.298, "pow": 1.164}
LIBM_BOUND = {fn: math.ceil(e) + 1.0 for fn, e in LIBM_MEASURED.items()}      # exp log cos sin: 2, arctan pow: 3
RTOL_FLOOR_ULP = 1e-14 / 2.0 ** -52              # no bound may be looser than rtol = 1e-14 (45 ulp at the least)

LD_IS_WIDER = np.finfo(np.longdouble).nmant > 52
REFERENCE_USED = "numpy.longdouble (%d-bit significand)" % (np.finfo(np.longdouble).nmant + 1) if LD_IS_WIDER \
    else "mpmath at 113 bits (long double is no wider than double here)"

# +-0, +-inf, NaN, the smallest subnormal, (about) the smallest normal, (about) the largest finite, +-1, negatives and a
# fraction (log / sqrt / pow of a negative; pow with a fractional exponent)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 2.2e-308, 1.797e308, 1.0, -1.0, -2.5, -8.0, 0.5,
                     1.0 / 3.0])
PAIR_A = np.repeat(SPECIALS, SPECIALS.size)     # every special meets every special: element i * S + j is (S[i], S[j])
PAIR_B = np.tile(SPECIALS, SPECIALS.size)


def operands(n, seed=0):
    """Two (n,) operands: a seeded random part, then the block of special pairs (as much of it as fits)."""
    rng = np.random.default_rng(1000 + seed + n)
    m = min(n, PAIR_A.size)
    a = np.concatenate([rng.standard_normal(n - m) * 3.0, PAIR_A[:m]])
    b = np.concatenate([rng.standard_normal(n - m) * 3.0 + 0.5, PAIR_B[:m]])
    return a, b


def same(got, want, value_only=None, what=""):
    """Bit-for-bit agreement with NumPy: shape, values (NaN where NaN), and the sign of every non-NaN element --
    but for the elements of the mask ``value_only``."""
    got = got.get() if isinstance(got, DA) else np.asarray(got)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (what, np.flatnonzero(bad.reshape(-1))[:5], got[bad][:5], want[bad][:5])
    sign = (np.signbit(got) != np.signbit(want)) & ~np.isnan(want)
    if value_only is not None:
        sign &= ~value_only
    assert not sign.any(), (what, "sign of zero", np.flatnonzero(sign.reshape(-1))[:5])


def zero_tie(a, b):
    a, b = np.broadcast_arrays(a, b)
    return (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))


# ---------------------------------------------------------------- the IEEE-exact op codes ----
# numpy's own expression for each binary op code: (code, reference of _ew(code, y) on x)
EXACT_BINARY = {"add": lambda x, y: x + y, "sub": lambda x, y: x - y, "mul": lambda x, y: x * y,
                "div": lambda x, y: x / y, "rsub": lambda x, y: y - x, "rdiv": lambda x, y: y / x,
                "min": np.minimum, "max": np.maximum}
EXACT_UNARY = {"neg": np.negative, "abs": np.abs, "sqrt": np.sqrt, "square": np.square}
ARITH = (("add", np.add, lambda x, y: x + y), ("sub", np.subtract, lambda x, y: x - y),
         ("mul", np.multiply, lambda x, y: x * y), ("div", np.true_divide, lambda x, y: x / y))
SCALARS = (0.0, -0.0, np.inf, np.nan, 5e-324, -2.5, 1.797e308)


def check_op_table():
    """The 18 op codes of the kernel's enum, all of them covered below."""
    assert sorted(DA._EW.values()) == list(range(18))
    covered = set(EXACT_BINARY) | set(EXACT_UNARY) | {"exp", "log", "cos", "sin", "arctan", "pow"}
    assert covered == set(DA._EW)


def check_elementwise_exact(n):
    """Same-size and scalar operands of length n, each op through every way DeviceArray exposes it."""
    ah, bh = operands(n)
    a, b = DA.from_numpy(ah), DA.from_numpy(bh)
    with np.errstate(all="ignore"):
        for name, ref in EXACT_BINARY.items():                          # every code, as _ew takes it
            tie = zero_tie(ah, bh) if name in ("min", "max") else None
            same(a._ew(name, b), ref(ah, bh), tie, name)
        for name, uf, op in ARITH:
            want = op(ah, bh)
            same(op(a, b), want, None, name + ": operator")
            same(op(a, bh), want, None, name + ": host array on the right")
            same(op(ah, b), want, None, name + ": host array on the left")
            same(uf(a, b), want, None, name + ": ufunc")
            same(uf(ah, b), want, None, name + ": ufunc, host array on the left")
            same(uf(a, bh), want, None, name + ": ufunc, host array on the right")
            for s in SCALARS:
                same(op(a, s), op(ah, s), None, name + ": scalar %r" % s)
                same(op(s, a), op(s, ah), None, name + ": python float %r on the left" % s)
                same(op(np.float64(s), a), op(np.float64(s), ah), None, name + ": np.float64 %r on the left" % s)
                same(uf(a, s), uf(ah, s), None, name + ": ufunc, scalar")
                same(uf(s, a), uf(s, ah), None, name + ": ufunc, scalar on the left")
        for uf in (np.minimum, np.maximum):
            same(uf(a, b), uf(ah, bh), zero_tie(ah, bh), uf.__name__)
            same(uf(ah, b), uf(ah, bh), zero_tie(ah, bh), uf.__name__ + ": host array on the left")
            for s in SCALARS:
                same(uf(a, s), uf(ah, s), zero_tie(ah, s), uf.__name__ + ": scalar")
                same(uf(np.float64(s), a), uf(s, ah), zero_tie(ah, s), uf.__name__ + ": np.float64 on the left")
            got = uf(a, b).get()
            assert np.all(np.isnan(got[np.isnan(ah) | np.isnan(bh)])), "NaN wherever either side is NaN"
            assert np.all(np.isnan(uf(a, np.nan).get()))
        for name, uf in EXACT_UNARY.items():
            same(a._ew(name), uf(ah), None, name)
            same(uf(a), uf(ah), None, name + ": ufunc")
        same(-a, -ah, None, "-x")
        same(abs(a), abs(ah), None, "abs(x)")
        same(np.fabs(a), np.fabs(ah), None, "fabs")
        same(np.divide(a, b), ah / bh, None, "np.divide")
        same(a ** 2, ah * ah, None, "x ** 2 is x * x")
        same(a ** 0.5, np.sqrt(ah), None, "x ** 0.5 is sqrt(x)")


def check_elementwise_forms(shape):
    """The six operand forms of _ew on an (N, d) array: same size, scalar alpha, a (1,) device array on the right
    (sb = 0) and on the left (sa = 0: the result takes the other operand's shape), a (d,) row on the right (sb = -d)
    and on the left (sa = -d).  The row holds specials, the rows of X hold every special in every column."""
    N, d = shape
    rng = np.random.default_rng(7 + N * d)
    S = SPECIALS.size
    Xh = rng.standard_normal((N, d)) * 2.0
    k = min(N, S)
    Xh[N - k:, :] = SPECIALS[:k, None]                      # the last rows: one special per row, in every column
    rowh = np.resize(SPECIALS, d)
    if d > S:
        rowh[S:] = rng.standard_normal(d - S)
    Yh = rng.standard_normal((N, d)) + 0.5
    X, row, Y = DA.from_numpy(Xh), DA.from_numpy(rowh), DA.from_numpy(Yh)
    row2 = DA.from_numpy(rowh.reshape(1, d))
    with np.errstate(all="ignore"):
        for name, ref in EXACT_BINARY.items():
            mm = name in ("min", "max")
            same(X._ew(name, Y), ref(Xh, Yh), None, name + ": same size")
            same(X._ew(name, row), ref(Xh, rowh), zero_tie(Xh, rowh) if mm else None, name + ": (N,d) with a row")
            same(row._ew(name, X), ref(rowh, Xh), zero_tie(Xh, rowh) if mm else None, name + ": a row with (N,d)")
            same(X._ew(name, row2), ref(Xh, rowh.reshape(1, d)), zero_tie(Xh, rowh) if mm else None,
                 name + ": (N,d) with a (1,d) row")
            same(X._ew(name, rowh), ref(Xh, rowh), zero_tie(Xh, rowh) if mm else None, name + ": a host row")
            for s in (-2.5, 0.0, np.inf, np.nan):
                one = DA.from_numpy(np.array([s]))
                tie = zero_tie(Xh, s) if mm else None
                same(X._ew(name, s), ref(Xh, s), tie, name + ": alpha")
                same(X._ew(name, one), ref(Xh, np.array([s])), tie, name + ": (1,) on the right")
                same(one._ew(name, X), ref(np.array([s]), Xh), tie, name + ": (1,) on the left")
        for name, uf, op in ARITH:                              # the same forms through the operators and ufuncs
            same(op(X, row), op(Xh, rowh), None, name)
            same(op(row, X), op(rowh, Xh), None, name)
            same(op(rowh, X), op(rowh, Xh), None, name + ": host row on the left")
            same(uf(row, X), op(rowh, Xh), None, name + ": ufunc")
            same(op(2.0, X), op(2.0, Xh), None, name + ": float on the left")
        for name, uf in EXACT_UNARY.items():
            same(uf(X), uf(Xh), None, name)
        # pow in the row forms: the specials' non-finite results and signs exactly, finite ones within the bound
        pow_agrees(X ** row, Xh, rowh, "pow: (N,d) ** row")
        pow_agrees(row ** X, rowh, Xh, "pow: row ** (N,d)")
        pow_agrees(X ** rowh, Xh, rowh, "pow: (N,d) ** host row")
        pow_agrees(np.power(X, row2), Xh, rowh.reshape(1, d), "np.power")


# ---------------------------------------------------------------- the device libm ----
def libm_inputs():
    """The inputs the libm bounds were measured over: per function a seeded random vector in the stated range and
    the specials.  pow: (base, exponent), the special pairs among them."""
    rng = np.random.default_rng(LIBM_SEED)
    n = 6000
    sp = SPECIALS
    trig = np.concatenate([rng.uniform(-1e5, 1e5, n), rng.uniform(-4.0, 4.0, n),
                           (np.arange(1, 400) * (np.pi / 2)), rng.standard_normal(200) * 1e-3, sp])
    trig = np.where(np.abs(trig) <= 1e5, trig, np.sign(trig))            # |x| <= 1e5 (NaN, +-inf -> +-1, NaN)
    trig = np.concatenate([trig, [np.inf, -np.inf, np.nan]])
    base = np.concatenate([rng.uniform(0.0, 1e3, n), np.exp(rng.uniform(-12.0, np.log(1e3), n))])
    base = np.where(base > 0.0, base, 1.0)
    expo = rng.uniform(-20.0, 20.0, base.size)
    expo[::7] = np.rint(expo[::7])
    return {
        "exp": np.concatenate([rng.uniform(-745.2, 709.8, n), rng.standard_normal(n) * 3.0, sp]),
        "log": np.concatenate([np.exp(rng.uniform(-708.0, 709.0, n)), rng.uniform(0.5, 2.0, n),
                               rng.uniform(0.0, 5e-308, 500), sp]),
        "cos": trig, "sin": trig,
        "arctan": np.concatenate([rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n), sp]),
        "pow": (np.concatenate([base, PAIR_A]), np.concatenate([expo, PAIR_B])),
    }


def _mp_round(v):
    """mpmath value -> the nearest double"""
    try:
        return float(v)
    except OverflowError:
        return math.copysign(math.inf, v)


def wide_reference(fn, x):
    """fn(x) in the wider format: a long double array, or a list of mpmath values (finite inputs only; the others
    are taken from NumPy, whose non-finite cases are C99's)."""
    if LD_IS_WIDER:
        with np.errstate(all="ignore"):
            return getattr(np, fn)(x.astype(np.longdouble))
    mpmath.mp.prec = 113
    f = {"exp": mpmath.exp, "log": mpmath.log, "cos": mpmath.cos, "sin": mpmath.sin, "arctan": mpmath.atan}[fn]
    with np.errstate(all="ignore"):
        out = getattr(np, fn)(x).astype(object)
    for i, v in enumerate(x):
        if np.isfinite(v) and np.isfinite(out[i]) and out[i] != 0.0:
            out[i] = f(mpmath.mpf(float(v)))
        elif np.isinf(v) and fn == "arctan":
            out[i] = mpmath.sign(v) * mpmath.pi / 2
    return out


def ulp_errors(got, ref, near_zero_floor=None):
    """|got - ref| in ulps of ref rounded to double (ref: long doubles or mpmath values).  Non-finite and NaN
    references must be met exactly.  Returns the largest error over the finite ones."""
    if ref.dtype == object:
        want = np.array([_mp_round(v) for v in ref], dtype=np.float64)
    else:
        with np.errstate(all="ignore"):
            want = ref.astype(np.float64)
    nf = ~np.isfinite(want)
    assert np.array_equal(got[nf], want[nf], equal_nan=True), ("non-finite results", got[nf][:8], want[nf][:8])
    assert np.all(np.isfinite(got[~nf])), "a finite result came back non-finite"
    f = ~nf
    if ref.dtype == object:                                         # (a value NumPy defines exactly: pow(NaN, 0) = 1)
        exact = np.array([not isinstance(v, mpmath.mpf) for v in ref]) & f
        assert np.array_equal(got[exact], want[exact]), ("exact results", got[exact][:8], want[exact][:8])
    unit = np.spacing(np.abs(want[f]))
    if near_zero_floor is not None:
        unit = np.maximum(unit, np.spacing(near_zero_floor))
    if ref.dtype == object:
        err = np.array([abs(mpmath.mpf(float(g)) - r) / mpmath.mpf(float(u))
                        for g, r, u in zip(got[f], ref[f], unit)], dtype=np.float64)
    else:
        err = (np.abs(got[f].astype(np.longdouble) - ref[f]) / unit.astype(np.longdouble)).astype(np.float64)
    return float(err.max()) if err.size else 0.0


def pow_reference(a, b):
    """a ** b as an object array: mpmath values where the result is finite, NumPy's (C99's) value elsewhere."""
    mpmath.mp.prec = 113
    a, b = (np.array(v, dtype=np.float64).reshape(-1) for v in np.broadcast_arrays(a, b))
    with np.errstate(all="ignore"):
        w = np.power(a, b)
    out = w.astype(object)
    for i in range(a.size):
        if np.isfinite(w[i]) and w[i] != 0.0 and np.isfinite(a[i]) and np.isfinite(b[i]) and a[i] != 0.0:
            out[i] = mpmath.power(mpmath.mpf(float(a[i])), mpmath.mpf(float(b[i])))
            assert not isinstance(out[i], mpmath.mpc)
    return out


def pow_agrees(got, a, b, what):
    got = got.get()
    assert got.shape == np.broadcast(a, b).shape, what
    err = ulp_errors(got.reshape(-1), pow_reference(a, b))
    with np.errstate(all="ignore"):
        w = np.power(*np.broadcast_arrays(a, b))
    z = w == 0.0
    assert np.array_equal(np.signbit(got[z]), np.signbit(w[z])), what
    assert err <= LIBM_BOUND["pow"], (what, err)


def libm_errors():
    """fn -> the largest error (ulp) of the device's exp log cos sin arctan pow over libm_inputs()."""
    inp = libm_inputs()
    out = {}
    for fn in ("exp", "log", "cos", "sin", "arctan"):
        x = inp[fn]
        got = getattr(np, fn)(DA.from_numpy(x)).get()
        floor = 2.0 ** -10 if fn in ("sin", "cos") else None
        out[fn] = ulp_errors(got, wide_reference(fn, x), floor)
        with np.errstate(all="ignore"):
            w = getattr(np, fn)(x)
        z = w == 0.0
        assert np.array_equal(np.signbit(got[z]), np.signbit(w[z])), fn
    a, b = inp["pow"]
    got = (DA.from_numpy(a) ** DA.from_numpy(b)).get()
    out["pow"] = ulp_errors(got, pow_reference(a, b))
    return out


def check_libm():
    """The six libm functions within the bounds of the table at the top, non-finite results exactly."""
    err = libm_errors()
    print("operator libm errors (ulp) against %s: %s" % (REFERENCE_USED, err))
    for fn, e in err.items():
        assert LIBM_BOUND[fn] <= RTOL_FLOOR_ULP
        assert e <= LIBM_BOUND[fn], (fn, e, LIBM_BOUND[fn])
    # the named cases
    x = DA.from_numpy(np.array([0.0, -1.0, np.nan, -8.0, 0.0, 1e308]))
    e = DA.from_numpy(np.array([1.0, 1.0, 0.0, 1.0 / 3.0, -1.0, 2.0]))
    lg = np.log(x).get()
    assert lg[0] == -np.inf and np.isnan(lg[1])
    pw = (x ** e).get()
    assert pw[2] == 1.0 and np.isnan(pw[3]) and pw[4] == np.inf and pw[5] == np.inf
    assert np.exp(DA.from_numpy(np.array([710.0]))).get()[0] == np.inf


def check_pow_routes():
    """x ** 2 and x ** 0.5 are x * x and sqrt(x) bit for bit (check_elementwise_exact); every other exponent is
    EW_POW: 3, -1, np.float64(2) (numpy squares there too: a correctly rounded x * x is inside pow's bound), and an
    array exponent on the device or the host.  What DeviceArray does not define raises TypeError."""
    rng = np.random.default_rng(3)
    xh = np.concatenate([rng.uniform(0.0, 1e3, 257), SPECIALS])
    eh = np.concatenate([rng.uniform(-20.0, 20.0, 257), SPECIALS[::-1]])
    x, e = DA.from_numpy(xh), DA.from_numpy(eh)
    for p in (3, -1, np.float64(2), 1.7, -0.5, 0):
        pow_agrees(x ** p, xh, float(p), "x ** %r" % p)
        pow_agrees(np.power(x, p), xh, float(p), "np.power(x, %r)" % p)
    pow_agrees(x ** e, xh, eh, "x ** device array")
    pow_agrees(x ** eh, xh, eh, "x ** host array")
    pow_agrees(np.power(x, e), xh, eh, "np.power(x, device array)")
    pow_agrees(x._ew("pow", e), xh, eh, "_ew('pow')")
    one = DA.from_numpy(np.array([2.0]))
    pow_agrees(one ** e, np.array([2.0]), eh, "(1,) ** array")
    pow_agrees(x ** one, xh, np.array([2.0]), "array ** (1,)")
    for bad in (lambda: 2.0 ** x, lambda: np.float64(2.0) ** x, lambda: np.tanh(x), lambda: np.power(xh, x),
                lambda: np.arctan2(x, x), lambda: np.add(x, x, out=None, where=True), lambda: np.add.reduce(x)):
        with pytest.raises(TypeError):
            bad()


def check_elementwise_c_level():
    """smc_elementwise itself: n = 0 is SMC_OK and writes nothing; an unknown op and a stride of 2 are refused."""
    L, h = _lib.lib(), _lib.ctx().h
    a = DA.from_numpy(np.arange(8.0))
    poison = np.full(8, -777.25)
    out = DA.from_numpy(poison)
    assert L.smc_elementwise(h, 0, a.ptr, 1, a.ptr, 1, 0.0, 0, out.ptr) == 0
    assert L.smc_elementwise(h, 0, a.ptr, 1, a.ptr, 1, 0.0, -3, out.ptr) == 0
    assert np.array_equal(out.get(), poison)
    for op, sa, sb in ((-1, 1, 1), (18, 1, 1), (0, 2, 1), (0, 1, 2)):
        with pytest.raises(ValueError):
            _lib.check(L.smc_elementwise(h, op, a.ptr, sa, a.ptr, sb, 0.0, 4, out.ptr))
    assert np.array_equal(out.get(), poison)
    for op in range(18):                                                # all 18 codes are launched
        _lib.check(L.smc_elementwise(h, op, a.ptr, 1, a.ptr, 1, 0.0, 8, out.ptr))
    with np.errstate(all="ignore"):
        assert np.array_equal(out.get(), np.arctan(np.arange(8.0)))


# ---------------------------------------------------------------- distributions ----
KINDS = ("scalar", "host1", "hostN", "dev1", "devN")


def as_kind(kind, v):
    """(the value as the distribution takes it, its host array) for an (N,) vector v."""
    if kind == "scalar":
        return float(v[0]), v[:1]
    if kind == "host1":
        return v[:1].copy(), v[:1]
    if kind == "hostN":
        return v.copy(), v
    if kind == "dev1":
        return DA.from_numpy(v[:1]), v[:1]
    return DA.from_numpy(v), v


def _is_dev(*kinds):
    return any(k.startswith("dev") for k in kinds)


def norm_logpdf_ld(x, loc, scale):
    """scipy.stats.norm.logpdf's formula (distributions.py:273-274) in long double, rounded to double."""
    x, loc, scale = (np.asarray(v, dtype=np.longdouble) for v in (x, loc, scale))
    y = (x - loc) / scale
    c = np.log(np.sqrt(2.0 * np.arctan(np.longdouble(1.0)) * 4.0))
    return (-y * y / 2.0 - c - np.log(scale)).astype(np.float64)


def check_normal(N):
    """Normal.logpdf / ppf / rvs(z=...) with the argument, loc and scale each a Python scalar, a host (1,) or (N,)
    array, a device (1,) or (N,) array: all 125 combinations.  Odd N and N = 1 end k_normal_rvs on a half pair."""
    rng = np.random.default_rng(40 + N)
    xv, lv, sv = rng.standard_normal(N) * 2.0, rng.standard_normal(N), rng.random(N) + 0.3
    uv, zv = rng.random(N) * 0.998 + 0.001, rng.standard_normal(N)
    assert not _lib.RESIDENT[0]
    for ka in KINDS:
        for kl in KINDS:
            for ks in KINDS:
                what = (N, ka, kl, ks)
                loc, lh = as_kind(kl, lv)
                sc, sh = as_kind(ks, sv)
                d = dists.Normal(loc=loc, scale=sc)
                dev = _is_dev(ka, kl, ks)
                for fn, arg in (("logpdf", xv), ("ppf", uv)):
                    a, ah = as_kind(ka, arg)
                    got = getattr(d, fn)(a)
                    assert isinstance(got, DA) == dev and isinstance(got, (DA, np.ndarray)), what
                    got = np.asarray(got)
                    ref = norm_logpdf_ld(ah, lh, sh) if fn == "logpdf" else sps.ndtri(ah) * sh + lh
                    assert got.shape == (max(ah.size, lh.size, sh.size),), what
                    assert np.max(np.abs(got - ref) / (1.0 + np.abs(ref))) < 1e-14, (fn, what)
                z, zh = as_kind(ka, zv)
                n = zh.size                                        # rvs(size = what z holds)
                if lh.size in (1, n) and sh.size in (1, n):
                    got = d.rvs(size=n, z=z)
                    assert isinstance(got, DA) == dev, what
                    assert np.array_equal(np.asarray(got), lh + sh * zh), what       # loc + scale * z, bit for bit
                else:
                    with pytest.raises(ValueError):
                        d.rvs(size=n, z=z)
                n = max(lh.size, sh.size)                          # rvs(size=None): the parameters' size
                if zh.size == n:
                    got = d.rvs(z=z)
                    assert isinstance(got, DA) == dev, what
                    assert np.array_equal(np.asarray(got).reshape(-1), lh + sh * zh), what
                else:
                    with pytest.raises(ValueError):
                        d.rvs(z=z)
    # return types: a scalar for rvs() of all-scalar parameters, device arrays for host inputs once resident
    r = dists.Normal(loc=1.0, scale=2.0).rvs(z=np.array([0.25]))
    assert np.ndim(r) == 0 and r == 1.5
    assert np.ndim(dists.Normal(loc=1.0, scale=2.0).rvs()) == 0
    pa.set_resident(True)
    try:
        d = dists.Normal(loc=lv, scale=0.5)
        for got in (d.logpdf(xv), d.ppf(uv), d.rvs(size=N, z=zv), d.rvs(size=N)):
            assert isinstance(got, DA) and got.shape == (N,)
        assert np.array_equal(d.rvs(size=N, z=zv).get(), lv + 0.5 * zv)
    finally:
        pa.set_resident(False)


def check_normal_philox(N, seed=977):
    """set_rng('philox'), z = None: loc + scale * the documented Philox normals of the call's counter."""
    rng = np.random.default_rng(N)
    lv = rng.standard_normal(N)
    mode = _lib.RNG_MODE[0]
    rs.set_rng("philox")
    try:
        for loc in (lv, DA.from_numpy(lv)):
            pa.seed(seed)
            for rep in range(2):
                counter = _lib._counter + 1                         # (the sub-stream the next stand-alone draw takes)
                got = dists.Normal(loc=loc, scale=0.7).rvs(size=N)
                assert _lib._counter == counter
                assert isinstance(got, DA) == isinstance(loc, DA)
                want = lv + 0.7 * orc.philox_normals(seed, N, counter)
                assert np.max(np.abs(np.asarray(got) - want)) < 1e-13, (N, rep)
    finally:
        rs.set_rng(mode)


def check_poisson(N):
    """Poisson.logpdf with k a scalar, a host (N,) or a float64 device (N,) array against a scalar, host or device
    rate, against the oracle's restatement of scipy's expression."""
    rng = np.random.default_rng(50 + N)
    kv = rng.poisson(4.0, N).astype(np.float64)
    kv[0] = 0.0
    rv = np.exp(rng.standard_normal(N))
    for kk in ("scalar", "hostN", "devN"):
        for kr in ("scalar", "hostN", "devN"):
            k, kh = as_kind(kk, kv if kk != "scalar" else np.array([3.0]))
            r, rh = as_kind(kr, rv)
            got = dists.Poisson(rate=r).logpdf(k)
            assert isinstance(got, DA) == _is_dev(kk, kr), (kk, kr)
            ref = orc.poisson_logpmf(kh, rh)
            assert np.max(np.abs(np.asarray(got) - ref) / (1.0 + np.abs(ref))) < 1e-14, (N, kk, kr)
    got = dists.Poisson(rate=rv).logpdf(kv.astype(np.int64))          # host counts are integers in the reference
    ref = orc.poisson_logpmf(kv, rv)
    assert np.max(np.abs(got - ref) / (1.0 + np.abs(ref))) < 1e-14


def spd(d, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d))
    return A @ A.T + d * np.eye(d)                                   # full, not diagonal


def check_mvnormal(d, N):
    """MvNormal.logpdf / rvs(z=...) / ppf with a full covariance: loc a scalar, (d,) or (N, d), x (d,) or (N, d),
    each on the host or the device, against the oracle within check_mvn_large's bounds."""
    rng = np.random.default_rng(60 + 7 * d + N)
    cov = spd(d, d)
    L = np.linalg.cholesky(cov)
    scale = 1.3
    locN, xN, zN = rng.standard_normal((N, d)), rng.standard_normal((N, d)) * 2.0, rng.standard_normal((N, d))
    uN = rng.random((N, d)) * 0.998 + 0.001
    locs = [(0.5, np.full(d, 0.5), False), (locN[0].copy(), locN[0], False), (locN.copy(), locN, False),
            (DA.from_numpy(locN[0]), locN[0], True), (DA.from_numpy(locN), locN, True)]
    xs = [(xN[0].copy(), xN[0], False), (xN.copy(), xN, False), (DA.from_numpy(xN[0]), xN[0], True),
          (DA.from_numpy(xN), xN, True)]
    for loc, lh, ldev in locs:
        mv = dists.MvNormal(loc=loc, scale=scale, cov=cov)
        for x, xh, xdev in xs:
            got = mv.logpdf(x)
            assert isinstance(got, DA) == (ldev or xdev)
            want = np.atleast_1d(orc.mvnormal_logpdf(np.atleast_2d(xh), lh, scale, L))
            got = np.asarray(got)
            assert got.shape == want.shape and want.shape == (N if (xh.ndim == 2 or lh.ndim == 2) else 1,), (d, N)
            assert orc_rel(got, want) < 1e-11, (d, N, lh.shape, xh.shape)
        for z, zdev in ((zN.copy(), False), (DA.from_numpy(zN), True)):
            got = mv.rvs(size=N, z=z)
            assert isinstance(got, DA) == (ldev or zdev) and got.shape == (N, d)
            assert np.max(np.abs(np.asarray(got) - orc.mvnormal_rvs(lh, scale, L, zN))) < 1e-12, (d, N)
        for u, udev in ((uN.copy(), False), (DA.from_numpy(uN), True)):
            got = mv.ppf(u)
            assert isinstance(got, DA) == (ldev or udev) and got.shape == (N, d)
            assert np.max(np.abs(np.asarray(got) - orc.mvnormal_rvs(lh, scale, L, sps.ndtri(uN)))) < 1e-12, (d, N)


def orc_rel(a, b):
    den = np.maximum(np.abs(b), 1e-300)
    return float(np.max(np.abs(a - b) / den))


def check_mvnormal_refused():
    mv = dists.MvNormal(loc=np.zeros(65), cov=spd(65, 1))
    with pytest.raises(ValueError):
        mv.logpdf(np.zeros((3, 65)))
    with pytest.raises(ValueError):
        mv.rvs(size=3, z=np.zeros((3, 65)))


def check_indep_prod():
    """IndepProd of three Normals: ppf and logpdf on a host and a device (257, 3), column by column."""
    rng = np.random.default_rng(70)
    par = ((1.0, 2.0), (0.0, 1.0), (-0.5, 0.5))
    d = dists.IndepProd(*[dists.Normal(loc=m, scale=s) for m, s in par])
    xh, uh = rng.standard_normal((257, 3)) * 2.0, rng.random((257, 3)) * 0.998 + 0.001
    want_lp = sum(norm_logpdf_ld(xh[:, i], m, s) for i, (m, s) in enumerate(par))
    want_q = np.stack([sps.ndtri(uh[:, i]) * s + m for i, (m, s) in enumerate(par)], axis=1)
    for dev in (False, True):
        x, u = (DA.from_numpy(xh), DA.from_numpy(uh)) if dev else (xh, uh)
        lp, q = d.logpdf(x), d.ppf(u)
        assert isinstance(lp, DA) == dev and isinstance(q, DA) == dev
        lp, q = np.asarray(lp), np.asarray(q)
        assert lp.shape == (257,) and q.shape == (257, 3)
        assert np.max(np.abs(lp - want_lp) / (1.0 + np.abs(want_lp))) < 3e-14      # (a sum of three terms of 1e-14)
        assert np.max(np.abs(q - want_q) / (1.0 + np.abs(want_q))) < 1e-14


# ---------------------------------------------------------------- rows and columns ----
def check_matmul(N, d, k):
    """X @ M and np.dot(X, M) against the long double product within the derived bound gamma_d sum |x| |m|."""
    rng = np.random.default_rng(80 + N + 64 * d + k)
    Xh = rng.standard_normal((N, d)) * 10.0 ** rng.integers(-3, 4, (N, d))
    Mh = rng.standard_normal((d, k))
    X = DA.from_numpy(Xh)
    if LD_IS_WIDER:
        want = (Xh.astype(np.longdouble)[:, :, None] * Mh.astype(np.longdouble)[None, :, :]).sum(axis=1)
    else:
        mpmath.mp.prec = 113
        want = np.array([[float(mpmath.fdot(Xh[i].tolist(), Mh[:, j].tolist())) for j in range(k)] for i in range(N)])
    gamma = d * 2.0 ** -53 / (1.0 - d * 2.0 ** -53)
    bound = gamma * (np.abs(Xh) @ np.abs(Mh))
    for got in (X @ Mh, np.dot(X, Mh)):
        assert isinstance(got, DA) and got.shape == (N, k)
        err = np.abs(got.get().astype(np.longdouble) - want).astype(np.float64)
        assert np.all(err <= bound), (N, d, k, float(np.max(err / np.maximum(bound, 1e-300))))


def check_matmul_edges():
    rng = np.random.default_rng(81)
    xh, Mh = rng.standard_normal(257), rng.standard_normal((1, 5))
    got = DA.from_numpy(xh) @ Mh                                     # a 1-D (257,) array is 257 rows of one
    assert got.shape == (257, 5) and np.array_equal(got.get(), xh[:, None] * Mh)
    X = DA.from_numpy(rng.standard_normal((4, 65)))
    with pytest.raises(ValueError):
        X @ np.zeros((65, 2))                                        # d = 65
    X = DA.from_numpy(rng.standard_normal((4, 3)))
    with pytest.raises(ValueError):
        X @ np.zeros((3, 65))                                        # k = 65
    with pytest.raises(ValueError):
        X @ np.zeros((4, 3))                                         # rows of M != d
    with pytest.raises(ValueError):
        np.dot(X, np.zeros(3))                                       # M must be 2-D
    with pytest.raises(TypeError):
        DA.from_numpy(np.arange(12).reshape(4, 3)) @ np.zeros((3, 2))


def check_columns(shape):
    """column(i), x[..., i], x[:, i] for every i in [-d, d); stack_columns / np.stack rebuild the array."""
    N, d = shape
    rng = np.random.default_rng(90 + N + d)
    Xh = rng.standard_normal((N, d))
    Xh.reshape(-1)[:: 5] = np.resize(SPECIALS, Xh.reshape(-1)[:: 5].size)
    X = DA.from_numpy(Xh)
    for i in range(-d, d):
        for got in (X.column(i), X[..., i], X[:, i], X[:, np.int64(i)]):
            assert got.shape == (N,)
            same(got, Xh[:, i], None, "column %d" % i)
    for i in (d, -d - 1):
        for f in (lambda: X.column(i), lambda: X[..., i], lambda: X[:, i]):
            with pytest.raises(IndexError):
                f()
    cols = [X[:, i] for i in range(d)]
    for back in (DA.stack_columns(cols), np.stack(cols, axis=1)):
        assert isinstance(back, DA) and back.shape == (N, d)
        same(back, Xh, None, "stack_columns")
    if N > 1:
        with pytest.raises(ValueError):
            DA.stack_columns(cols + [DA.from_numpy(Xh[:-1, 0])])
    with pytest.raises(TypeError):
        DA.from_numpy(Xh[:, 0]).column(0)                            # 1-D
    with pytest.raises(TypeError):
        DA.from_numpy(np.arange(N * d).reshape(N, d)).column(0)      # int64


def check_gather(M, d):
    """x[A] from N = 1000 rows: A a host int64 array, a list, a device int64 array; float64 and int64 sources."""
    N = 1000
    rng = np.random.default_rng(100 + M + d)
    Xh = rng.standard_normal((N, d)) if d > 1 else rng.standard_normal(N)
    Xh.reshape(-1)[:SPECIALS.size] = SPECIALS
    Ih = rng.integers(-2 ** 62, 2 ** 62, size=Xh.shape)              # an int64 source (h_order[idx], core.py:344)
    A = rng.integers(0, N, size=M)
    A[0] = 0
    A[-1] = N - 1 if M > 1 else 0
    for src, srch in ((DA.from_numpy(Xh), Xh), (DA.from_numpy(Ih), Ih)):
        for idx in (A, list(A), DA.from_numpy(A), A.astype(np.int32)):
            got = src[idx]
            assert isinstance(got, DA) and got.dtype == srch.dtype and got.shape == srch[A].shape
            g, w = got.get(), srch[A]
            assert np.array_equal(g.view(np.int64), w.view(np.int64)), (M, d)         # the words themselves


def check_host_index():
    """A host index follows NumPy: negatives wrap, a boolean mask selects, a float index array and an index out of
    range raise IndexError -- and the caller's index array is left as it was."""
    rng = np.random.default_rng(110)
    for Xh in (rng.standard_normal(1000), rng.standard_normal((1000, 5))):
        X = DA.from_numpy(Xh)
        A = np.array([-1, 0, -1000, 999, -500, 3])
        keep = A.copy()
        assert np.array_equal(X[A].get(), Xh[A]) and np.array_equal(A, keep)
        assert np.array_equal(X[[-1, 2]].get(), Xh[[-1, 2]])
        mask = Xh.reshape(1000, -1)[:, 0] > 0.3
        assert np.array_equal(X[mask].get(), Xh[mask])
        assert np.array_equal(X[list(mask)].get(), Xh[mask])
        for bad in (np.array([1.0, 2.0]), [0.5], np.array([0, 1000]), np.array([-1001]), [3, 1000],
                    np.ones(999, dtype=bool), np.array(["1"])):
            with pytest.raises(IndexError):
                X[bad]
        for bad in ((A, 0), (A, slice(None)), (slice(None), slice(None)), (0, 1), (Ellipsis, A)):
            with pytest.raises(TypeError):
                X[bad]
        with pytest.raises(TypeError):
            X[DA.from_numpy(np.array([1.0, 2.0]))]                   # a float64 device array is no index


# ---------------------------------------------------------------- refusals ----
def check_refusals():
    """Every call that returned a wrong answer without an error, or read past an allocation, before the host layer
    checked what it hands the kernels: now refused before any launch, or computed as NumPy computes it."""
    xh = np.arange(8.0)
    x = DA.from_numpy(xh)
    k = DA.from_numpy(np.arange(8))
    assert k.dtype == np.int64
    msg = "device arithmetic is defined for float64 arrays"
    # dtype: an int64 device array is never read as doubles
    for f in (lambda: x + k, lambda: k + x, lambda: x * k, lambda: np.add(x, k), lambda: np.minimum(x, k),
              lambda: x ** k, lambda: xh + k, lambda: -k, lambda: np.exp(k),
              lambda: dists.Poisson(rate=x + 1.0).logpdf(k),
              lambda: dists.Normal(loc=k).logpdf(x), lambda: dists.Normal(scale=k).ppf(x),
              lambda: dists.Normal(loc=x).logpdf(k), lambda: dists.Normal(loc=x).rvs(size=8, z=k),
              lambda: dists.MvNormal(loc=DA.from_numpy(np.arange(2)), cov=np.eye(2)).logpdf(np.zeros((4, 2))),
              lambda: dists.MvNormal(cov=np.eye(2), loc=np.zeros(2)).logpdf(DA.from_numpy(np.arange(8).reshape(4, 2))),
              lambda: dists.MvNormal(cov=np.eye(2), loc=np.zeros(2)).rvs(size=4, z=DA.from_numpy(np.arange(8))),
              lambda: dists.MvNormal(cov=np.eye(2), loc=np.zeros(2)).ppf(DA.from_numpy(np.arange(8).reshape(4, 2))),
              lambda: rs.Weights(lw=k), lambda: rs.Weights(lw=x).add(k), lambda: rs.Weights().add(k),
              lambda: rs.Weights(lw=xh.copy()).add(k)):
        with pytest.raises(TypeError, match=msg):
            f()
    # sizes of device operands: nothing is read past an allocation
    a, b = DA.from_numpy(np.zeros(1024)), DA.from_numpy(np.zeros(5))
    for f in (lambda: dists.Normal(loc=a).logpdf(b), lambda: dists.Normal(loc=b).logpdf(a),
              lambda: dists.Normal(loc=a, scale=b).ppf(0.5), lambda: dists.Poisson(rate=a).logpdf(b),
              lambda: dists.Normal(loc=a).rvs(size=1024, z=np.ones(4)),
              lambda: dists.Normal(loc=a).rvs(size=1024, z=b), lambda: dists.Normal(loc=a).rvs(z=b),
              lambda: dists.Normal(loc=b).rvs(size=1024),
              lambda: dists.MvNormal(loc=DA.from_numpy(np.zeros(6)), cov=np.eye(3)).logpdf(np.zeros((100, 3))),
              lambda: dists.MvNormal(loc=DA.from_numpy(np.zeros(6)), cov=np.eye(3)).rvs(size=100, z=np.zeros((100, 3))),
              lambda: dists.MvNormal(loc=np.zeros(3), cov=np.eye(3)).rvs(size=100, z=DA.from_numpy(np.zeros(6))),
              lambda: dists.MvNormal(loc=np.zeros(3), cov=np.eye(3)).rvs(size=100, z=np.zeros(6)),
              lambda: dists.MvNormal(loc=np.zeros(3), cov=np.eye(3)).logpdf(DA.from_numpy(np.zeros(1024))),
              lambda: a + b, lambda: rs.Weights(lw=a).add(b)):
        with pytest.raises(ValueError):
            f()
    # broadcast shapes: as NumPy, or refused
    X3h = np.arange(9.0).reshape(3, 3)
    X3 = DA.from_numpy(X3h)
    ch = np.array([[10.0], [20.0], [30.0]])
    c4, col4 = np.arange(4.0), np.arange(4.0).reshape(4, 1)
    bc = "operands could not be broadcast together"
    for f in (lambda: X3 + DA.from_numpy(ch), lambda: X3 + ch, lambda: DA.from_numpy(ch) + X3, lambda: ch * X3,
              lambda: DA.from_numpy(c4) + DA.from_numpy(col4), lambda: DA.from_numpy(col4) + DA.from_numpy(c4),
              lambda: x + np.ones((8, 1)), lambda: np.ones((8, 1)) - x, lambda: np.maximum(x, np.ones((8, 1))),
              lambda: x + DA.from_numpy(np.ones(7)), lambda: x + np.ones(7), lambda: X3 + np.ones((3, 2)),
              lambda: X3 + np.ones((2, 3)), lambda: X3 + DA.from_numpy(np.ones(9))):
        with pytest.raises(ValueError, match=bc):
            f()
    with np.errstate(all="ignore"):
        for other in (np.ones((1, 8)), np.ones((1, 1)), np.ones((1, 1, 8)), np.full((1,), 2.0), np.float64(2.0)):
            for o in (other, DA.from_numpy(other)):                  # the shapes NumPy gives, (1, 8) among them
                same(x + o, xh + other, None, "x + %s" % (np.shape(other),))
                same(o - x, other - xh, None, "%s - x" % (np.shape(other),))
        same(X3 + np.arange(3.0), X3h + np.arange(3.0), None, "row")
        same(X3 + DA.from_numpy(np.arange(3.0).reshape(1, 3)), X3h + np.arange(3.0), None, "(1, d) row")
        same(DA.from_numpy(ch) + DA.from_numpy(ch), ch + ch, None, "(N, 1) with (N, 1)")
        same(DA.from_numpy(np.ones((2, 3, 3))) + X3, 1.0 + np.broadcast_to(X3h, (2, 3, 3)), None, "trailing block")
    # indices
    assert np.array_equal(x[xh > 3].get(), xh[xh > 3])
    with pytest.raises(IndexError):
        x[np.array([1.0, 2.0])]
    # an array exponent reaches EW_POW
    e = DA.from_numpy(np.full(8, 2.0))
    assert np.array_equal((x ** e).get(), xh ** 2.0)
