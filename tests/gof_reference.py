"""The goodness-of-fit statistics of include/sgmcmc_hip.h (section "Goodness of fit") restated with numpy, scipy and mpmath.

Per element, F, 1 - F and their logarithms come from mpmath at 50 digits (the regularised incomplete gamma and beta
functions, erfc), from the EXACT value of the fp64 inputs, and are rounded to fp64 once.  The statistics are formed from
those in 80-bit arithmetic (np.longdouble), whose rounding is 2^-11 of an fp64's.  mpmath is the reference wherever scipy
is not finite: ``gennorm.logsf(30, 2)``, ``gennorm.logsf(3, 8)``, ``dgamma.logsf(800, 1)`` and ``dgamma.logsf(1000, 3)``
are ``-inf`` in scipy 1.15 and -904.67, -6571.4, -800.69 and -987.57 here.
"""
import collections

import mpmath
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
DIGITS = 50
FAMILIES = ("uniform", "norm", "laplace", "t", "gennorm", "dgamma")
SHAPED = ("t", "gennorm", "dgamma")

Exact = collections.namedtuple("Exact", "F S lF lS lt T")
Exact.__doc__ = ("fp64 arrays: F, S = 1 - F, their logarithms, and lt = log T, T the probability beyond |x - loc| on one "
                 "side (uniform: lt = min(lF, lS), T = min(F, S))")
Stats = collections.namedtuple("Stats", "ks ks_plus ks_minus index cvm ad")


def unpack(family, params):
    "(shape or None, loc, scale) in mpmath numbers"
    params = [mpmath.mpf(float(v)) for v in params]
    if family in SHAPED:
        return params[0], params[1], params[2]
    return None, params[0], params[1]


def tail(family, shape, z):
    "T(z), the probability beyond z > 0 on one side, in the working precision"
    if family == "norm":
        return mpmath.erfc(z / mpmath.sqrt(2)) / 2
    if family == "laplace":
        return mpmath.exp(-z) / 2
    if family == "t":                                   # whichever of I_x(df/2, 1/2) and 1 - I_(1 - x)(1/2, df/2) has the smaller argument
        den, half = shape + z * z, mpmath.mpf(1) / 2
        if z * z < shape:
            with mpmath.extradps(20):
                return (1 - mpmath.betainc(half, shape / 2, 0, z * z / den, regularized=True)) / 2
        return mpmath.betainc(shape / 2, half, 0, shape / den, regularized=True) / 2
    if family == "gennorm":
        return mpmath.gammainc(1 / shape, z ** shape, mpmath.inf, regularized=True) / 2
    if family == "dgamma":
        return mpmath.gammainc(shape, z, mpmath.inf, regularized=True) / 2
    raise ValueError(family)


def _log(v):
    return mpmath.log(v) if v > 0 else -mpmath.inf


def exact_one(family, params, x):
    "(F, S, lF, lS, lt, T) of one fp64 x as mpmath numbers"
    shape, loc, scale = unpack(family, params)
    x = mpmath.mpf(float(x))
    if family == "uniform":
        u = min(max((x - loc) / scale, mpmath.mpf(0)), mpmath.mpf(1))
        F, S = u, 1 - u
        lF, lS = _log(F), _log(S)
        return F, S, lF, lS, min(lF, lS), min(F, S)
    d = x - loc
    z = abs(d) / scale
    T = tail(family, shape, z) if z > 0 else mpmath.mpf(1) / 2
    lt, big, lbig = _log(T), 1 - T, mpmath.log1p(-T)
    if d > 0:
        return big, T, lbig, lt, lt, T
    if d < 0:
        return T, big, lt, lbig, lt, T
    return T, T, lt, lt, lt, T


def exact(family, params, xs):
    "``Exact`` of the fp64 values xs: 50 digits, rounded once"
    with mpmath.workdps(DIGITS):
        rows = [[float(v) for v in exact_one(family, params, x)] for x in np.asarray(xs, dtype=np.float64).ravel()]
    return Exact(*np.array(rows, dtype=np.float64).reshape(-1, 6).T)


def tail_window(family, params, x, width):
    """(T(z + width), T(max(z - width, 0))) in fp64, z = |x - loc| / scale exactly: what the tail at x can be when z is
    known to `width` only (a quantile loc +- scale z carries the rounding of its product and of its sum)"""
    with mpmath.workdps(DIGITS):
        shape, loc, scale = unpack(family, params)
        z, width = abs(mpmath.mpf(float(x)) - loc) / scale, mpmath.mpf(float(width))
        inner = max(z - width, mpmath.mpf(0))
        return float(tail(family, shape, z + width)), float(tail(family, shape, inner) if inner > 0 else mpmath.mpf(1) / 2)


def statistics(F, lF, lS):
    """``Stats`` of u_i = F(x_(i)) and the logarithms, in ascending order of x: include/sgmcmc_hip.h, definition 2, in
    80-bit arithmetic.  ``index`` is 1-based: the smallest index that attains the supremum (of D+ where D+ >= D-)."""
    F, lF, lS = (np.asarray(v, dtype=np.float64).astype(LD) for v in (F, lF, lS))
    n = len(F)
    i = np.arange(1, n + 1, dtype=LD)
    nl = LD(n)
    dp, dm = i / nl - F, F - (i - 1) / nl
    ip, im = int(np.argmax(dp)), int(np.argmax(dm))               # argmax: the first of equal values
    ks_plus, ks_minus = dp[ip], dm[im]
    index = (ip if ks_plus >= ks_minus else im) + 1
    e = F - (2 * i - 1) / (2 * nl)
    cvm = 1 / (12 * nl) + np.sum(e * e)
    with np.errstate(invalid="ignore"):
        terms = (2 * i - 1) * lF + (2 * (nl - i) + 1) * lS
    total = np.sum(terms) if np.all(np.isfinite(terms)) else LD(-np.inf)
    ad = -nl - total / nl
    return Stats(float(max(ks_plus, ks_minus)), float(ks_plus), float(ks_minus), index, float(cvm), float(ad))


def uniform_exact(xs, loc=0.0, scale=1.0):
    "``Exact`` of the uniform family in 80-bit arithmetic (its F is a clamp, its logarithms are libm's): for large n"
    u = np.clip((np.asarray(xs, dtype=np.float64).astype(LD) - LD(loc)) / LD(scale), 0, 1)
    with np.errstate(divide="ignore"):
        lF, lS = np.log(u), np.log1p(-u)
    f = [v.astype(np.float64) for v in (u, 1 - u, lF, lS, np.minimum(lF, lS), np.minimum(u, 1 - u))]
    return Exact(*f)


def element_tolerances(ex, tol, uniform=False):
    """What a per-element tolerance `tol` of the log-tail (relative to max(1, |lt|)) allows F, log F and log(1 - F) to
    deviate by, to first order: (tol_u, tol_lF, tol_lS), absolute, per element.  The small side's logarithm is lt itself:
    tol max(1, |lt|); the plain tail T = exp(lt) moves by dT = T tol max(1, |lt|); the large side is 1 - T and
    log1p(-T): dT (+ one rounding) and dT / (1 - T) (+ one rounding).  uniform: F is a rounded quotient, its logarithms
    are held to tol max(1, |log|)."""
    lt_tol = tol * np.maximum(1.0, np.abs(ex.lt))
    if uniform:
        with np.errstate(invalid="ignore"):
            tl = lambda l: np.where(np.isfinite(l), tol * np.maximum(1.0, np.abs(l)), 0.0)   # noqa: E731
        return np.full(len(ex.F), EPS), tl(ex.lF), tl(ex.lS)
    dT = np.where(np.isfinite(ex.lt), ex.T * lt_tol, 0.0)
    tol_u = dT + EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        big = dT / (1.0 - ex.T) + EPS * np.abs(np.log1p(-ex.T))
    lower = ex.F <= ex.S                                          # x on the lower side: log F is the log-tail
    small = np.where(np.isfinite(ex.lt), lt_tol, 0.0)
    return tol_u, np.where(lower, small, big), np.where(lower, big, small)


def statistic_bounds(ex, tol, uniform=False):
    """(dD, dW2, dA2): the allowed deviation of each statistic, by first-order propagation of ``element_tolerances``:
       |dD|   <= max tol_u + eps
       |dW^2| <= sum 2 |u_i - c_i| tol_u,i + 4 eps W^2
       |dA^2| <= (1/n) sum [(2 i - 1) tol_lF,i + (2 (n - i) + 1) tol_lS,i] + 4 eps (n + |sum| / n)"""
    tol_u, tol_lF, tol_lS = element_tolerances(ex, tol, uniform)
    n = len(ex.F)
    i = np.arange(1, n + 1, dtype=np.float64)
    st = statistics(ex.F, ex.lF, ex.lS)
    c = (2 * i - 1) / (2 * n)
    dD = float(np.max(tol_u)) + EPS
    dW = float(np.sum(2 * np.abs(ex.F - c) * tol_u)) + 4 * EPS * st.cvm
    total = abs(st.ad + n) * n                                    # |sum|
    dA = float(np.sum((2 * i - 1) * tol_lF + (2 * (n - i) + 1) * tol_lS)) / n + 4 * EPS * (n + total / n)
    return dD, dW, dA


# ---- the grid of the special-function test ------------------------------------------------------------------------------
LOC, SCALE = 0.375, 1.75            # a non-trivial location and scale (exact in fp64)
NORM_Z = (0.0, 1e-300, 1e-8, 0.5, 5.0, 38.0, 40.0)
GRID = (
    [("norm", (), z) for z in NORM_Z]
    + [("laplace", (), z) for z in NORM_Z + (700.0, 800.0)]
    + [("t", (df,), z) for df in (0.5, 2.01, 5.0, 1e4) for z in (0.0, 1e-8, 1.0, 40.0, 1e6)]
    + [("gennorm", (b,), z) for b in (0.3, 1.0, 2.0, 8.0) for z in (0.0, 1e-3, 0.5, 3.0, 5.0, 30.0, 1e4)]
    + [("dgamma", (a,), z) for a in (0.2, 1.0, 3.0, 50.0) for z in (1e-3, 10.0, 50.0, 200.0, 800.0, 1000.0)]
)
LOWEST_LOG_TAIL = -1e5              # combinations whose exact log-tail is below it are dropped
# where scipy 1.15 returns -inf: (family, shape, z at loc = 0, scale = 1)
SCIPY_INFINITE = (("gennorm", (2.0,), 30.0), ("gennorm", (8.0,), 3.0), ("dgamma", (1.0,), 800.0), ("dgamma", (3.0,), 1000.0))


def grid_cases():
    """[(family, params, x)]: every grid point on both sides of loc, at (0, 1) -- where x is z itself -- and at (LOC, SCALE),
    where x = loc +- z scale is rounded and the exact functions are taken at that x.  The four points where scipy is
    -inf are among them; combinations whose log-tail is below LOWEST_LOG_TAIL are dropped."""
    cases = []
    with mpmath.workdps(DIGITS):
        for fam, shape, z in GRID:
            if z > 0 and mpmath.log(tail(fam, mpmath.mpf(shape[0]) if shape else None, mpmath.mpf(z))) < LOWEST_LOG_TAIL:
                continue
            for loc, scale in ((0.0, 1.0), (LOC, SCALE)):
                for sign in ((1.0, -1.0) if z > 0 else (1.0,)):
                    cases.append((fam, shape + (loc, scale), loc + sign * z * scale))
    assert all((fam, shape + (0.0, 1.0), z) in cases for fam, shape, z in SCIPY_INFINITE)
    return cases


def log_tail_distance(value, lt):
    "the distance of a log-tail from the exact one, relative to max(1, |lt|)"
    return abs(value - lt) / max(1.0, abs(lt))
