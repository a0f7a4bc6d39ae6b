"""The definitions behind bnn_priors_amd/temperature.py, restated for tests/test_temperature.py: the chi-square tails and
quantiles in mpmath at 50 digits, the EWMA and Cochran's weighted mean / standard error in numpy (in float64, the
restatement, and in longdouble, its yardstick).

With a = d / 2 and r = T^ / T the lower tail is P(a, a r), the upper Q = 1 - P.  For d <= 1e6 both come from
``mpmath.gammainc``; above it (and in the far tails at d = 1e6) that raises NoConvergence.  Then, within 10 sqrt(a) of a,
the tail on r's side of 1 is the integral of the density t^(a-1) e^-t / Gamma(a) from x outwards over 15 pieces of 4 sqrt(a);
beyond, it is the series of P or Legendre's continued fraction of Q summed at 50 digits, which end after about
115 a / |x - a| terms there.  The other tail is one minus it.  Where gammainc exists the three agree to 1e-30 relative
(tests/test_temperature.py::test_reference_methods_agree).
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = 2.0 ** -52
GAMMAINC_MAX_D = 10 ** 6


def _by_quadrature(a, x):
    """(P, Q) near the bulk, |x - a| <= 10 sqrt(a): the tail on x's side of a as the integral of the density from x
    outwards over 15 pieces of 4 sqrt(a), the other one minus it"""
    lg, width = mp.loggamma(a), 4 * mp.sqrt(a)
    density = lambda t: mp.exp((a - 1) * mp.log(t) - t - lg)
    if x < a:
        p = mp.quad(density, [max(mp.mpf(0), x - i * width) for i in range(15, -1, -1)])
        return p, 1 - p
    q = mp.quad(density, [x + i * width for i in range(16)])
    return 1 - q, q


def _by_expansion(a, x):
    """(P, Q) in a far tail, |x - a| > 10 sqrt(a), where the convergent expansions end after about 115 a / |x - a| terms at
    50 digits: the series of P below a, Legendre's continued fraction of Q (modified Lentz) above it"""
    front = mp.exp(a * mp.log(x) - x - mp.loggamma(a))
    tiny = mp.mpf(10) ** -60
    if x < a:
        term = total = 1 / a
        k = a
        while term > tiny * total:
            k += 1
            term *= x / k
            total += term
        p = front * total
        return p, 1 - p
    b = x + 1 - a
    c, d = 1 / (tiny * tiny), 1 / b
    h = d
    i = 0
    while True:
        i += 1
        an = -i * (i - a)
        b += 2
        d = 1 / (an * d + b)
        c = b + an / c
        delta = d * c
        h *= delta
        if abs(delta - 1) < tiny:
            break
    q = front * h
    return 1 - q, q


def tails(d, r):
    "(P, Q) of chi^2_d / d at the double r, taken as the exact number it is: mpf"
    a, x = mp.mpf(d) / 2, mp.mpf(d) / 2 * mp.mpf(r)
    if d <= GAMMAINC_MAX_D:
        try:
            return mp.gammainc(a, 0, x, regularized=True), mp.gammainc(a, x, mp.inf, regularized=True)
        except mp.libmp.NoConvergence:                     # (far tails at the largest of these sizes)
            pass
    return _by_quadrature(a, x) if abs(x - a) <= 10 * mp.sqrt(a) else _by_expansion(a, x)


def log_tails(d, r):
    p, q = tails(d, r)
    return mp.log(p), mp.log(q)


def sensitivity(d, r, upper):
    "|x d log F / dx| at x = a r, F the upper or the lower tail: what one relative rounding of r does to log F, per eps"
    a = mp.mpf(d) / 2
    x = a * mp.mpf(r)
    p, q = tails(d, r)
    return abs(mp.exp(a * mp.log(x) - x - mp.loggamma(a)) / (q if upper else p))


def quantile(d, prob, upper, start_given=None):
    "the r with tail(d, r) = prob (prob a double taken exactly): mpf.  start: a double known to be close"
    a = mp.mpf(d) / 2
    target = mp.log(mp.mpf(prob))
    z = mp.sqrt(2) * mp.erfinv(2 * mp.mpf(prob) - 1)
    if upper:
        z = -z
    start = (1 - 1 / (9 * a) + z / (3 * mp.sqrt(a))) ** 3
    if not start > 0:
        start = mp.exp((target + mp.loggamma(a + 1)) / a) / a
    if start_given is not None:
        start = mp.mpf(start_given)
    r = start
    for _ in range(60):                                   # Newton on the log-tail: d log F / dr = -+ density / F
        p, q = tails(d, r)
        x = a * r
        tail = q if upper else p
        slope = mp.exp(a * mp.log(x) - x - mp.loggamma(a)) / tail / r
        step = (mp.log(tail) - target) / (-slope if upper else slope)
        r = r - step
        if abs(step) < mp.mpf(10) ** -40 * r:
            break
    return r


def interval(d, confidence):
    "(lower, upper) of plot.py's _gamma_confidence: the tails (1 - c) / 2 and 1 - (1 + c) / 2, formed in double as scipy is given them"
    c = float(confidence)
    return quantile(d, (1.0 - c) / 2.0, False), quantile(d, 1.0 - (1.0 + c) / 2.0, True)


def ewma(x, alpha, dtype=np.float64):
    "y_0 = x_0, y_t = (1 - alpha) x_t + alpha y_(t-1) along the last axis, one step after the other"
    x = np.asarray(x).astype(dtype)
    if alpha == 0.0:
        return x.copy()
    alpha = dtype(alpha)
    y = np.empty_like(x)
    y[..., 0] = x[..., 0]
    for t in range(1, x.shape[-1]):
        y[..., t] = (dtype(1) - alpha) * x[..., t] + alpha * y[..., t - 1]
    return y


def weighted_var_se(w, x, dtype=np.float64):
    "plot.py's weighted_var_se (Cochran 1977), the same expression"
    w, x = np.asarray(w).astype(dtype), np.asarray(x).astype(dtype)
    n = dtype(w.shape[0])
    total = w.sum()
    mean = (x * w).sum(-1) / total
    wbar = total / n
    dw = w - wbar
    e = w * x - wbar * mean[..., None]
    se = n / ((n - dtype(1)) * total ** 2) * ((e ** 2).sum(-1) - dtype(2) * mean * (e * dw).sum(-1) + mean ** 2 * (dw * dw).sum())
    return mean, se


def bound(ref64, ref_long, result_scale=None):
    """tests/test_raob.py's rule: four times the float64 restatement's own distance from longdouble plus 4 ulp of the
    largest magnitude, both as max-norms over the finite entries"""
    ref64, ref_long = np.asarray(ref64), np.asarray(ref_long)
    ok = np.isfinite(ref_long.astype(np.float64))
    if not ok.any():
        return 0.0
    scale = float(np.max(np.abs(ref_long[ok]).astype(np.float64))) if result_scale is None else result_scale
    dist = float(np.max(np.abs(ref64[ok].astype(np.longdouble) - ref_long[ok])))
    return 4.0 * dist + 4.0 * EPS * scale
