"""Plain numpy restatement of the regression scores that ``include/sgmcmc_hip.h`` defines (``sgmcmc_gmix_rows`` /
``sgmcmc_gmix_quantiles`` / ``sgmcmc_pit_calibration``; bnn_priors_amd/regression.py), in a floating-point type of the
caller's choice (``np.float64``, or ``np.longdouble`` to measure what fp64 loses).  Written from the definition, not from
the kernels: whole-array numpy over all pairs of samples, no tiles, no slices, no partials.

numpy has no error function.  In ``np.float64`` it is scipy's; in ``np.longdouble`` it is a Taylor expansion about the
nearest multiple of 1/8 whose coefficients (erf and its derivatives, Hermite polynomials times exp(-x^2)) mpmath supplies
at 40 digits: absolute accuracy about 1e-19, which is what the absolute and first-term-relative comparisons here need
(``erfc`` is 1 - erf there: the 80-bit tails are accurate absolutely, not relatively)."""
import functools

import numpy as np

ERF_STEP, ERF_KNOTS, ERF_ORDER = 8, 57, 22          # knots k / 8 for k = 0 .. 56 (x <= 7); erf(x > 7.0625) = 1 - 2e-23


@functools.lru_cache(maxsize=None)
def _erf_coefficients():
    import mpmath
    coef = np.zeros((ERF_ORDER + 1, ERF_KNOTS), dtype=np.longdouble)
    with mpmath.workdps(40):
        pre = 2 / mpmath.sqrt(mpmath.pi)
        for k in range(ERF_KNOTS):
            x = mpmath.mpf(k) / ERF_STEP
            g = pre * mpmath.exp(-x * x)
            for n in range(ERF_ORDER + 1):
                v = mpmath.erf(x) if n == 0 else (-1) ** (n - 1) * mpmath.hermite(n - 1, x) * g / mpmath.factorial(n)
                coef[n, k] = np.longdouble(mpmath.nstr(v, 30))
    coef.setflags(write=False)
    return coef


def erf(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    if dtype is np.float64:
        from scipy.special import erf as erf64
        return erf64(x)
    coef = _erf_coefficients()
    a = np.abs(x)
    k = np.minimum(np.rint(np.where(np.isfinite(a), a, 0) * ERF_STEP), ERF_KNOTS - 1).astype(np.int64)
    dx = np.minimum(a - k.astype(np.longdouble) / ERF_STEP, np.longdouble(1))
    r = coef[ERF_ORDER][k]
    for n in range(ERF_ORDER - 1, -1, -1):
        r = r * dx + coef[n][k]
    r = np.where(a > 7.0625, np.longdouble(1), r)
    return np.where(np.isnan(x), x, np.sign(x) * r)


def erfc(x, dtype=np.float64):
    if dtype is np.float64:
        from scipy.special import erfc as erfc64
        return erfc64(np.asarray(x, dtype=dtype))
    return 1 - erf(x, dtype)


def sum0(a):
    "the sum over the first axis, pairwise (numpy sums pairwise only along a contiguous last axis)"
    return np.ascontiguousarray(np.moveaxis(a, 0, -1)).sum(-1)


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def normal_cdf(z, dtype=np.float64):
    "Phi(z) = erfc(-z / sqrt 2) / 2"
    return erfc(-np.asarray(z, dtype=dtype) / np.sqrt(dtype(2)), dtype) / 2


def abs_moment(m, s, dtype=np.float64):
    "A(m, s) = m erf(m / (s sqrt 2)) + 2 s phi(m / s)"
    z = m / s
    return m * erf(z / np.sqrt(dtype(2)), dtype) + 2 * s * np.exp(-z * z / 2) / np.sqrt(2 * _pi(dtype))


def broadcast(mean, scale, dtype=np.float64):
    "mean [E, N, D] and scale ([E], [E, D] or broadcastable to [E, N, D]) as two [E, N, D] arrays"
    mu = np.asarray(mean, dtype=dtype)
    sg = np.asarray(scale, dtype=dtype)
    if sg.ndim == 1:
        sg = sg[:, None, None]
    elif sg.ndim == 2:
        sg = sg[:, None, :]
    return mu, np.broadcast_to(sg, mu.shape)


def mixture_reference(mean, scale, y=None, dtype=np.float64, budget=1 << 21):
    """dict of mean, var_aleatoric, var_epistemic, var and, with y [N, D], sq_err, lpd, pit, crps and crps_first (the CRPS'
    first term, which its tolerance is relative to), each [N, D]"""
    mu, sg = broadcast(mean, scale, dtype)
    E, N, D = mu.shape
    with np.errstate(all="ignore"):
        mbar = sum0(mu) / E
        alea = sum0(sg * sg) / E
        epi = sum0((mu - mbar) ** 2) / E
        out = {"mean": mbar, "var_aleatoric": alea, "var_epistemic": epi, "var": alea + epi}
        if y is not None:
            yy = np.asarray(y, dtype=dtype)
            z = (yy - mu) / sg
            logpdf = -z * z / 2 - np.log(sg) - np.log(2 * _pi(dtype)) / 2
            top = logpdf.max(0)
            out["sq_err"] = (yy - mbar) ** 2
            out["lpd"] = top + np.log(sum0(np.exp(logpdf - top))) - np.log(dtype(E))
            out["pit"] = sum0(normal_cdf(z, dtype)) / E
            first = sum0(abs_moment(yy - mu, sg, dtype)) / E
            i, j = np.triu_indices(E, 1)
            pairs = np.zeros((N, D), dtype=dtype)
            rows = max(1, budget // max(1, len(i) * D))
            for n0 in range(0, N, rows):
                m, v = mu[:, n0:n0 + rows], (sg * sg)[:, n0:n0 + rows]
                pairs[n0:n0 + rows] = sum0(abs_moment(m[i] - m[j], np.sqrt(v[i] + v[j]), dtype))
            out["crps_first"] = first
            out["crps"] = first - (pairs + sum0(sg) / np.sqrt(_pi(dtype))) / (dtype(E) * E)
        bad = np.isnan(mu).any(0) | ~(sg > 0).all(0) | (False if y is None else np.isnan(np.asarray(y, dtype=dtype)))
        return {k: np.where(bad, np.nan, v) for k, v in out.items()}


def cdf_reference(x, mean, scale, dtype=np.float64):
    "F(x) for x [..., N, D]"
    mu, sg = broadcast(mean, scale, dtype)
    x = np.asarray(x, dtype=dtype)
    return sum0(np.stack([normal_cdf((x - mu[e]) / sg[e], dtype) for e in range(mu.shape[0])])) / mu.shape[0]


def density_reference(x, mean, scale, dtype=np.float64):
    "the mixture's density f(x) for x [..., N, D]"
    mu, sg = broadcast(mean, scale, dtype)
    x = np.asarray(x, dtype=dtype)
    return sum(np.exp(-((x - mu[e]) / sg[e]) ** 2 / 2) / sg[e] for e in range(mu.shape[0])) \
        / (mu.shape[0] * np.sqrt(2 * _pi(dtype)))


def hull_reference(mean, scale, z):
    "(min_e, max_e) of the components' own quantiles mu_e + sigma_e z, in fp64: [Q, N, D] each"
    mu, sg = broadcast(mean, scale)
    comp = mu[None] + sg[None] * np.asarray(z, dtype=np.float64).reshape(-1, 1, 1, 1)
    return comp.min(1), comp.max(1)


def quantile_reference(mean, scale, probs, z, steps=200):
    "F(q) = p by plain bisection of the hull, [Q, N, D]"
    lo, hi = hull_reference(mean, scale, z)
    p = np.asarray(probs, dtype=np.float64).reshape(-1, 1, 1)
    for _ in range(steps):
        mid = lo + (hi - lo) / 2
        below = cdf_reference(mid, mean, scale) < p
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return lo + (hi - lo) / 2


def pit_reference(u, levels, central, dtype=np.float64):
    "dict of ks, counts [J] = #{u <= p_j}, calibration_error and cover [len(central)] = #{(1-c)/2 <= u <= (1+c)/2}"
    s = np.sort(np.asarray(u, dtype=dtype))
    n = len(s)
    k = np.arange(1, n + 1).astype(dtype)
    p = np.asarray(levels, dtype=dtype)
    c = np.asarray(central, dtype=dtype)
    counts = (s[None, :] <= p[:, None]).sum(1)
    lo, hi = (1 - c) / 2, (1 + c) / 2
    cover = ((s[None, :] >= lo[:, None]) & (s[None, :] <= hi[:, None])).sum(1)
    return {"ks": np.maximum(k / n - s, s - (k - 1) / n).max(), "counts": counts,
            "calibration_error": ((counts.astype(dtype) / n - p) ** 2).sum() / len(p), "cover": cover}


REGIMES = ("tight", "wide", "outlier", "tail")
LAYOUTS = ("E", "ED", "END")


def random_case(rng, E, N, D, layout, regime):
    """(mean [E, N, D], scale in ``layout``, y [N, D]) of a regime: sigma << the spread of mu ("tight"), sigma >> it
    ("wide"), one sample far from the rest ("outlier"), y about 8 sigma out in either tail ("tail")"""
    shape = {"E": (E,), "ED": (E, D), "END": (E, N, D)}[layout]
    jitter = rng.uniform(0.5, 1.5, shape)
    if regime == "tight":
        mean, scale = rng.normal(0.0, 1.0, (E, N, D)), 1e-2 * jitter
    elif regime == "wide":
        mean, scale = 1e-2 * rng.normal(0.0, 1.0, (E, N, D)), jitter
    elif regime == "outlier":
        mean, scale = 0.1 * rng.normal(0.0, 1.0, (E, N, D)), 0.3 * jitter
        mean[E // 2] += 25.0
    else:
        mean, scale = 0.05 * rng.normal(0.0, 1.0, (E, N, D)), 0.9 + 0.2 * (jitter - 0.5)
    mu, sg = broadcast(mean, scale)
    pick = rng.integers(0, E, (N, D))
    rows, cols = np.meshgrid(np.arange(N), np.arange(D), indexing="ij")
    y = mu[pick, rows, cols] + sg[pick, rows, cols] * rng.normal(0.0, 1.0, (N, D))
    if regime == "tail":
        y = np.where((rows + cols) % 2 == 0, 8.0, -8.0) + 0.01 * rng.normal(0.0, 1.0, (N, D))
    return mean, scale, y
