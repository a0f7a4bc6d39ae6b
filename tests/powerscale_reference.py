"""numpy restatement of include/sgmcmc_hip.h, "Power-scaling sensitivity": the keyed column sort and the weighted-ECDF
distance with the weighted moments, operation by operation.  numpy's fp64 elementwise arithmetic rounds every operation
once and contracts nothing, so everything but log1p is the device's arithmetic to the bit; ``distance`` reports which
results involve log1p at all.  Not imported by the package."""
import collections
import math

import numpy as np

MIN_DRAWS, MAX_DRAWS, TILE_CELLS, MAX_TILE = 5, 8192, 8192, 64
TWO_LN2 = 1.3862943611198906
SERIES_TERMS = 16
COEFFS = tuple(1.0 / (k * (2 * k - 1)) for k in range(1, SERIES_TERMS + 1))        # the doubles nearest 1 / (k (2k - 1))

Distance = collections.namedtuple("Distance", "dist wmean wsd num den W series max_delta log1p_args")


def tile_quantities(N):
    if not MIN_DRAWS <= N <= MAX_DRAWS:
        return 0
    return min(TILE_CELLS // max(8, 1 << (N - 1).bit_length()), MAX_TILE)


def keyed_sort(x):
    """x [N, Q] (the draws in the order t = m S + s) -> (sorted [N, Q] fp64, order [N, Q] int64, bad [Q]): every column
    ascending by value, ties by ascending draw index (a stable sort by value); -0.0 as +0.0; a column with a non-finite
    draw is NaN, its order the identity (the definition leaves it unspecified)."""
    x = np.asarray(x, dtype=np.float64) + 0.0                  # -0.0 + 0.0 = +0.0
    N, Q = x.shape
    bad = ~np.isfinite(x).all(axis=0)
    order = np.argsort(np.where(bad[None, :], 0.0, x), axis=0, kind="stable")
    ordered = np.take_along_axis(x, order, axis=0)
    ordered[:, bad] = np.nan
    order[:, bad] = np.arange(N)[:, None]
    return ordered, order, bad


def g_series(delta):
    "the series of g in x = delta^2 by Horner: acc = 0; for k = 16 .. 1: acc = (acc + c_k) x"
    x = delta * delta
    acc = np.zeros_like(x)
    for k in range(SERIES_TERMS, 0, -1):
        acc = (acc + COEFFS[k - 1]) * x
    return acc


def g_log1p(delta):
    "(1 - delta) log1p(-delta) + (1 + delta) log1p(delta) with 0 (-inf) = 0"
    with np.errstate(all="ignore"):
        t1 = np.where(delta >= 1.0, 0.0, (1.0 - delta) * np.log1p(-delta))
        t2 = np.where(delta <= -1.0, 0.0, (1.0 + delta) * np.log1p(delta))
    return t1 + t2


def g(delta):
    "-> (g(delta), which elements took the series)"
    delta = np.asarray(delta, dtype=np.float64)
    small = np.abs(delta) < 0.25
    with np.errstate(all="ignore"):
        return np.where(small, g_series(delta), g_log1p(np.where(small, 0.5, delta))), small


def distance(ordered, order, w, keep_args=False):
    """ordered, order [N, Q] (the keyed sort's output) and linear weights w [N, A] -> ``Distance``: dist, wmean, wsd, num
    (after the division by 2 ln 2), den, each [A, Q]; W [A]; series [A, Q]: every delta of the result took the series
    (|delta| < 1/4: the result is fixed to the bit); max_delta [A, Q]; log1p_args: with ``keep_args`` the deltas that took
    the log1p form, concatenated (the arguments of log1p are -delta and delta)."""
    ordered, w = np.asarray(ordered, dtype=np.float64), np.asarray(w, dtype=np.float64)
    order = np.asarray(order).astype(np.int64)
    N, Q = ordered.shape
    A = w.shape[1]
    W = np.zeros(A)
    for t in range(N):
        W = W + w[t]
    with np.errstate(all="ignore"):
        valid = (np.isfinite(w) & (w >= 0.0)).all(axis=0) & (W > 0.0) & np.isfinite(W)
        nan_col = np.isnan(ordered[0])
        C, top, den, swv = (np.zeros((A, Q)) for _ in range(4))
        series = np.ones((A, Q), dtype=bool)
        max_delta = np.zeros((A, Q))
        args = []
        Wc = W[:, None]
        for i in range(N):
            wi = w[order[i]].T                                  # [A, Q]
            v = ordered[i][None, :]
            swv = swv + wi * v
            if i == N - 1:
                break
            C = C + wi
            Qi = C / Wc
            Pi = float(i + 1) / float(N)
            s = Pi + Qi
            delta = (Qi - Pi) / s
            ds = (ordered[i + 1][None, :] - v) * s
            den = den + ds
            gd, small = g(delta)
            top = top + ds * gd
            live = valid[:, None] & ~nan_col[None, :]
            series &= small | ~live
            max_delta = np.where(live, np.maximum(max_delta, np.abs(delta)), max_delta)
            if keep_args and (~small & live).any():
                args.append(delta[~small & live])
        first, last = ordered[0][None, :], ordered[N - 1][None, :]
        constant = np.broadcast_to(first == last, (A, Q))
        mean = np.where(constant, first, swv / Wc)
        m2 = np.zeros((A, Q))
        for i in range(N):
            c = ordered[i][None, :] - mean
            m2 = m2 + w[order[i]].T * (c * c)
        num = top / TWO_LN2
        dist = np.where(den == 0.0, 0.0, np.sqrt(num / den))
        sd = np.where(constant, 0.0, np.sqrt(m2 / Wc))
    dead = ~valid[:, None] | nan_col[None, :]
    out = [np.where(dead, np.nan, t) for t in (dist, mean, sd, num, den)]
    return Distance(*out, W, series, max_delta, np.concatenate(args) if args else np.zeros(0))


def distance_of_draws(x, w, **kw):
    "x [N, Q], w [N, A] -> ``Distance`` through ``keyed_sort``"
    ordered, order, _ = keyed_sort(x)
    return distance(ordered, order, w, **kw)


def ratios(log_component, alphas):
    "[N, A]: (alpha - 1) log p"
    return np.asarray(log_component, dtype=np.float64).reshape(-1, 1) * np.array([a - 1.0 for a in alphas])


def sensitivity(d_lo, d_hi, alpha):
    "(psi, mean_gradient, sd_gradient) from the (dist, wmean, wsd) triples at the powers 1 / alpha and alpha"
    scale = 2.0 * math.log2(alpha)
    return (d_lo[0] + d_hi[0]) / scale, (d_hi[1] - d_lo[1]) / scale, (d_hi[2] - d_lo[2]) / scale


def diagnosis(psi_prior, psi_likelihood, threshold):
    "0 none, 1 prior-data conflict, 2 strong prior or weak likelihood"
    p, l = psi_prior >= threshold, psi_likelihood >= threshold
    return (p & l).astype(np.int8) * 1 + (p & ~l).astype(np.int8) * 2


def g_exact(delta, digits=50):
    "g in mpmath arithmetic"
    import mpmath
    with mpmath.workdps(digits):
        d = mpmath.mpf(delta)
        t1 = mpmath.mpf(0) if d >= 1 else (1 - d) * mpmath.log1p(-d)
        t2 = mpmath.mpf(0) if d <= -1 else (1 + d) * mpmath.log1p(d)
        return t1 + t2


def log1p_distance(args, digits=50):
    "the largest relative distance of numpy's log1p from mpmath's over the arguments (each a double, taken exactly)"
    import mpmath
    worst = 0.0
    with mpmath.workdps(digits):
        for u in np.asarray(args, dtype=np.float64):
            if u <= -1.0 or u == 0.0:
                continue
            want = mpmath.log1p(mpmath.mpf(float(u)))
            worst = max(worst, float(abs((mpmath.mpf(float(np.log1p(u))) - want) / want)))
    return worst
