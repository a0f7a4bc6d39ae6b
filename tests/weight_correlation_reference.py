"""The definitions of include/sgmcmc_hip.h, "Correlation between the variables of a stack of weight samples", restated in
numpy at a chosen precision (np.float64 or np.longdouble).  Plain and slow on purpose: nothing here shares code, summation
order or layout with csrc/corr_hip.inc or bnn_priors_amd/weight_correlation.py."""
import numpy as np


def as_matrix(w, var_dim):
    "[S, *shape] -> [V, n]: axis var_dim of shape holds the variables, the remaining axes row-major the observations"
    w = np.asarray(w)
    axis = 1 + var_dim % (w.ndim - 1)
    return np.moveaxis(w, axis, 0).reshape(w.shape[axis], -1)


def mean(x, dtype):
    "m_v = x_v(0) + sum_k (x_v(k) - x_v(0)) / n"
    x = np.asarray(x).astype(dtype)
    x0 = x[:, :1]
    return x0[:, 0] + (x - x0).sum(axis=1) / dtype(x.shape[1])


def covariance(x, ddof=1, dtype=np.float64, m=None, order=None):
    """x [V, n] -> dict(n, mean, cov, corr, zero_variance, nonfinite).  ``m``: means to use instead of x's own;
    ``order`` [V, n]: permute every variable's deviations by its row of the table first (a replicate of the test)."""
    x = np.asarray(x)
    V, n = x.shape
    bad = int((~np.isfinite(x)).sum())
    nan = np.full((V, V), np.nan, dtype=dtype)
    if bad:
        return dict(n=n, mean=np.full(V, np.nan, dtype=dtype), cov=nan, corr=nan.copy(),
                    zero_variance=np.zeros(V, dtype=bool), nonfinite=bad)
    m = mean(x, dtype) if m is None else np.asarray(m, dtype=dtype)
    d = x.astype(dtype) - m[:, None]
    if order is not None:
        d = np.take_along_axis(d, np.asarray(order), axis=1)
    G = d @ d.T
    g = np.diag(G).copy()
    zero = g == 0
    cov = G / dtype(n - ddof)
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = G / np.sqrt(g[:, None] * g[None, :])
    cov[zero, :] = 0
    cov[:, zero] = 0
    corr[zero, :] = np.nan
    corr[:, zero] = np.nan
    return dict(n=n, mean=m, cov=cov, corr=corr, zero_variance=zero, nonfinite=0)


def offdiag(corr, dtype=np.float64):
    """-> dict(variables, pairs, mean, mean_abs, rms, max_abs, argmax, sum_sq) over the pairs i < j of the variables whose
    diagonal entry is not NaN; the arg-max is the smallest (i, j) in row-major order on a tie"""
    corr = np.asarray(corr).astype(dtype)
    keep = np.flatnonzero(~np.isnan(np.diag(corr)))
    a, b = np.triu_indices(len(keep), 1)                 # row-major over i < j
    i, j = keep[a], keep[b]
    nan = dtype(np.nan)
    if len(i) == 0:
        return dict(variables=len(keep), pairs=0, mean=nan, mean_abs=nan, rms=nan, max_abs=nan, argmax=(-1, -1),
                    sum_sq=nan)
    r = corr[i, j]
    at = int(np.argmax(np.abs(r)))                       # the first of equal maxima
    np_ = dtype(len(r))
    return dict(variables=len(keep), pairs=len(r), mean=r.sum() / np_, mean_abs=np.abs(r).sum() / np_,
                rms=np.sqrt((r * r).sum() / np_), max_abs=np.abs(r)[at], argmax=(int(i[at]), int(j[at])),
                sum_sq=(r * r).sum())


def schott(V, n, dtype=np.float64):
    "(mean, variance) of sum_{i<j} r^2 of V independent Gaussian variables observed n times"
    V, nu = dtype(V), dtype(n - 1)
    return V * (V - 1) / (2 * nu), V * (V - 1) * (nu - 1) / (nu * nu * (nu + 2))


def permutation_test(x, perms, dtype=np.float64):
    """x [V, n], perms [B, V, n] -> dict(observed, null [B, 2] = (rms, max |r|), p_rms, p_max, expected_rms, schott_mean,
    schott_var, schott_z).  Every replicate permutes each variable's deviations from the DATA's means."""
    x = np.asarray(x)
    V, n = x.shape
    base = covariance(x, 1, dtype)
    obs = offdiag(base["corr"], dtype)
    null = np.empty((len(perms), 2), dtype=dtype)
    for b, table in enumerate(perms):
        o = offdiag(covariance(x, 1, dtype, m=base["mean"], order=table)["corr"], dtype)
        null[b] = o["rms"], o["max_abs"]
    B = len(perms)
    s_mean, s_var = schott(obs["variables"], n, dtype)
    return dict(observed=obs, null=null, p_rms=(1 + int((null[:, 0] >= obs["rms"]).sum())) / (B + 1),
                p_max=(1 + int((null[:, 1] >= obs["max_abs"]).sum())) / (B + 1),
                expected_rms=1 / np.sqrt(dtype(n - 1)), schott_mean=s_mean, schott_var=s_var,
                schott_z=(obs["sum_sq"] - s_mean) / np.sqrt(s_var))
