"""A numpy restatement of the kernel Stein discrepancy, its wild bootstrap test and Stein thinning as
include/sgmcmc_hip.h defines them ("Kernel Stein discrepancy and Stein thinning").

``stein_matrix(..., wide=True)`` evaluates K in the DIFFERENCE form in np.longdouble -- r2_ij = sum_d (x_id - x_jd)^2,
t_ij = sum_d (g_id - g_jd) (x_id - x_jd), C_ij = sum_d g_id g_jd -- which shares neither the anchor nor the Gram
identities with the kernels; ``wide=False`` evaluates the anchor / Gram form of the header in float64, operation by
operation in the header's order (but with numpy's own summation order inside the three matrix products).
"""
import numpy as np

LD = np.longdouble


def _pairs(x, g):
    "[(x [S, D_t], g [S, D_t])] in key order"
    if isinstance(x, dict):
        assert sorted(x) == sorted(g)
        return [(np.asarray(x[k]).reshape(len(x[k]), -1), np.asarray(g[k]).reshape(len(g[k]), -1)) for k in sorted(x)]
    return [(np.asarray(x), np.asarray(g))]


def lower_median(v):
    "torch.median's: the lower of the two middle values"
    return np.sort(np.asarray(v).reshape(-1))[(np.size(v) - 1) // 2]


def stein_parts(x, g, wide):
    "-> (r2 [S, S], t [S, S], C [S, S], d, nonfinite) in np.longdouble (difference form) or float64 (anchor / Gram form)"
    with np.errstate(all="ignore"):                      # (a NaN or Inf input is counted; its arithmetic is of no interest)
        return _stein_parts(x, g, wide)


def _stein_parts(x, g, wide):
    pairs = _pairs(x, g)
    S = pairs[0][0].shape[0]
    dtype = LD if wide else np.float64
    r2, t, C = (np.zeros((S, S), dtype) for _ in range(3))
    A, B = np.zeros((S, S), dtype), np.zeros((S, S), dtype)
    d = bad = 0
    for xa, ga in pairs:
        bad += int((~np.isfinite(xa)).sum() + (~np.isfinite(ga)).sum())
        d += xa.shape[1]
        xw, gw = xa.astype(dtype), ga.astype(dtype)
        if wide:
            for i in range(S):
                dx, dg = xw[i] - xw, gw[i] - gw
                r2[i] += (dx * dx).sum(axis=1)
                t[i] += (dg * dx).sum(axis=1)
                C[i] += (gw[i] * gw).sum(axis=1)
        else:
            xt = xw - xw[0]
            A, B, C = A + xt @ xt.T, B + xt @ gw.T, C + gw @ gw.T     # the Gram matrices are added in key order
    if not wide:
        a, b = np.diag(A), np.diag(B)
        iu = np.triu_indices(S)
        r2[iu] = np.maximum(0, (a[iu[0]] + a[iu[1]]) - 2 * A[iu])
        t[iu] = ((b[iu[0]] - B[iu]) - B.T[iu]) + b[iu[1]]
        r2, t = np.triu(r2) + np.triu(r2, 1).T, np.triu(t) + np.triu(t, 1).T       # evaluated at (min, max), mirrored
        C = np.triu(C) + np.triu(C, 1).T
    return r2, t, C, d, bad


def stein_matrix(x, g, c=1.0, beta=-0.5, wide=True):
    """-> dict(K, r2, c2, d, nonfinite): K_ij = u^beta C_ij - 2 beta u^(beta - 1) (t_ij + d) - 4 beta (beta - 1)
    u^(beta - 2) r2_ij with u = c^2 + r2_ij; c = "median": c^2 is the lower median of r2 over i < j."""
    r2, t, C, d, bad = stein_parts(x, g, wide)
    dtype = r2.dtype.type
    S = r2.shape[0]
    c2 = lower_median(r2[np.triu_indices(S, 1)]) if isinstance(c, str) else dtype(c) * dtype(c)
    beta = dtype(beta)
    with np.errstate(all="ignore"):
        u = c2 + r2
        p0 = 1 / np.sqrt(u) if beta == -0.5 else u ** beta
        p1 = p0 / u
        p2 = p1 / u
        K = (p0 * C - (2 * beta) * p1 * (t + d)) - (4 * beta * (beta - 1)) * p2 * r2
    if bad:
        K, r2 = np.full_like(K, np.nan), np.full_like(r2, np.nan)
    return dict(K=K, r2=r2, c2=c2, d=d, nonfinite=bad)


def ksd_stats(K):
    S = K.shape[0]
    total = K.sum()
    with np.errstate(invalid="ignore"):
        v = total / (S * S)
        return dict(v_stat=v, u_stat=(total - np.trace(K)) / (S * (S - 1)), ksd=np.sqrt(v), row_mean=K.sum(axis=1) / S)


def quadratic_forms(K, W):
    "Q_r = W_r^T K W_r / S^2 for W [R, S]"
    W = np.asarray(W, K.dtype)
    return np.einsum("ri,ri->r", W @ K, W) / (K.shape[0] ** 2)


def sign_process(u, flip_prob=0.5):
    """u [R, S] uniforms -> the +-1 Markov chains: W_r0 = -1 if u_r0 < 1/2, and W_rt = -W_r,t-1 if u_rt < flip_prob"""
    p = np.full(u.shape[1], flip_prob)
    p[0] = 0.5
    return np.cumprod(np.where(u < p, -1.0, 1.0), axis=1)


def p_value(null, observed):
    return (1 + int((np.asarray(null) >= observed).sum())) / (len(null) + 1)


def wild_bootstrap(K, signs):
    v = ksd_stats(K)["v_stat"]
    null = quadratic_forms(K, signs)
    return dict(v_stat=v, null=null, p=p_value(null, v))


def thin(K, m):
    """Stein thinning with the running sums: pi_m = argmin_j [K_jj / 2 + sum_{a < m} K(pi_a, j)] (the first index on a tie),
    total_m = total_{m-1} + (2 sum_{a < m} K(pi_a, pi_m) + K(pi_m, pi_m)), path_m = sqrt(total_m) / m."""
    S = K.shape[0]
    half, run = K.diagonal() / 2, np.zeros(S, K.dtype)
    total = K.dtype.type(0)
    idx, path = np.zeros(m, np.int64), np.zeros(m, K.dtype)
    with np.errstate(invalid="ignore"):
        for a in range(m):
            obj = half + run
            p = int(np.argmin(np.where(np.isnan(obj), np.inf, obj))) if not np.isnan(obj).all() else 0
            total = total + (2 * run[p] + K[p, p])
            idx[a], path[a] = p, np.sqrt(total) / (a + 1)
            run = run + K[p]
    return idx, path
