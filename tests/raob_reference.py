"""The Rao-Blackwellised regression model's closed forms restated in numpy (the definitions of include/sgmcmc_hip.h,
section "The Rao-Blackwellised regression model"), in any floating dtype: float64 is the RESTATEMENT the kernels are
compared with, ``np.longdouble`` (x87 extended: 64-bit significand) is the reference that says how far a float64
evaluation of these formulas is from the truth.  ``direct_gaussian`` is the independent check: the same log density as
the plain N-variate Gaussian log N(y | 0, s2 f f^T + v I), with its N x N Cholesky factor, in longdouble.

    G = f^T f, c = f^T y, yy = y^T y, A = s2 G + v I = L L^T, w = L^-1 c, b = L^-T w
    log p  = -1/2 [N log 2 pi + (N - F) log v + yy / v + 2 sum log L_aa - (s2 / v) |w|^2]
    d/df_n = -s2 A^-1 f_n + (s2 / v) r_n b,  r_n = y_n - s2 f_n . b
    d/dv   = -1/2 [(N - F) / v - yy / v^2 + |L^-1|_F^2 + (s2 / v^2) |w|^2 + (s2 / v) |b|^2]
    predictive at f*: mean s2 f* . b, variance v s2 |L^-1 f*|^2 + v
    posterior_w(): mean sqrt(s2) b, root sqrt(v) L^-1
"""
import collections

import numpy as np

LOG_2PI = np.longdouble("1.8378770664093454835606594728112352797")

Marginal = collections.namedtuple("Marginal", "ll dv df b L Linv Ainv G c yy w_mean w_root")


def cholesky(A):
    "right-looking Cholesky in A's dtype (numpy's LAPACK has no longdouble); raises on a pivot that is not > 0"
    A = A.copy()
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        if not A[j, j] > 0 or not np.isfinite(A[j, j]):
            raise np.linalg.LinAlgError(f"pivot {j} = {A[j, j]}")
        L[j, j] = np.sqrt(A[j, j])
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L


def lower_inverse(L):
    "X = L^-1 by the forward substitution swept over the columns of L"
    n = L.shape[0]
    X = np.eye(n, dtype=L.dtype)
    for j in range(n):
        X[j, :j + 1] = X[j, :j + 1] / L[j, j]
        X[j + 1:, :j + 1] -= np.outer(L[j + 1:, j], X[j, :j + 1])
    return X


def marginal(f, y, v, s2, dtype=np.float64):
    "every quantity of the state record, the gradients and posterior_w() in ``dtype``; f [N, F], y [N] or [N, 1]"
    f = np.asarray(f, dtype=dtype)
    y = np.asarray(y, dtype=dtype).reshape(-1)
    v, s2 = dtype(v), dtype(s2)
    N, F = f.shape
    G, c, yy = f.T @ f, f.T @ y, y @ y
    A = s2 * G + v * np.eye(F, dtype=dtype)
    L = cholesky(A)
    Linv = lower_inverse(L)
    w = Linv @ c
    b = Linv.T @ w
    Ainv = Linv.T @ Linv
    quad, bb, tr = w @ w, b @ b, (Linv * Linv).sum()
    logdet = 2 * np.log(np.diag(L)).sum()
    ll = -(N * dtype(LOG_2PI) + (N - F) * np.log(v) + yy / v + logdet - (s2 / v) * quad) / 2
    dv = -((N - F) / v - yy / (v * v) + tr + (s2 / (v * v)) * quad + (s2 / v) * bb) / 2
    r = y - s2 * (f @ b)
    df = -s2 * (f @ Ainv) + (s2 / v) * np.outer(r, b)
    return Marginal(ll, dv, df, b, L, Linv, Ainv, G, c, yy, np.sqrt(s2) * b, np.sqrt(v) * Linv)


def predictive(m, f_star, v, s2, dtype=np.float64):
    f_star = np.asarray(f_star, dtype=dtype)
    v, s2 = dtype(v), dtype(s2)
    u = f_star @ m.Linv.T
    return s2 * (f_star @ m.b), (v * s2) * (u * u).sum(1) + v


def direct_gaussian(f, y, v, s2):
    "log N(y | 0, s2 f f^T + v I) through the N x N covariance, in longdouble: O(N^3), for small N"
    ld = np.longdouble
    f = np.asarray(f, dtype=ld)
    y = np.asarray(y, dtype=ld).reshape(-1)
    N = f.shape[0]
    K = ld(s2) * (f @ f.T) + ld(v) * np.eye(N, dtype=ld)
    L = cholesky(K)
    z = lower_inverse(L) @ y
    return -(N * LOG_2PI + 2 * np.log(np.diag(L)).sum() + z @ z) / 2


def case_inputs(N, F, seed=0, dead_column=None, scale=1.0):
    """ReLU-like features (non-negative, about half of them zero) and targets, float64; ``dead_column``: a feature that
    is zero in every row"""
    rng = np.random.default_rng([seed, N, F])
    f = np.maximum(rng.standard_normal((N, F)), 0.0) * scale
    if dead_column is not None:
        f[:, dead_column] = 0.0
    return f, 2.0 * rng.standard_normal((N, 1))


def bound(restated, exact, factor=4, ulps=4):
    """The rule of tests/test_raob.py: a kernel result may differ from the longdouble value by ``factor`` times the
    distance of the float64 restatement from it plus ``ulps`` float64 ulps of the result; for an array both distances are
    max-norms and the ulp is that of the largest entry, which is the scale the entries' rounding errors have (an entry of
    A^-1 f_n or of L^-1 is a sum of terms of that size, whatever the entry's own size)."""
    exact = np.asarray(exact, dtype=np.longdouble)
    dist = float(np.max(np.abs(np.asarray(restated, dtype=np.longdouble) - exact)))
    return factor * dist + ulps * float(np.spacing(np.float64(np.max(np.abs(exact))))), dist


def distance(result, exact):
    return float(np.max(np.abs(np.asarray(result, dtype=np.longdouble) - np.asarray(exact, dtype=np.longdouble))))
