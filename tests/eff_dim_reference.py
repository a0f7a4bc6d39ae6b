"""Numpy restatement of include/sgmcmc_hip.h, "Lanczos": the step of full reorthogonalisation, the implicit QL eigensolver of
a symmetric tridiagonal matrix, the Ritz vectors, the "positive" rule and N_eff.  ``wide=True`` computes in longdouble
(where numpy has one wider than float64), ``wide=False`` in float64: the difference of the two is the rounding error that the
tests' tolerances are measured from.  Sums run chunk by chunk (CHUNK coordinates per partial sum, the partials added in
chunk order); the order inside a chunk is numpy's, not the kernels', which is what the factor in the tests allows for."""
import math

import numpy as np

CHUNK = 256
MAX_SWEEPS = 60
WIDE = np.longdouble
HAS_WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def _t(wide):
    return WIDE if wide else np.float64


def dot(a, b, wide=False):
    "sum_i a_i b_i: one partial sum per chunk of CHUNK coordinates, the partials added in chunk order"
    T = _t(wide)
    a, b = np.asarray(a, T), np.asarray(b, T)
    total = T(0)
    for c in range(0, a.shape[0], CHUNK):
        total = total + np.sum(a[c:c + CHUNK] * b[c:c + CHUNK], dtype=T)
    return total


def dots(V, w, wide=False):
    "c_k = V_k . w for every row of V, by ``dot``'s order"
    T = _t(wide)
    V, w = np.asarray(V, T), np.asarray(w, T)
    total = np.zeros(V.shape[0], T)
    for c in range(0, w.shape[0], CHUNK):
        total = total + (V[:, c:c + CHUNK] * w[None, c:c + CHUNK]).sum(axis=1, dtype=T)
    return total


def gs_pass(V, w, wide=False):
    "one pass of classical Gram-Schmidt: c = V w, then w - sum_k c_k V_k with k ascending -> (c, w)"
    T = _t(wide)
    V, w = np.asarray(V, T), np.asarray(w, T).copy()
    c = dots(V, w, wide)
    for k in range(V.shape[0]):
        w = w - c[k] * V[k]
    return c, w


def step(V, w, scale, rtol, wide=False, restart=False):
    """The arithmetic of one step on the rows V [j + 1, D] and w = A V_j -> dict(c1, c2, alpha, beta, scale, ok, v_next,
    norm_before).  ``restart``: w is a fresh vector; no alpha, scale unchanged, ok = norm after > rtol * norm before."""
    T = _t(wide)
    V, w = np.asarray(V, T), np.asarray(w, T)
    before = np.sqrt(dot(w, w, wide))
    c1, w = gs_pass(V, w, wide)
    c2, w = gs_pass(V, w, wide)
    beta = np.sqrt(dot(w, w, wide))
    alpha = c1[-1] + c2[-1]
    if restart:
        ok = bool(beta > T(rtol) * before)
        alpha = T(0)
    else:
        scale = max(T(scale), abs(alpha), beta)
        ok = bool(beta > T(rtol) * scale)
    v_next = w * (T(1) / beta) if ok else np.zeros_like(w)
    return dict(c1=c1, c2=c2, alpha=alpha, beta=beta if ok else T(0), norm=beta, scale=scale, ok=ok, v_next=v_next,
                norm_before=before)


def default_rtol(D):
    return 64 * 2.0 ** -52 * np.sqrt(D)


def lanczos(A, n_steps, v0=None, seed=0, rtol=None, wide=False):
    """``n_steps`` steps on the symmetric matrix A -> dict(alpha, beta, V, m, restarts).  Restart vectors come from numpy's
    generator (the device draws other numbers: after a restart only invariants compare)."""
    T = _t(wide)
    A = np.asarray(A, T)
    D = A.shape[0]
    m = min(n_steps, D)
    rtol = default_rtol(D) if rtol is None else rtol
    rng = np.random.default_rng(seed)
    v = np.asarray(rng.standard_normal(D) if v0 is None else v0, T)
    V = np.zeros((m, D), T)
    V[0] = v / np.sqrt(dot(v, v, wide))
    alpha, beta = np.zeros(m, T), np.zeros(m, T)
    scale, restarts = T(0), 0
    for j in range(m):
        r = step(V[:j + 1], A @ V[j], scale, rtol, wide)
        alpha[j], beta[j], scale = r["alpha"], r["beta"], r["scale"]
        if j + 1 == m:
            break
        if r["ok"]:
            V[j + 1] = r["v_next"]
            continue
        for _ in range(3):
            r = step(V[:j + 1], rng.standard_normal(D), scale, rtol, wide, restart=True)
            if r["ok"]:
                break
        else:
            raise RuntimeError("no restart vector survived")
        V[j + 1] = r["v_next"]
        restarts += 1
    return dict(alpha=alpha, beta=beta, V=V, m=m, restarts=restarts)


def tridiag_eig(alpha, beta, wide=False, vectors=True):
    """Implicit QL with Wilkinson shifts on the tridiagonal (alpha, beta[:m - 1]) -> (theta ascending with ties by original
    index, Y with the vectors in columns, sweeps, failed).  e_i is negligible when |e_i| <= eps64 (|d_i| + |d_i+1|): the
    float64 epsilon in both precisions, as on the device.  ``vectors=False`` leaves Y out (None): the eigenvalues do not
    depend on it.  The scalars are Python floats (float64) or numpy longdoubles, held in lists."""
    T = _t(wide)
    scalar = T if wide else float
    hyp, csign = (np.hypot, np.copysign) if wide else (math.hypot, math.copysign)
    m = len(alpha)
    d = [scalar(v) for v in np.asarray(alpha, T)]
    e = [scalar(v) for v in np.asarray(beta, T)[:m - 1]] + [scalar(0)]
    Z = np.eye(m, dtype=T) if vectors else None     # Z[i] is eigenvector i (the device's transposed layout)
    eps, one, two, zero = scalar(2.0 ** -52), scalar(1), scalar(2), scalar(0)
    sweeps, failed = 0, False
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for l in range(m):
            it = 0
            while True:
                mm = l
                while mm < m - 1:
                    if abs(e[mm]) <= eps * (abs(d[mm]) + abs(d[mm + 1])):
                        break
                    mm += 1
                if mm == l:
                    break
                if it == MAX_SWEEPS:
                    failed = True
                    break
                it += 1
                sweeps += 1
                g = (d[l + 1] - d[l]) / (two * e[l])
                r = hyp(g, one)
                g = d[mm] - d[l] + e[l] / (g + csign(r, g))
                s, c, p = one, one, zero
                i = mm - 1
                if vectors:
                    f_row = Z[mm].copy()
                while i >= l:
                    f, b = s * e[i], c * e[i]
                    r = hyp(f, g)
                    e[i + 1] = r
                    if r == 0:
                        d[i + 1] -= p
                        e[mm] = zero
                        break
                    s, c = f / r, g / r
                    g = d[i + 1] - p
                    r = (d[i] - g) * s + two * c * b
                    p = s * r
                    d[i + 1] = g + p
                    g = c * r - b
                    if vectors:                         # (the row above is carried, as a thread of the device carries it)
                        zi = Z[i]
                        Z[i + 1] = s * zi + c * f_row
                        f_row = c * zi - s * f_row
                    i -= 1
                if vectors:
                    Z[i + 1] = f_row
                if i < l:
                    d[l] -= p
                    e[l] = g
                    e[mm] = zero
            if failed:
                break
    d = np.array(d, T)
    if failed or not np.all(np.isfinite(d)):
        return np.full(m, np.nan, T), (np.full((m, m), np.nan, T) if vectors else None), sweeps, True
    order = np.argsort(d, kind="stable")
    return d[order], (Z[order].T.copy() if vectors else None), sweeps, False


def positive(theta, m=None):
    "(values, small): a Ritz value <= m eps max|theta| is returned as exactly 1.0 (its vector as zeros)"
    theta = np.asarray(theta)
    m = theta.shape[0] if m is None else m
    small = theta <= m * 2.0 ** -52 * np.max(np.abs(theta))
    return np.where(small, theta.dtype.type(1), theta), small


def ritz(V, Y, cols, theta=None, positive_rule=False, wide=False):
    "U [D, k] = V^T Y[:, cols], each column's sign making Y[0, col] >= 0; with the positive rule the small ones are zeros"
    T = _t(wide)
    V, Y = np.asarray(V, T), np.asarray(Y, T)
    U = V.T @ Y[:, cols]
    U = U * np.where(Y[0, cols] >= 0, T(1), T(-1))[None, :]
    if positive_rule:
        U[:, positive(np.asarray(theta, T))[1][cols]] = 0
    return U


def eff_dim(eigs, alphas, wide=False):
    "(n_eff [..., A], nonpositive [...], nonfinite [...]) of raw eigenvalues [..., k]"
    T = _t(wide)
    eigs = np.asarray(eigs, T)
    alphas = np.atleast_1d(np.asarray(alphas, T))
    fin = np.isfinite(eigs)
    pos = fin & (eigs > 0)
    lam = np.where(pos, eigs, T(1))[..., None]
    terms = np.where(pos[..., None], lam / (lam + alphas), T(0))
    return terms.sum(axis=-2, dtype=T), (fin & ~pos).sum(axis=-1), (~fin).sum(axis=-1)
