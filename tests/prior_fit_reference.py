"""The definitions of include/sgmcmc_hip.h ("Fitting the data-driven priors ...") restated in numpy: the same shift, the
same EM iterations, the same equations solved by the same safeguarded Newton steps, in any float type (np.float64, or
np.longdouble to measure what fp64 rounding costs).  Sums are numpy's (pairwise), not the kernels' tile order: the
tolerances of tests/test_prior_fit.py allow for that."""
import numpy as np

PI = "3.14159265358979323846264338327950288"
HALF_LOG_2PI = "0.918938533204672741780329736405617639"


def _c(dtype, num, den=1):
    return dtype(num) / dtype(den)


def digamma(x, dtype=np.float64):
    "recurrence up to x >= 10, then the asymptotic series through B_14"
    x, r = dtype(x), dtype(0)
    while x < 10:
        r -= 1 / x
        x += 1
    f = 1 / (x * x)
    c = lambda n, d=1: _c(dtype, n, d)                                                      # noqa: E731
    t = f * (c(1, 12) - f * (c(1, 120) - f * (c(1, 252) - f * (c(1, 240) - f * (c(1, 132)
        - f * (c(691, 32760) - f * c(1, 12)))))))
    return r + (np.log(x) - dtype(0.5) / x - t)


def trigamma(x, dtype=np.float64):
    x, r = dtype(x), dtype(0)
    while x < 10:
        r += 1 / (x * x)
        x += 1
    f = 1 / (x * x)
    c = lambda n, d=1: _c(dtype, n, d)                                                      # noqa: E731
    t = (f / x) * (c(1, 6) - f * (c(1, 30) - f * (c(1, 42) - f * (c(1, 30) - f * (c(5, 66)
        - f * (c(691, 2730) - f * c(7, 6)))))))
    return r + (1 / x + dtype(0.5) * f + t)


def log_gamma(x, dtype=np.float64):
    x, prod = dtype(x), dtype(1)
    while x < 10:
        prod *= x
        x += 1
    f = 1 / (x * x)
    c = lambda n, d=1: _c(dtype, n, d)                                                      # noqa: E731
    t = (1 / x) * (c(1, 12) - f * (c(1, 360) - f * (c(1, 1260) - f * (c(1, 1680) - f * (c(1, 1188)
        - f * (c(691, 360360) - f * c(1, 156)))))))
    return (((x - dtype(0.5)) * np.log(x) - x) + dtype(HALF_LOG_2PI) + t) - np.log(prod)


def events_of(w, P, event_dim=None, permute=None):
    """w [S, *shape] -> [events, F, P]: ``permute`` and ``event_dim`` as prior.MultivariateT; event_dim None = the
    trailing dimensions that hold P elements (F = 1)"""
    w = np.asarray(w)
    shape = w.shape[1:]
    permute = tuple(range(len(shape))) if permute is None else tuple(permute)
    x = np.transpose(w, (0,) + tuple(1 + p for p in permute))
    if event_dim is None:
        return x.reshape(-1, 1, P)
    D = int(np.prod(x.shape[x.ndim - event_dim:]))
    return x.reshape(-1, D // P, P)


def moments_reference(X, ddof=1, dtype=np.float64):
    "X [n, P] -> dict(n, mean, cov, skew, kurt, var, pooled_mean, pooled_var, pooled_skew, pooled_kurt, bad)"
    X = np.asarray(X)
    n, P = X.shape
    bad = int((~np.isfinite(X)).sum())
    nan = dtype("nan")
    if bad:
        return dict(n=n, bad=bad, mean=np.full(P, nan), cov=np.full((P, P), nan), skew=np.full(P, nan),
                    kurt=np.full(P, nan), var=np.full(P, nan), pooled_mean=nan, pooled_var=nan, pooled_skew=nan,
                    pooled_kurt=nan)
    X = X.astype(dtype)
    c = np.median(X[[0, n // 2, n - 1]], axis=0).astype(dtype)
    d = X - c
    nn = dtype(n)
    s1 = d.sum(0)
    m = s1 / nn
    s2, s3, s4 = (d * d).sum(0) / nn, ((d * d) * d).sum(0) / nn, ((d * d) * (d * d)).sum(0) / nn
    m2 = s2 - m * m
    m3 = (s3 - 3 * m * s2) + 2 * (m * m) * m
    m4 = ((s4 - 4 * m * s3) + 6 * (m * m) * s2) - 3 * (m * m) * (m * m)
    mean = c + m
    pos = m2 > 0
    var = np.where(pos, m2, dtype(0))
    safe = np.where(pos, m2, dtype(1))
    skew = np.where(pos, m3 / (safe * np.sqrt(safe)), nan)
    kurt = np.where(pos, m4 / (safe * safe) - 3, nan)
    C = d.T @ d - np.outer(s1, s1 / nn)
    C[np.diag_indices(P)] = np.where(np.diag(C) > 0, np.diag(C), dtype(0))
    cov = C / (nn - dtype(ddof))
    pm = mean.sum() / dtype(P)
    dl = mean - pm
    d2 = dl * dl
    M2 = (var + d2).sum() / dtype(P)
    M3 = ((m3 + 3 * dl * var) + d2 * dl).sum() / dtype(P)
    M4 = (((m4 + 4 * dl * m3) + 6 * d2 * var) + d2 * d2).sum() / dtype(P)
    return dict(n=n, bad=0, mean=mean, cov=cov, skew=skew, kurt=kurt, var=var, pooled_mean=pm, pooled_var=M2,
                pooled_skew=M3 / (M2 * np.sqrt(M2)) if M2 > 0 else nan,
                pooled_kurt=M4 / (M2 * M2) - 3 if M2 > 0 else nan)


def mvt_loglik(E, mu, S, nu, dtype=np.float64):
    "sum over the events E [events, F, P] of the log density of the t with scatter I_F (x) S and nu degrees of freedom"
    E = np.asarray(E).astype(dtype)
    n_ev, F, P = E.shape
    L = np.linalg.cholesky(np.asarray(S, dtype=np.float64)).astype(dtype) if dtype is np.float64 else _cholesky(S, dtype)
    z = _solve_lower(L, (E - mu).reshape(-1, P).T, dtype)
    M = (z * z).sum(0).reshape(n_ev, F).sum(1)
    return _loglik(M, np.log(np.diag(L)).sum(), nu, n_ev, F, P, dtype)


def _loglik(M, half_log_det, nu, n_ev, F, P, dtype):
    D = dtype(F * P)
    nu = dtype(nu)
    per = ((log_gamma((nu + D) / 2, dtype) - log_gamma(nu / 2, dtype)) - D / 2 * np.log(dtype(PI) * nu)) \
        - dtype(F) * half_log_det
    return dtype(n_ev) * per - (nu + D) / 2 * np.log1p(M / nu).sum()


def _cholesky(S, dtype):
    S = np.asarray(S, dtype=dtype)
    P = S.shape[0]
    L = np.zeros((P, P), dtype=dtype)
    for a in range(P):
        for b in range(a + 1):
            s = S[a, b] - (L[a, :b] * L[b, :b]).sum()
            if a == b:
                if not s > 0:
                    raise np.linalg.LinAlgError("not positive definite")
                L[a, a] = np.sqrt(s)
            else:
                L[a, b] = s / L[b, b]
    return L


def _solve_lower(L, B, dtype):
    "L^-1 B by forward substitution, in dtype"
    P = L.shape[0]
    Z = np.zeros(B.shape, dtype=dtype)
    for a in range(P):
        Z[a] = (B[a] - L[a, :a] @ Z[:a]) / L[a, a]
    return Z


def solve_nu(c, nu0, lo, hi, dtype=np.float64):
    "the root in [lo, hi] of log(nu / 2) - psi(nu / 2) + c, as fit::solve_nu"
    half = dtype(0.5)
    g = lambda nu: (np.log(half * nu) - digamma(half * nu, dtype)) + c                       # noqa: E731
    lo, hi = dtype(lo), dtype(hi)
    if not g(lo) > 0:
        return lo
    if not g(hi) < 0:
        return hi
    a, b, x = lo, hi, min(max(dtype(nu0), lo), hi)
    for _ in range(200):
        gx = g(x)
        if gx > 0:
            a = x
        elif gx < 0:
            b = x
        else:
            return x
        dg = 1 / x - half * trigamma(half * x, dtype)
        xn = x - gx / dg
        if not (xn > a and xn < b):
            xn = half * (a + b)
        if abs(xn - x) <= dtype(1e-15) * xn:
            return xn
        x = xn
    return x


def fit_mvt_reference(E, df_init=5., df_bounds=(2.01, 1e4), max_iter=500, tol=1e-10, dtype=np.float64, plain=False):
    """EM of definition 2 on E [events, F, P].  Returns dict(loc, S, scale_tril, df, loglik, trace, iterations, converged,
    df_at_bound); NaN parameters after a non-finite input or a singular S."""
    E = np.asarray(E)
    n_ev, F, P = E.shape
    nan = dtype("nan")
    failed = dict(loc=np.full(P, nan), S=np.full((P, P), nan), scale_tril=np.full((P, P), nan), df=nan, loglik=nan,
                  trace=np.zeros(0, dtype), iterations=0, converged=False, df_at_bound=False)
    mom = moments_reference(E.reshape(-1, P), ddof=0, dtype=dtype)
    if mom["bad"]:
        return failed
    E = E.astype(dtype)
    D = dtype(F * P)
    nu = dtype(df_init)
    mu = mom["mean"]
    S = mom["cov"] * ((nu - 2) / nu)
    lo, hi = dtype(df_bounds[0]), dtype(df_bounds[1])
    trace, iterations, converged = [], 0, False

    def stats(mu, S, nu):
        L = _cholesky(S, dtype)
        d = E - mu
        z = _solve_lower(L, d.reshape(-1, P).T, dtype)
        M = (z * z).sum(0).reshape(n_ev, F).sum(1)
        return d, M, _loglik(M, np.log(np.diag(L)).sum(), nu, n_ev, F, P, dtype)

    try:
        while True:
            d, M, ll = stats(mu, S, nu)
            if not np.isfinite(ll):
                return dict(failed, trace=np.array(trace, dtype), iterations=iterations)
            if converged or iterations >= max_iter:
                break
            trace.append(ll)
            u = (nu + D) / (nu + M)
            W = dtype(F) * u.sum() if not plain else dtype(F * n_ev)
            A = (u[:, None, None] * d).sum((0, 1))
            B = np.einsum("e,efa,efb->ab", u, d, d)
            step = A / (dtype(F) * u.sum())
            S_new = (B - np.outer(A, step)) / W
            S_new = np.tril(S_new) + np.tril(S_new, -1).T
            _cholesky(S_new, dtype)
            h = (nu + D) / 2
            c = ((1 + (np.log(u) - u).sum() / dtype(n_ev)) + digamma(h, dtype)) - np.log(h)
            nu_new = solve_nu(c, nu, lo, hi, dtype)
            sd = np.sqrt(np.diag(S_new))
            delta = max(abs(nu_new - nu) / nu_new, (abs(step) / sd).max(), (abs(S_new - S) / np.outer(sd, sd)).max())
            mu, S, nu = mu + step, S_new, nu_new
            iterations += 1
            converged = bool(delta <= tol)
    except np.linalg.LinAlgError:
        return dict(failed, trace=np.array(trace, dtype), iterations=iterations)
    cov = S * (nu / (nu - 2))
    return dict(loc=mu, S=S, scale_tril=_cholesky(cov, dtype), df=nu, loglik=ll, trace=np.array(trace, dtype),
                iterations=iterations, converged=converged, df_at_bound=bool(nu == lo or nu == hi))


def abs_stats_reference(x, loc, beta, dtype=np.float64):
    "(n, zeros, [sum d, sum log d, sum d^beta, sum d^beta log d, sum d^beta log^2 d]) over the d = |x - loc| > 0"
    d = np.abs(np.asarray(x).reshape(-1).astype(dtype) - dtype(loc))
    zeros = int((d == 0).sum())
    d = d[d != 0]
    l = np.log(d)
    p = np.exp(dtype(beta) * l)
    return d.size + zeros, zeros, np.array([d.sum(), l.sum(), p.sum(), (p * l).sum(), ((p * l) * l).sum()], dtype)


def solve_dgamma(s, dtype=np.float64):
    "a with log a - psi(a) = s > 0 (Minka's start and generalised Newton step)"
    s = dtype(s)
    a = (3 - s + np.sqrt((s - 3) * (s - 3) + 24 * s)) / (12 * s)
    for _ in range(100):
        an = 1 / (1 / a + ((np.log(a) - digamma(a, dtype)) - s) / (a * a * (1 / a - trigamma(a, dtype))))
        done = abs(an - a) <= dtype(1e-14) * an
        a = an
        if done:
            break
    return a


def gennorm_profile(beta, n, sums, dtype=np.float64):
    "g(beta) and g'(beta) of the profile score of the generalised normal at a given location"
    beta, n = dtype(beta), dtype(n)
    _, _, sp, spl, spll = sums
    r = spl / sp
    inv = 1 / beta
    la = np.log(beta * sp / n)
    g = ((1 + digamma(inv, dtype) * inv) - r) + la * inv
    dg = (((-digamma(inv, dtype) * inv * inv - trigamma(inv, dtype) * inv * inv * inv) - (spll / sp - r * r))
          + (inv + r) * inv) - la * inv * inv
    return g, dg


def solve_gennorm(stats_at, n, dtype=np.float64):
    "beta by Newton on the profile score from beta = 1; stats_at(beta) -> the five sums; returns (beta, sums at beta)"
    beta = dtype(1)
    for _ in range(100):
        sums = stats_at(beta)
        g, dg = gennorm_profile(beta, n, sums, dtype)
        bn = beta - g / dg
        if not bn > beta / 2:
            bn = beta / 2
        elif bn > 2 * beta:
            bn = 2 * beta
        done = abs(bn - beta) <= dtype(1e-12) * bn
        beta = bn
        if done:
            break
    return beta, stats_at(beta)


def fit_marginal_reference(x, families=("norm", "laplace", "t", "gennorm", "dgamma"), loc=0., dtype=np.float64):
    "{family: (params in scipy's order, mean log-likelihood)} of the elements of x"
    x = np.asarray(x).reshape(-1)
    out = {}
    n, zeros, sums = abs_stats_reference(x, loc, 1.0, dtype)
    nn = dtype(n)
    loc_t = dtype(loc)
    for fam in families:
        if fam == "norm":
            m = moments_reference(x.reshape(-1, 1), ddof=0, dtype=dtype)
            out[fam] = ((m["mean"][0], np.sqrt(m["var"][0])),
                        -(np.log(2 * dtype(PI) * m["var"][0]) + 1) / 2)
        elif fam == "laplace":
            b = sums[0] / nn
            out[fam] = ((loc_t, b), -np.log(2 * b) - 1)
        elif fam == "t":
            f = fit_mvt_reference(x.reshape(-1, 1, 1), dtype=dtype)
            out[fam] = ((f["df"], f["loc"][0], np.sqrt(f["S"][0, 0])), f["loglik"] / nn)
        elif fam == "dgamma":
            if zeros:
                raise ValueError(f"{zeros} elements equal loc")
            m1, ml = sums[0] / nn, sums[1] / nn
            a = solve_dgamma(np.log(m1) - ml, dtype)
            scale = m1 / a
            out[fam] = ((a, loc_t, scale),
                        (((a - 1) * ml - m1 / scale) - np.log(dtype(2))) - log_gamma(a, dtype) - a * np.log(scale))
        elif fam == "gennorm":
            beta, s = solve_gennorm(lambda b: abs_stats_reference(x, loc, b, dtype)[2], n, dtype)
            alpha = np.exp(np.log(beta * s[2] / nn) / beta)
            out[fam] = ((beta, loc_t, alpha),
                        ((np.log(beta) - np.log(2 * alpha)) - log_gamma(1 / beta, dtype)) - 1 / beta)
        else:
            raise ValueError(fam)
    return out


def fit_prior_data_reference(stacks, mean_covs_file, fits_file, dtype=np.float64):
    mean_covs, fits = {}, {}
    for key, w in stacks.items():
        w = np.asarray(w)
        if w.ndim == 5:
            P = w.shape[-1] * w.shape[-2]
            m = moments_reference(w.reshape(-1, P), ddof=1, dtype=dtype)
            mean_covs[key] = (np.asarray(m["mean"], np.float32), np.asarray(m["cov"], np.float64))
        else:
            m = moments_reference(w.reshape(-1, 1), ddof=1, dtype=dtype)
            mean_covs[key] = (np.float64(m["mean"][0]), np.float64(m["cov"][0, 0]))
        fits[key] = {fam: tuple(float(v) for v in p) for fam, (p, _) in
                     fit_marginal_reference(w, ("norm", "laplace", "dgamma"), 0., dtype).items()}
    return {mean_covs_file: mean_covs, fits_file: fits}
