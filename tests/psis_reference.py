"""The definition of PSIS-LOO and WAIC (include/sgmcmc_hip.h, "Model comparison") restated in numpy fp64 -- written from
the definition, not from the kernels: a sort where the kernels count, one column at a time.

Per column of ``ll [S, N]`` (log p(y_i | theta_s)), with r = -ll:
 1. x_s = r_s - max_s r_s
 2. M = ceil(min(0.2 S, 3 sqrt(S / r_eff))), at most 544; cut = max(x_(S-M-1), log DBL_MIN); ec = exp(cut)
 3. the tail: the draws with x_s > cut, n2 of them, ascending, ties by draw index; n2 <= 4: khat = +inf, no smoothing
 4. t_j = exp(x_tail_j) - ec and the Zhang-Stephens (2009) fit: m = 30 + floor(sqrt(n2)),
    b_j = 1 / t_(n2-1) + (1 - sqrt(m / (j - 1/2))) / (3 t_(floor(n2/4 + 1/2) - 1)), kappa_j = mean log1p(-b_j t),
    L_j = n2 (log(-b_j / kappa_j) - kappa_j - 1), w_j = 1 / sum_l exp(L_l - L_j), bbar = sum b_j w_j,
    kappa = mean log1p(-bbar t), sigma = -kappa / bbar, khat = (n2 kappa + 5) / (n2 + 10)
 5. khat finite: tail element j becomes log(sigma expm1(-khat log1p(-p_j)) / khat + ec), p_j = (j + 1/2) / n2
    (khat = 0: log(-sigma log1p(-p_j) + ec))
 6. x <- min(x, 0); lw = x - logsumexp x
and pareto_k = khat, elpd_loo = logsumexp(lw + ll), lppd = logsumexp ll - log S, p_loo = lppd - elpd_loo, p_waic =
var(ll, ddof=1) in two passes, elpd_waic = lppd - p_waic.  A column with a non-finite ll (or an r_eff that is not a
positive finite number) is NaN in every output, with M = n2 = 0.

``total`` is the function every sum of the restatement goes through: ``np.sum`` (numpy's pairwise order) by default,
``math.fsum`` (exactly rounded) to measure how much the order of summation can matter.

    psis_reference(ll, r_eff=None) -> PsisResult of [N] arrays (``lw`` [S, N]; ``tail_pos`` [S, N]: a tail draw's
    ascending position j, -1 outside the tail)
    totals(result, S) -> dict of the totals
"""
import collections
import math

import numpy as np

LOG_DBL_MIN = float(np.log(np.finfo(np.float64).tiny))
MAX_TAIL = 544
FIELDS = ("pareto_k", "elpd_loo", "lppd", "p_loo", "p_waic", "elpd_waic")
PsisResult = collections.namedtuple("PsisResult", FIELDS + ("sigma", "cut", "M", "n2", "lw", "tail_pos"))


def tail_length(S, r_eff=1.0):
    return min(int(np.ceil(min(0.2 * S, 3.0 * np.sqrt(S / r_eff)))), MAX_TAIL)


def k_threshold(S):
    return min(1.0 - 1.0 / math.log10(S), 0.7)


def logsumexp(v, total=np.sum):
    mx = v.max()
    return mx + np.log(total(np.exp(v - mx)))


def gpd_fit(t, total=np.sum):
    "t: the exceedances in ascending order -> (khat, sigma)"
    n2 = len(t)
    m = 30 + int(np.floor(np.sqrt(n2)))
    j = np.arange(1, m + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        b = 1.0 / t[n2 - 1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * t[int(np.floor(n2 / 4 + 0.5)) - 1])
        kap = np.array([total(np.log1p(-bj * t)) / n2 for bj in b])
        L = n2 * (np.log(-b / kap) - kap - 1.0)
        w = np.array([1.0 / total(np.exp(L - Lj)) for Lj in L])
        bbar = total(b * w)
        kappa = total(np.log1p(-bbar * t)) / n2
        return (n2 * kappa + 5.0) / (n2 + 10.0), -kappa / bbar


def psis_column(ll, r_eff=1.0, total=np.sum):
    "one column -> dict of its outputs"
    ll = np.asarray(ll, dtype=np.float64)
    S = len(ll)
    nan = np.nan
    if not (np.isfinite(ll).all() and np.isfinite(r_eff) and r_eff > 0):
        return dict(pareto_k=nan, elpd_loo=nan, lppd=nan, p_loo=nan, p_waic=nan, elpd_waic=nan, sigma=nan, cut=nan,
                    M=0, n2=0, lw=np.full(S, nan), tail_pos=np.full(S, -1))
    r = -ll
    x = r - r.max()
    M = tail_length(S, r_eff)
    cut = max(np.sort(x)[S - M - 1], LOG_DBL_MIN)
    ec = np.exp(cut)
    tail = np.flatnonzero(x > cut)
    tail = tail[np.argsort(x[tail], kind="stable")]              # ascending, ties by draw index
    n2 = len(tail)
    tail_pos = np.full(S, -1)
    tail_pos[tail] = np.arange(n2)
    khat, sigma = np.inf, nan
    if n2 > 4:
        khat, sigma = gpd_fit(np.exp(x[tail]) - ec, total)
        if np.isfinite(khat):
            l1 = np.log1p(-((np.arange(n2) + 0.5) / n2))
            with np.errstate(all="ignore"):
                g = -sigma * l1 if khat == 0 else sigma * np.expm1(-khat * l1) / khat
                x = x.copy()
                x[tail] = np.log(g + ec)
    x = np.minimum(x, 0.0)
    lw = x - logsumexp(x, total)
    elpd = logsumexp(lw + ll, total)
    lppd = logsumexp(ll, total) - np.log(float(S))
    mean = total(ll) / S
    p_waic = total((ll - mean) ** 2) / (S - 1)
    return dict(pareto_k=khat, elpd_loo=elpd, lppd=lppd, p_loo=lppd - elpd, p_waic=p_waic, elpd_waic=lppd - p_waic,
                sigma=sigma, cut=cut, M=M, n2=n2, lw=lw, tail_pos=tail_pos)


def psis_reference(ll, r_eff=None, total=np.sum):
    ll = np.asarray(ll, dtype=np.float64)
    ll = ll.reshape(-1, ll.shape[-1])
    S, N = ll.shape
    r_eff = np.ones(N) if r_eff is None else np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (N,))
    cols = [psis_column(ll[:, i], r_eff[i], total) for i in range(N)]
    out = {k: np.array([c[k] for c in cols]) for k in FIELDS + ("sigma", "cut")}
    out.update({k: np.array([c[k] for c in cols], dtype=np.int64) for k in ("M", "n2")})
    out["lw"] = np.stack([c["lw"] for c in cols], axis=1)
    out["tail_pos"] = np.stack([c["tail_pos"] for c in cols], axis=1)
    return PsisResult(**out)


def se(v):
    "sqrt(N var(v, ddof=1)): the standard error of sum_i v_i"
    v = np.asarray(v, dtype=np.float64)
    if len(v) < 2:
        return float("nan")
    with np.errstate(all="ignore"):
        return float(np.sqrt(len(v) * np.var(v, ddof=1)))


def totals(res, S):
    k = res.pareto_k
    with np.errstate(all="ignore"):
        return dict(elpd_loo=float(res.elpd_loo.sum()), se_loo=se(res.elpd_loo), p_loo=float(res.p_loo.sum()),
                    lppd=float(res.lppd.sum()), elpd_waic=float(res.elpd_waic.sum()), se_waic=se(res.elpd_waic),
                    p_waic=float(res.p_waic.sum()), n_bad=float((k > k_threshold(S)).sum()),
                    k_max=float(np.nan if np.isnan(k).any() else k.max()))


def compare(pointwise):
    "{name: pointwise [N]} -> [(name, elpd, elpd_diff, dse)] best first"
    elpd = {n: float(np.sum(v)) for n, v in pointwise.items()}
    names = sorted(pointwise, key=lambda n: -elpd[n])
    best = pointwise[names[0]]
    return [(n, elpd[n], elpd[n] - elpd[names[0]], 0.0 if n == names[0] else se(pointwise[n] - best)) for n in names]
