"""The definition of the posterior summaries with Monte Carlo standard errors (include/sgmcmc_hip.h, "Posterior
summaries") restated in numpy fp64 -- written from the definition, not from the kernels: ``np.sort`` for the order
statistics, plain numpy means, ``scipy.special.betaincinv`` for the inverse incomplete beta function, the quantile formula
of ``rank_diag_reference.quantile`` and the ESS of ``chain_diag_reference``.

    x[m][s][q] -> SummaryResult(mean, sd, mcse_mean, mcse_sd, ess_mean, ess_sd, quantiles, mcse_quantile, ess_quantile,
                                hdi_lower, hdi_upper, m2, m4, a, b, lo, hi, ordered, csq, margin_mean, margin_sd,
                                margin_quantile, margin_rank)

``ordered`` is [N, Q] and ``csq`` [J, n, Q] (NaN for a quantity with a non-finite draw); the per-probability results are
[P, Q].  ``margin_mean`` / ``margin_sd`` / ``margin_quantile`` are the margins (chain_diag_reference) of the three kinds
of ESS; ``margin_rank`` [P, Q] is how far a N and b N are from an integer, the discrete decision behind lo and hi.  A
comparison against another implementation may leave out quantities whose margin is at the level of that
implementation's error."""
import collections
import math

import numpy as np
import scipy.special

from chain_diag_reference import chain_diag_reference, sequences
from rank_diag_reference import quantile

LOWER_TAIL, UPPER_TAIL = 0.1586553, 0.8413447             # Phi(-1), Phi(1) as posterior::mcse_quantile writes them

SummaryResult = collections.namedtuple(
    "SummaryResult", "mean sd mcse_mean mcse_sd ess_mean ess_sd quantiles mcse_quantile ess_quantile hdi_lower hdi_upper "
                     "m2 m4 a b lo hi ordered csq margin_mean margin_sd margin_quantile margin_rank")


def beta_ranks(ess_q, p, N):
    """ess_q [Q] -> (a, b, lo, hi, margin): the beta quantiles, the two ranks (0-based; -1 where ess_q is NaN) and the
    distance of a N and b N from the nearest integer (inf where ess_q is NaN)"""
    ok = np.isfinite(ess_q)
    e = np.where(ok, ess_q, 1.0)
    alpha, beta = e * p + 1.0, e * (1.0 - p) + 1.0
    a = scipy.special.betaincinv(alpha, beta, LOWER_TAIL)
    b = scipy.special.betaincinv(alpha, beta, UPPER_TAIL)
    aN, bN = a * N, b * N
    lo = np.maximum(np.floor(aN), 1.0).astype(np.int64) - 1
    hi = np.minimum(np.ceil(bN), float(N)).astype(np.int64) - 1
    margin = np.minimum(np.abs(aN - np.round(aN)), np.abs(bN - np.round(bN)))
    nan = np.nan
    return (np.where(ok, a, nan), np.where(ok, b, nan), np.where(ok, lo, -1).astype(np.int32),
            np.where(ok, hi, -1).astype(np.int32), np.where(ok, margin, np.inf))


def hdi(ordered, mass):
    "ordered [N, Q] ascending -> (lower, upper): the narrowest window of floor(mass N) + 1 order statistics, the first one"
    N = ordered.shape[0]
    k = math.floor(mass * N)
    assert 1 <= k <= N - 1
    first = (ordered[k:] - ordered[:N - k]).argmin(axis=0)        # argmin returns the first minimum
    cols = np.arange(ordered.shape[1])
    return ordered[first, cols], ordered[first + k, cols]


def exact_moments(v):
    """v [N, Q] finite -> (mean, m2, m4) with every sum by ``math.fsum`` (correctly rounded), the yardstick of the
    summation error of any implementation"""
    N, Q = v.shape
    mean, m2, m4 = np.empty(Q), np.empty(Q), np.empty(Q)
    for q in range(Q):
        col = v[:, q]
        mean[q] = col[0] if (col == col[0]).all() else math.fsum(col) / N
        c2 = (col - mean[q]) ** 2
        m2[q] = math.fsum(c2) / N
        m4[q] = math.fsum(c2 * c2) / N
    return mean, m2, m4


def summary_reference(x, probs=(0.05, 0.5, 0.95), hdi_prob=0.94, split=True):
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    seq = sequences(x, split) + 0.0                       # [J, n, Q]; -0.0 counts as, and is written as, +0.0
    J, n, Q = seq.shape
    N, P = J * n, len(probs)
    v = seq.reshape(N, Q)                                 # the draws in sequence order
    bad = ~np.isfinite(v).all(axis=0)
    v = np.where(bad, 0.0, v)                             # summarised as zeros, NaN in every result below
    nan = np.nan
    with np.errstate(all="ignore"):
        ordered = np.sort(v, axis=0)
        constant = (v == v[0]).all(axis=0)
        mean = np.where(constant, v[0], v.sum(axis=0) / N)
        c = v - mean
        csq = c * c
        m2, m4 = csq.sum(axis=0) / N, (csq * csq).sum(axis=0) / N
        sd = np.sqrt(m2 * N / (N - 1))
        flat = bad | (m2 == 0.0)                          # no ess and no mcse
        of_mean = chain_diag_reference(v.reshape(J, n, Q), split=False)
        of_sd = chain_diag_reference(csq.reshape(J, n, Q), split=False)
        ess_mean, ess_sd = np.where(flat, nan, of_mean.ess), np.where(flat, nan, of_sd.ess)
        mcse_mean = sd / np.sqrt(ess_mean)
        mcse_sd = np.sqrt((m4 - m2 * m2) / ess_sd / m2 / 4.0)
        quantiles, ess_q, margin_q = np.empty((P, Q)), np.empty((P, Q)), np.empty((P, Q))
        a, b, mcse_q, margin_rank = (np.empty((P, Q)) for _ in range(4))
        lo, hi = np.empty((P, Q), dtype=np.int32), np.empty((P, Q), dtype=np.int32)
        cols = np.arange(Q)
        for k, p in enumerate(probs):
            quantiles[k] = quantile(v, p)
            of_q = chain_diag_reference((v <= quantiles[k]).astype(np.float64).reshape(J, n, Q), split=False)
            ess_q[k] = np.where(bad, nan, of_q.ess)
            margin_q[k] = np.where(bad, np.inf, of_q.margin)
            a[k], b[k], lo[k], hi[k], margin_rank[k] = beta_ranks(ess_q[k], p, N)
            mcse_q[k] = np.where(lo[k] < 0, nan, (ordered[hi[k], cols] - ordered[lo[k], cols]) / 2.0)
        hdi_lower, hdi_upper = hdi(ordered, hdi_prob)
        for arr in (mean, sd, m2, m4, hdi_lower, hdi_upper):
            arr[bad] = nan
        quantiles[:, bad] = nan
        ordered[:, bad] = nan
        csq[:, bad] = nan
    return SummaryResult(mean, sd, mcse_mean, mcse_sd, ess_mean, ess_sd, quantiles, mcse_q, ess_q, hdi_lower, hdi_upper,
                         m2, m4, a, b, lo, hi, ordered, csq.reshape(J, n, Q), np.where(flat, np.inf, of_mean.margin),
                         np.where(flat, np.inf, of_sd.margin), margin_q, margin_rank)
