"""The definition of the rank-normalised R-hat with bulk and tail ESS (include/sgmcmc_hip.h, "Rank-normalised R-hat")
restated in numpy fp64 -- written from the definition, not from the kernels: ranks from ``scipy.stats.rankdata``, the
normal quantile function from ``scipy.special.ndtri``, the quantile formula spelled out one rounding at a time, and
R-hat / ESS of the resulting [J, n, Q] arrays from ``chain_diag_reference(., split=False)``.

    x[m][s][q] -> RankResult(rhat, ess_bulk, ess_tail, rhat_bulk, rhat_folded, ess_lower, ess_upper, median, q_lower,
                             q_upper, z, z_folded, ind_lower, ind_upper, pairs_bulk, pairs_lower, pairs_upper,
                             margin_bulk, margin_tail)

``z`` / ``z_folded`` / ``ind_*`` are [J, n, Q] (NaN for a quantity with a non-finite draw).  ``margin_bulk`` is the margin (chain_diag_reference) of the bulk ESS,
``margin_tail`` the smaller margin of the two indicators' ESS: a comparison against another implementation may leave
out quantities whose margin is at rounding level."""
import collections

import numpy as np
import scipy.special
import scipy.stats

from chain_diag_reference import chain_diag_reference, sequences

RankResult = collections.namedtuple(
    "RankResult", "rhat ess_bulk ess_tail rhat_bulk rhat_folded ess_lower ess_upper median q_lower q_upper "
                  "z z_folded ind_lower ind_upper pairs_bulk pairs_lower pairs_upper margin_bulk margin_tail")


def average_ranks(v):
    "v [N, Q] -> r [N, Q]: #{j : v_j < v_i} + (#{j : v_j = v_i} + 1) / 2 down every column (-0.0 = 0.0)"
    return scipy.stats.rankdata(v, method="average", axis=0)


def normal_scores(v):
    "v [N, Q] -> z [N, Q] = ndtri((r - 3/8) / (N + 1/4)); numerator and denominator are exact, one division"
    N = v.shape[0]
    return scipy.special.ndtri((average_ranks(v) - 0.375) / (N + 0.25))


def quantile(v, p):
    """type 7 (numpy's 'linear') down every column of v [N, Q], each operation rounded once, interpolating from the
    nearer neighbour as numpy does"""
    N = v.shape[0]
    ordered = np.sort(v, axis=0)
    pos = (N - 1) * p
    lo = int(np.floor(pos))
    hi = min(lo + 1, N - 1)
    frac = pos - lo
    diff = ordered[hi] - ordered[lo]
    if frac >= 0.5:
        rest = 1.0 - frac
        return ordered[hi] - diff * rest
    return ordered[lo] + diff * frac


def rank_diag_reference(x, split=True, tail_probs=(0.05, 0.95)):
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    seq = sequences(x, split) + 0.0                       # [J, n, Q]; -0.0 counts as, and is written as, +0.0
    J, n, Q = seq.shape
    N = J * n
    v = seq.reshape(N, Q)                                 # the draws in sequence order
    bad = ~np.isfinite(v).all(axis=0)
    v = np.where(bad, 0.0, v)                             # ranked as zeros, NaN in every result below
    with np.errstate(all="ignore"):
        median, q_lower, q_upper = quantile(v, 0.5), quantile(v, tail_probs[0]), quantile(v, tail_probs[1])
        folded = np.abs(v - median)
        bad_folded = bad | ~np.isfinite(folded).all(axis=0)
        z = normal_scores(v).reshape(J, n, Q)
        z_folded = normal_scores(np.where(bad_folded, 0.0, folded)).reshape(J, n, Q)
        ind_lower = (v <= q_lower).astype(np.float64).reshape(J, n, Q)
        ind_upper = (v <= q_upper).astype(np.float64).reshape(J, n, Q)
        bulk = chain_diag_reference(z, split=False)
        fold = chain_diag_reference(z_folded, split=False)
        lower = chain_diag_reference(ind_lower, split=False)
        upper = chain_diag_reference(ind_upper, split=False)
        rhat_bulk, ess_bulk, rhat_folded = bulk.rhat.copy(), bulk.ess.copy(), fold.rhat.copy()
        ess_lower, ess_upper = lower.ess.copy(), upper.ess.copy()
        margin_bulk, margin_tail = bulk.margin.copy(), np.minimum(lower.margin, upper.margin)
        nan = np.nan
        for a in (rhat_bulk, ess_bulk, ess_lower, ess_upper, median, q_lower, q_upper):
            a[bad] = nan
        rhat_folded[bad_folded] = nan
        z[:, :, bad] = nan
        ind_lower[:, :, bad] = nan                        # the indicators of such a quantity are not defined
        ind_upper[:, :, bad] = nan
        z_folded[:, :, bad_folded] = nan
        margin_bulk[bad] = np.inf
        margin_tail[bad] = np.inf
        rhat = np.where(np.isnan(rhat_bulk) | np.isnan(rhat_folded), nan, np.maximum(rhat_bulk, rhat_folded))
        ess_tail = np.where(np.isnan(ess_lower) | np.isnan(ess_upper), nan, np.minimum(ess_lower, ess_upper))
    return RankResult(rhat, ess_bulk, ess_tail, rhat_bulk, rhat_folded, ess_lower, ess_upper, median, q_lower, q_upper,
                      z, z_folded, ind_lower, ind_upper, np.where(bad, 0, bulk.pairs), np.where(bad, 0, lower.pairs),
                      np.where(bad, 0, upper.pairs), margin_bulk, margin_tail)
