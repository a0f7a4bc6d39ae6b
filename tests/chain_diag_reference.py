"""The definition of split-R-hat and the effective sample size (include/sgmcmc_hip.h, "Between-chain diagnostics")
restated in numpy fp64 -- written from the definition, not from the kernels: plain means and sums in numpy's own order.

    x[m][s][q] -> Result(rhat [Q], ess [Q], pairs [Q], margin [Q])

``pairs`` is K.  ``margin`` is how far the quantity's discrete decisions are from flipping: the smallest ``|P_k|`` met
while looking for K (k = 1 .. K, or .. n/2 - 1 if no pair was non-positive) and the smallest ``|P_k - P'_{k-1}|`` met in
the monotone step (k = 1 .. K - 1).  A comparison against another implementation of the same definition may leave out
quantities whose margin is at rounding level: there K, and with it the ESS, legitimately differ."""
import collections

import numpy as np

Result = collections.namedtuple("Result", "rhat ess pairs margin")


def sequences(x, split=True):
    "x [M, S, Q] -> [J, n, Q]: with split, chain m gives sequence 2m = draws [0, n) and 2m + 1 = draws [S - n, S)"
    M, S, Q = x.shape
    if not split:
        return x
    n = S // 2
    return np.stack([x[:, :n], x[:, S - n:]], axis=1).reshape(2 * M, n, Q)


def chain_diag_reference(x, split=True):
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    seq = sequences(x, split)
    J, n, Q = seq.shape
    assert n >= 4
    half = n // 2
    with np.errstate(all="ignore"):
        mu = seq.mean(axis=1)                                   # [J, Q]
        c = seq - mu[:, None, :]
        acov = np.empty((n, Q))                                 # mean_j a_j[t]
        for t in range(n):
            acov[t] = (np.einsum("jsq,jsq->jq", c[:, :n - t], c[:, t:]) / n).mean(axis=0)
        W = acov[0] * n / (n - 1)
        b_over_n = mu.var(axis=0, ddof=1) if J > 1 else np.zeros(Q)
        varp = W * (n - 1) / n + b_over_n
        rhat = np.sqrt(varp / W)
        rho = 1.0 - (W - acov) / varp
        rho[0] = 1.0
        P = rho[0:2 * half:2] + rho[1:2 * half:2]               # [half, Q]
        nonpos = P[1:] <= 0.0
        K = np.where(nonpos.any(axis=0), nonpos.argmax(axis=0) + 1, half)
        mono = np.minimum.accumulate(P, axis=0)
        tau = -1.0 + 2.0 * np.cumsum(mono, axis=0)[K - 1, np.arange(Q)]
        tau = np.maximum(tau, 1.0 / np.log10(J * n))
        ess = J * n / tau
        k = np.arange(half)[:, None]
        looked = (k >= 1) & (k <= np.minimum(K, half - 1))
        stepped = (k >= 1) & (k < K)
        step_gap = np.abs(P[1:] - mono[:-1])
        margin = np.minimum(np.where(looked, np.abs(P), np.inf).min(axis=0),
                            np.where(stepped[1:], step_gap, np.inf).min(axis=0))
    bad = ~np.isfinite(W) | (W == 0.0)
    rhat[bad] = np.nan
    ess[bad] = np.nan
    K = np.where(bad, 0, K).astype(np.int32)
    margin[bad] = np.inf
    return Result(rhat, ess, K, margin)
