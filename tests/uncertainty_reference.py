"""Plain numpy restatement of the uncertainty decomposition and the risk-coverage curve that ``include/sgmcmc_hip.h``
defines (``sgmcmc_uncertainty_rows`` / ``sgmcmc_risk_coverage``; bnn_priors_amd/uncertainty.py), in a floating-point
type of the caller's choice (``np.float64``, or ``np.longdouble`` to measure what fp64 loses), and the curve once more in
exact rationals.  Written from the definition, not from the kernels: whole-array numpy, no chunks, no scans."""
import itertools
from fractions import Fraction

import numpy as np


def decompose_reference(acc, labels=None, dtype=np.float64):
    """acc [E, N, C] normalised log-probabilities -> dict of probs [N, C], pred, max_prob, margin, entropy,
    expected_entropy, mutual_info, disagreement and, with labels, nll, brier, hit"""
    a = np.asarray(acc, dtype=dtype)
    E, N, C = a.shape
    with np.errstate(all="ignore"):
        m = a.max(0)
        m = np.where(np.isfinite(m), m, 0)
        lme = m + np.log(np.exp(a - m).sum(0)) - np.log(dtype(E))
        z = np.exp(lme - lme.max(-1, keepdims=True))
        probs = z / z.sum(-1, keepdims=True)
        pred = probs.argmax(-1)
        rows = np.arange(N)
        max_prob = probs[rows, pred]
        others = probs.copy()
        others[rows, pred] = -np.inf
        second = others.max(-1) if C > 1 else np.zeros(N, dtype)
        entropy = -np.where(probs == 0, 0, probs * np.log(np.where(probs == 0, 1, probs))).sum(-1)
        plogp = np.where(np.isneginf(a), 0, np.exp(a) * np.where(np.isneginf(a), 0, a))        # [E, N, C]
        expected = -plogp.sum(0).sum(-1) / dtype(E)
        gap = entropy - expected
        disagreement = (a.argmax(-1) != pred).sum(0).astype(dtype) / dtype(E)
        bad = np.isnan(a).any(axis=(0, 2))
        disagreement = np.where(bad, np.nan, disagreement)
        out = {"probs": probs, "pred": pred, "max_prob": max_prob, "margin": max_prob - second, "entropy": entropy,
               "expected_entropy": expected, "mutual_info": np.where(gap < 0, 0, gap), "disagreement": disagreement}
        if labels is not None:
            y = np.asarray(labels)
            onehot = (np.arange(C) == y[:, None]).astype(dtype)
            out["nll"] = -np.log(probs[rows, y])
            out["brier"] = ((probs - onehot) ** 2).sum(-1)
            out["hit"] = (pred == y).astype(np.int64)
    return out


def _groups(scores):
    "stable descending order of the scores and the [a, b) rank ranges of its tie groups"
    s = np.asarray(scores)
    order = np.argsort(-s, kind="stable")
    ss = s[order]
    starts = np.r_[0, np.nonzero(ss[1:] != ss[:-1])[0] + 1, len(s)]
    return order, list(zip(starts[:-1].tolist(), starts[1:].tolist()))


def risk_coverage_reference(scores, losses, dtype=np.float64):
    """(risk [N], aurc, mean loss): cum(k) = A + (k - a) L / (b - a) inside the tie group of ranks (a, b], A the loss sum
    before it and L its own; risk[k - 1] = cum(k) / k"""
    order, groups = _groups(scores)
    loss = np.asarray(losses, dtype=dtype)[order]
    n = len(loss)
    risk = np.empty(n, dtype)
    A = dtype(0)
    for a, b in groups:
        L = loss[a:b].sum()
        k = np.arange(a + 1, b + 1).astype(dtype)
        risk[a:b] = (A + (k - dtype(a)) * L / dtype(b - a)) / k
        A = A + L
    return risk, np.cumsum(risk)[-1] / dtype(n), A / dtype(n)       # (cumsum: added in rank order, as the definition says)


def risk_coverage_exact(scores, losses):
    "the curve in rationals, for losses that are exact in fp64 (0/1): a list of Fraction"
    order, groups = _groups(scores)
    loss = [Fraction(float(v)) for v in np.asarray(losses, dtype=np.float64)[order]]
    risk, A = [], Fraction(0)
    for a, b in groups:
        L = sum(loss[a:b], Fraction(0))
        risk += [(A + (k - a) * L / (b - a)) / k for k in range(a + 1, b + 1)]
        A += L
    return risk


def aurc_exact(risk):
    "the mean of a curve of Fractions (slow beyond a few hundred entries: the denominators grow)"
    return sum(risk, Fraction(0)) / len(risk)


def risk_coverage_enumerated(scores, losses):
    """the definition behind the tie rule, by brute force (small N): the mean, over every order of the rows inside every
    tie group, of the plain curve cumsum(loss) / k -- a list of Fraction"""
    order, groups = _groups(scores)
    loss = [Fraction(float(v)) for v in np.asarray(losses, dtype=np.float64)[order]]
    n = len(loss)
    total, count = [Fraction(0)] * n, 0
    for arrangement in itertools.product(*[itertools.permutations(loss[a:b]) for a, b in groups]):
        seq = [v for grp in arrangement for v in grp]
        run = Fraction(0)
        for k, v in enumerate(seq):
            run += v
            total[k] += run / (k + 1)
        count += 1
    return [t / count for t in total]


def eaurc_reference(scores, losses, dtype=np.float64):
    "aurc minus the aurc of the oracle ordering scores = -losses"
    loss = np.asarray(losses, dtype=dtype)
    return risk_coverage_reference(scores, loss, dtype)[1] - risk_coverage_reference(-loss, loss, dtype)[1]


def random_table(rng, E, N, C, inf_share=0.05):
    """random normalised log-probabilities [E, N, C], about ``inf_share`` of the entries -inf (probability 0), no
    (sample, row) all -inf"""
    f = rng.normal(scale=2.0, size=(E, N, C))
    drop = rng.random((E, N, C)) < inf_share
    drop[..., 0] &= ~drop.all(-1)                   # keep one class alive
    f[drop] = -np.inf
    with np.errstate(divide="ignore"):
        return f - np.log(np.exp(f).sum(-1, keepdims=True))
