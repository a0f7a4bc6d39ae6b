"""Plain restatement of the calibration and out-of-distribution metrics that ``include/sgmcmc_hip.h`` defines
(``sgmcmc_ensemble_probs`` / ``sgmcmc_calibration_error`` / ``sgmcmc_rank_metrics``; bnn_priors_amd/calibration.py):
the reference's ``ece`` / ``ace`` / ``rmsce`` (bnn_priors/third_party/calibration_error.py) and sklearn's
``roc_auc_score`` / ``average_precision_score`` in numpy fp64, and the same quantities once more in exact rationals
(``exact_gce``, ``exact_auroc_auprc``, ``mann_whitney_auroc``).  Written from the definitions, not from the kernels:
whole-array numpy, no chunks, no scans."""
import math
from fractions import Fraction

import numpy as np
import torch

EPS = np.finfo(np.float64).eps                     # 2^-52, the reference's guard against empty bins
EPS_EXACT = Fraction(1, 2 ** 52)


def _sorted_column(keys, hits):
    "the keys > 0 in stable ascending order, and their hits"
    keys, hits = np.asarray(keys, dtype=np.float64), np.asarray(hits)
    keep = keys > 0
    order = np.argsort(keys[keep], kind="stable")
    return keys[keep][order], hits[keep][order]


def _bin_edges(s, bounds, num_bins):
    """positions 0 = e_0 <= e_1 <= ... <= e_B = m in the sorted column s: bin k is s[e_k : e_{k+1}], np.digitize's bins of
    the upper bounds (given: even; None: the reference's adaptive bounds of num_bins bins)"""
    m = len(s)
    if bounds is None:                 # num_bins <= 1: no upper bound, one bin
        step = m / num_bins if num_bins else 0.0
        bounds = s[np.minimum(np.rint(np.arange(1, max(num_bins, 1)) * step), m - 1).astype(np.int64)]
    return np.concatenate([[0], np.searchsorted(s, bounds, side="left"), [m]])


def np_gce(keys, hits, bounds=None, num_bins=None, l2=False):
    "one column: keys > 0 kept, sorted; bins = ranges of the sorted column between the np.digitize bounds"
    s, h = _sorted_column(keys, hits)
    m = len(s)
    if m == 0:
        return 0.0
    edges = _bin_edges(s, bounds, num_bins)
    err = 0.0
    for a, b in zip(edges[:-1], edges[1:]):
        cnt = float(b - a) + EPS
        e = (float(h[a:b].sum()) / cnt - s[a:b].sum() / cnt) * (cnt / m)
        err += e * e if l2 else abs(e)
    return err


def exact_gce(keys, hits, bounds=None, num_bins=None, l2=False):
    """np_gce's bins with every sum in rationals (the keys are exact doubles, eps is exactly 2^-52): the l1 error, or
    for l2 the sum of squares before the root, as a Fraction.  An empty bin contributes exactly 0 and is skipped."""
    s, h = _sorted_column(keys, hits)
    m = len(s)
    if m == 0:
        return Fraction(0)
    edges = np.unique(_bin_edges(s, bounds, num_bins)).tolist()
    exact = [Fraction(float(v)) for v in s]
    err = Fraction(0)
    for a, b in zip(edges[:-1], edges[1:]):
        cnt = (b - a) + EPS_EXACT
        e = (Fraction(int(h[a:b].sum())) / cnt - sum(exact[a:b], Fraction(0)) / cnt) * (cnt / m)
        err += e * e if l2 else abs(e)
    return err


def _two_columns(probs):
    "calibration_error.py:204-214: a single column p is the binary problem [[1 - p, p]]"
    probs = np.asarray(probs, dtype=np.float64)
    if probs.shape[1] == 1:
        probs = np.stack([1.0 - probs[:, 0], probs[:, 0]], 1)
    return probs


def np_metrics(labels, probs, num_bins=30, datapoints_per_bin=100):
    labels, probs = np.asarray(labels), _two_columns(probs)
    N, C = probs.shape
    pred = probs.argmax(1)
    conf = probs[np.arange(N), pred]
    hit = (pred == labels).astype(np.int64)
    bounds = np.histogram_bin_edges([], bins=num_bins, range=(0.0, 1.0))[1:]
    return {"ece": np_gce(conf, hit, bounds=bounds),
            "ace": sum(np_gce(probs[:, j], (labels == j).astype(np.int64), num_bins=num_bins) / C for j in range(C)),
            "rmsce": math.sqrt(np_gce(conf, hit, num_bins=int(N / datapoints_per_bin), l2=True))}


def exact_metrics(labels, probs, num_bins=30, datapoints_per_bin=100):
    "np_metrics with exact_gce: ece and ace as Fractions, rmsce as the Fraction under the root"
    labels, probs = np.asarray(labels), _two_columns(probs)
    N, C = probs.shape
    pred = probs.argmax(1)
    conf = probs[np.arange(N), pred]
    hit = (pred == labels).astype(np.int64)
    bounds = np.histogram_bin_edges([], bins=num_bins, range=(0.0, 1.0))[1:]
    return {"ece": exact_gce(conf, hit, bounds=bounds),
            "ace": sum(exact_gce(probs[:, j], (labels == j).astype(np.int64), num_bins=num_bins)
                       for j in range(C)) / C,
            "rmsce2": exact_gce(conf, hit, num_bins=int(N / datapoints_per_bin), l2=True)}


def exact_auroc_auprc(s_in, s_out):
    """AUROC as an exact rational (trapezoids in Python ints) and average precision over the distinct thresholds in
    descending order"""
    scores = np.concatenate([s_in, s_out])
    pos = np.concatenate([np.ones(len(s_in), np.int64), np.zeros(len(s_out), np.int64)])
    order = np.argsort(-scores, kind="stable")
    scores, pos = scores[order], pos[order]
    P, Nn = len(s_in), len(s_out)
    last = np.r_[np.nonzero(np.diff(scores))[0], len(scores) - 1]      # the last position of each tie group
    tps = np.cumsum(pos)[last]
    fps = last + 1 - tps
    area2, ap, tp0, fp0 = 0, 0.0, 0, 0
    for tp, fp in zip(tps.tolist(), fps.tolist()):
        area2 += (fp - fp0) * (tp + tp0)
        ap += (tp / P - tp0 / P) * (tp / (tp + fp))
        tp0, fp0 = tp, fp
    return Fraction(area2, 2 * P * Nn), ap


def mann_whitney_auroc(s_in, s_out):
    "(2 #{pos > neg} + #{pos == neg}) / (2 P Nn) by comparing every pair: no order, no thresholds, no trapezoids"
    s_in, s_out = np.asarray(s_in, dtype=np.float64), np.asarray(s_out, dtype=np.float64)
    greater = equal = 0
    for lo in range(0, len(s_in), 1024):           # [1024, Nn] comparisons at a time
        block = s_in[lo:lo + 1024, None]
        greater += int((block > s_out[None, :]).sum())
        equal += int((block == s_out[None, :]).sum())
    return Fraction(2 * greater + equal, 2 * len(s_in) * len(s_out))


def np_ensemble_probs(acc):
    "Categorical(logits=logsumexp_e acc - log E).probs, fp64 on the host"
    a = torch.as_tensor(acc, dtype=torch.float64).cpu()
    lme = a.logsumexp(0) - math.log(a.shape[0])
    return torch.softmax(lme, -1).numpy()
