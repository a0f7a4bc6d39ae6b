"""Calibration and out-of-distribution metrics of a posterior ensemble on the device (``csrc/calib_hip.inc``; C ABI
``sgmcmc_ensemble_probs`` / ``sgmcmc_row_max`` / ``sgmcmc_stable_order`` / ``sgmcmc_calibration_error`` /
``sgmcmc_rank_metrics``) -- what the reference computes in numpy on the host after its evaluation loop:

    ece / ace / rmsce      bnn_priors/third_party/calibration_error.py (exp_utils.py:323-327)
    auroc / auprc          sklearn roc_auc_score / average_precision_score of the ensemble's max-probability,
                           in-distribution (positive) against out-of-distribution (exp_utils.py:343-380)

Everything runs in fp64 in an order fixed by the sizes (counts in integers), so two calls give the same bits; each
metric function synchronises with the host once, when it reads its result.

Multi-chain: ``ensemble_across_chains`` returns the cross-chain ``lme`` of ``acc``; ``ensemble_probs(lme.unsqueeze(0),
labels)`` turns it into the ensemble's probabilities (log 1 = 0).
"""
import collections
import functools

import numpy as np
import torch

from . import _hip

__all__ = ("Ensemble", "ensemble_probs", "ece", "ace", "rmsce", "calibration_metrics", "auroc_auprc")

MAX_CLASSES = 128
MAX_ROWS = 131072
MAX_BINS = 4096

Ensemble = collections.namedtuple("Ensemble", "probs conf pred hit")
Ensemble.__doc__ = ("probs [N, C] fp64, conf [N] = max-prob, pred [N] = first argmax (int64), hit [N] = pred == labels "
                    "(int64; None without labels)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor")
    return t


def _labels(labels, probs):
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.shape[0] != probs.shape[0] \
            or labels.dtype.is_floating_point:
        raise ValueError("labels must be an integer [N] tensor matching the probabilities' rows")
    _cuda(labels, "labels")
    if labels.device != probs.device:
        raise ValueError("labels and probabilities are on different devices")
    return labels.to(torch.int64).contiguous()


def _probs(probs):
    if not isinstance(probs, torch.Tensor) or probs.dim() != 2:
        raise ValueError("probs must be an [N, C] tensor")
    n, c = probs.shape
    if not 0 < c <= MAX_CLASSES:
        raise ValueError(f"{c} classes: 1 .. {MAX_CLASSES} are supported")
    if not 0 < n <= MAX_ROWS:
        raise ValueError(f"{n} rows: 1 .. {MAX_ROWS} are supported")
    _cuda(probs, "probs")
    return probs.to(torch.float64).contiguous()


def ensemble_probs(acc, labels=None):
    """acc [E, N, C]: per-sample normalised log-probabilities (``evaluation.predictive_tables``) ->
    ``Ensemble`` of ``softmax(logsumexp_e acc - log E)`` = ``Categorical(logits=lme).probs``, its max-prob, first
    argmax and (with ``labels`` [N]) hits.  One pass over the table, no host synchronisation."""
    if not isinstance(acc, torch.Tensor) or acc.dim() != 3:
        raise ValueError("acc must be an [E, N, C] tensor")
    E, N, C = acc.shape
    if not 0 < C <= MAX_CLASSES:
        raise ValueError(f"{C} classes: 1 .. {MAX_CLASSES} are supported")
    if E == 0 or N == 0 or E >= 2 ** 31 or N >= 2 ** 31:
        raise ValueError("acc needs at least one sample and one row")
    _cuda(acc, "acc")
    acc = acc.to(torch.float64).contiguous()
    dev = acc.device
    if labels is not None:
        _cuda(labels, "labels")
        if labels.shape != (N,) or labels.dtype.is_floating_point or labels.device != dev:
            raise ValueError("labels must be an integer [N] tensor on acc's device")
        labels = labels.to(torch.int64).contiguous()
    probs = torch.empty((N, C), dtype=torch.float64, device=dev)
    conf = torch.empty(N, dtype=torch.float64, device=dev)
    pred = torch.empty(N, dtype=torch.int64, device=dev)
    hit = None if labels is None else torch.empty(N, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        err = _hip.lib().sgmcmc_ensemble_probs(acc.data_ptr(), 0 if labels is None else labels.data_ptr(), E, N, C,
                                               probs.data_ptr(), conf.data_ptr(), pred.data_ptr(),
                                               0 if hit is None else hit.data_ptr(), _stream())
    _hip.check(err, "sgmcmc_ensemble_probs")
    return Ensemble(probs, conf, pred, hit)


def _order(keys, n, ncols, elem_stride, col_stride):
    perm = torch.empty((ncols, n), dtype=torch.int32, device=keys.device)
    _hip.check(_hip.lib().sgmcmc_stable_order(keys.data_ptr(), elem_stride, col_stride, n, ncols, perm.data_ptr(),
                                              _stream()), "sgmcmc_stable_order")
    return perm


@functools.lru_cache(maxsize=16)
def _even_bounds(num_bins, device):
    "np.histogram_bin_edges([], num_bins, (0, 1))[1:], bit for bit (copied to the device once)"
    edges = np.histogram_bin_edges([], bins=num_bins, range=(0.0, 1.0))[1:]
    return torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).to(device)


def _calib(keys, perm, target, class_conditional, n, ncols, elem_stride, col_stride, bounds, num_bins, l2, out):
    col_err = torch.empty(ncols, dtype=torch.float64, device=keys.device)
    err = _hip.lib().sgmcmc_calibration_error(keys.data_ptr(), elem_stride, col_stride, perm.data_ptr(),
                                              target.data_ptr(), int(class_conditional), n, ncols,
                                              0 if bounds is None else bounds.data_ptr(), num_bins, int(l2),
                                              col_err.data_ptr(), out.data_ptr(), _stream())
    _hip.check(err, "sgmcmc_calibration_error")


def _check_bins(num_bins):
    if not 0 <= int(num_bins) <= MAX_BINS:
        raise ValueError(f"num_bins must lie in 0 .. {MAX_BINS}")
    return int(num_bins)


def calibration_metrics(labels, probs, metrics=("ece", "ace", "rmsce"), num_bins=30, datapoints_per_bin=100):
    """The reference's ``ece`` / ``ace`` / ``rmsce`` (calibration_error.py:379-426, default arguments) of ``probs``
    [N, C] against ``labels`` [N], as a dict of floats, with one host synchronisation at the end.  ``ece`` and
    ``rmsce`` share one ordering of the max-probs.

    ``probs`` of shape [N, 1] is the binary problem: the column p becomes ``[[1 - p, p]]`` in fp64 before anything else,
    as the reference's ``update_state`` does, and ``labels`` are 0 / 1.  (``ensemble_probs`` keeps C = 1 as it is: the
    softmax of one class is 1.)

    A NaN anywhere in the probabilities gives NaN for every metric.  (The reference's numpy code would drop such rows
    through its ``> 0`` filter and report a number over the rest; a NaN ensemble is reported as such here.)"""
    metrics = tuple(metrics)
    if set(metrics) - {"ece", "ace", "rmsce"}:
        raise ValueError(f"unknown metrics {sorted(set(metrics) - {'ece', 'ace', 'rmsce'})}")
    num_bins = _check_bins(num_bins)
    probs = _probs(probs)
    labels = _labels(labels, probs)
    if probs.shape[1] == 1:                         # calibration_error.py:204-210: one column p is [[1 - p, p]]
        probs = torch.cat([1.0 - probs, probs], 1)
    N, C = probs.shape
    dev = probs.device
    rms_bins = num_bins if datapoints_per_bin is None else _check_bins(int(N / datapoints_per_bin))
    out = torch.empty(len(metrics), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        if {"ece", "rmsce"} & set(metrics):
            conf = torch.empty(N, dtype=torch.float64, device=dev)
            pred = torch.empty(N, dtype=torch.int64, device=dev)
            hit = torch.empty(N, dtype=torch.int64, device=dev)
            _hip.check(_hip.lib().sgmcmc_row_max(probs.data_ptr(), labels.data_ptr(), N, C, conf.data_ptr(),
                                                 pred.data_ptr(), hit.data_ptr(), _stream()), "sgmcmc_row_max")
            perm = _order(conf, N, 1, 1, 0)
        for i, name in enumerate(metrics):
            if name == "ece":                       # even bins, max-prob, l1
                if num_bins == 0:
                    raise ValueError("ece needs num_bins >= 1")
                _calib(conf, perm, hit, False, N, 1, 1, 0, _even_bounds(num_bins, dev), num_bins, False, out[i:])
            elif name == "rmsce":                   # adaptive, int(N / datapoints_per_bin) bins, max-prob, l2
                _calib(conf, perm, hit, False, N, 1, 1, 0, None, rms_bins, True, out[i:])
            else:                                   # adaptive, class-conditional over every column, l1
                pc = _order(probs, N, C, C, 1)
                _calib(probs, pc, labels, True, N, C, C, 1, None, num_bins, False, out[i:])
        vals = out.cpu().tolist()
    return dict(zip(metrics, vals))


def ece(labels, probs, num_bins=30):
    "Expected calibration error (calibration_error.py:379): even bins over the max-prob, l1"
    return calibration_metrics(labels, probs, ("ece",), num_bins=num_bins)["ece"]


def ace(labels, probs, num_bins=30):
    "Adaptive calibration error (calibration_error.py:417): adaptive bins per class column, l1, mean over classes"
    return calibration_metrics(labels, probs, ("ace",), num_bins=num_bins)["ace"]


def rmsce(labels, probs, num_bins=30, datapoints_per_bin=100):
    """Root-mean-squared calibration error (calibration_error.py:390): adaptive bins over the max-prob, l2; with
    ``datapoints_per_bin`` the bin count is int(N / datapoints_per_bin) (one bin below that many rows)"""
    return calibration_metrics(labels, probs, ("rmsce",), num_bins=num_bins,
                               datapoints_per_bin=datapoints_per_bin)["rmsce"]


def auroc_auprc(scores_in, scores_out):
    """(AUROC, average precision) of the scores with the in-distribution set as the positive class -- sklearn's
    ``roc_auc_score`` / ``average_precision_score`` as exp_utils.py:368-373 calls them.  The ROC area is accumulated in
    integers, so AUROC is the exact rational 2 area / (2 P Nn) correctly rounded.  Raises ``ValueError`` if either set
    is empty or a score is NaN (as sklearn does)."""
    if not all(isinstance(s, torch.Tensor) and s.dim() == 1 for s in (scores_in, scores_out)):
        raise ValueError("scores must be 1-d tensors")
    P, Nn = scores_in.shape[0], scores_out.shape[0]
    if P == 0 or Nn == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    n = P + Nn
    if n > MAX_ROWS:
        raise ValueError(f"{n} scores: at most {MAX_ROWS} are supported")
    _cuda(scores_in, "scores_in")
    _cuda(scores_out, "scores_out")
    if scores_in.device != scores_out.device:
        raise ValueError("scores_in and scores_out are on different devices")
    dev = scores_in.device
    scores = torch.cat([scores_in.to(torch.float64), scores_out.to(torch.float64)]).contiguous()
    out = torch.empty(3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        perm = _order(scores, n, 1, 1, 0)
        _hip.check(_hip.lib().sgmcmc_rank_metrics(scores.data_ptr(), perm.data_ptr(), n, P, out.data_ptr(),
                                                  _stream()), "sgmcmc_rank_metrics")
        auroc, auprc, has_nan = out.cpu().tolist()
    if has_nan:
        raise ValueError("Input contains NaN.")
    return auroc, auprc
