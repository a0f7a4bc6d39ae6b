"""Uncertainty of a posterior ensemble on the device (``csrc/uncert_hip.inc``; C ABI ``sgmcmc_uncertainty_rows`` /
``sgmcmc_risk_coverage``, definitions in ``include/sgmcmc_hip.h``) -- what the reference does not compute:

    decompose       per row of the per-sample table ``acc [E, N, C]``: the ensemble's probabilities, max-prob, margin,
                    predictive entropy H[pbar], expected (aleatoric) entropy mean_e H[p_e], their difference the mutual
                    information between prediction and weights (epistemic, BALD), the samples' disagreement with the
                    ensemble's prediction and, with labels, the ensemble's NLL and Brier score
    risk_coverage   the risk-coverage curve of selective prediction, its area (AURC) and the excess over the oracle
                    ordering (E-AURC; Geifman et al. 2019), ties averaged over their random order
    ood_scores      the three scores of a decomposition as "higher = more in-distribution", for ``auroc_auprc``

Everything runs in fp64 in an order fixed by the sizes (counts in integers), so two calls give the same bits;
``decompose`` does not synchronise with the host, ``risk_coverage`` does once, when it reads its result.
"""
import collections

import torch

from . import _hip
from .calibration import MAX_CLASSES, MAX_ROWS, _cuda, _order, _stream

__all__ = ("Uncertainty", "RiskCoverage", "decompose", "risk_coverage", "ood_scores")

Uncertainty = collections.namedtuple("Uncertainty", "probs pred max_prob margin entropy expected_entropy mutual_info "
                                                    "disagreement nll brier hit")
Uncertainty.__doc__ = ("probs [N, C] fp64 and, per row [N]: pred = first argmax (int64), max_prob, margin = max-prob minus "
                       "the second largest, entropy of probs, expected_entropy = mean over the samples of their own "
                       "entropy, mutual_info = max(entropy - expected_entropy, 0), disagreement = the share of samples "
                       "whose argmax is not pred (fp64; nats); with labels nll = -log probs[y], brier and hit = "
                       "pred == labels (int64), else None")

RiskCoverage = collections.namedtuple("RiskCoverage", "aurc eaurc risk order")
RiskCoverage.__doc__ = ("aurc, eaurc: floats; risk [N] fp64: the selective risk at coverage (k + 1) / N; order [N] int64: "
                        "the rows from the most confident down (equal scores: the later row first)")


def decompose(acc, labels=None):
    """acc [E, N, C]: per-sample NORMALISED log-probabilities (``evaluation.predictive_tables`` / ``logit_tables``; not
    renormalised here) -> ``Uncertainty``.  ``probs`` / ``max_prob`` / ``pred`` / ``hit`` are bit for bit those of
    ``calibration.ensemble_probs``.  A NaN in a row makes that row's floating-point fields NaN.  One pass over the
    table, no host synchronisation."""
    if not isinstance(acc, torch.Tensor) or acc.dim() != 3:
        raise ValueError("acc must be an [E, N, C] tensor")
    E, N, C = acc.shape
    if not 0 < C <= MAX_CLASSES:
        raise ValueError(f"{C} classes: 1 .. {MAX_CLASSES} are supported")
    if E == 0 or N == 0 or E >= 2 ** 31 or N >= 2 ** 31:
        raise ValueError("acc needs at least one sample and one row (fewer than 2^31 of each)")
    if labels is not None and (not isinstance(labels, torch.Tensor) or labels.shape != (N,)
                               or labels.dtype.is_floating_point or labels.dtype == torch.bool):
        raise ValueError("labels must be an integer [N] tensor")
    _cuda(acc, "acc")
    if labels is not None:
        _cuda(labels, "labels")
        if labels.device != acc.device:
            raise ValueError("labels and acc are on different devices")
        labels = labels.to(torch.int64).contiguous()
    acc = acc.to(torch.float64).contiguous()
    dev = acc.device
    probs = torch.empty((N, C), dtype=torch.float64, device=dev)
    f = torch.empty((8, N), dtype=torch.float64, device=dev)   # max_prob margin entropy expected mutual disagreement nll brier
    pred = torch.empty(N, dtype=torch.int64, device=dev)
    hit = None if labels is None else torch.empty(N, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        err = _hip.lib().sgmcmc_uncertainty_rows(
            acc.data_ptr(), 0 if labels is None else labels.data_ptr(), E, N, C, probs.data_ptr(), f[0].data_ptr(),
            pred.data_ptr(), 0 if hit is None else hit.data_ptr(), f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(),
            f[4].data_ptr(), f[5].data_ptr(), 0 if labels is None else f[6].data_ptr(),
            0 if labels is None else f[7].data_ptr(), _stream())
    _hip.check(err, "sgmcmc_uncertainty_rows")
    return Uncertainty(probs, pred, f[0], f[1], f[2], f[3], f[4], f[5], None if labels is None else f[6],
                       None if labels is None else f[7], hit)


def risk_coverage(scores, losses):
    """scores [N] (higher = more confident) and losses [N] (``1 - hit``, ``nll``, ...) -> ``RiskCoverage``: ``risk[k]``
    is the mean loss of the k + 1 most confident rows, rows of equal score entering with their group's mean loss (the
    expectation over a random order among them, so the curve does not depend on the order of the rows); ``aurc`` is the
    mean of ``risk``; ``eaurc = aurc - aurc*`` with ``aurc*`` the same of the oracle ordering ``scores = -losses``.
    Integer-valued losses give the correctly rounded rationals.  Raises ``ValueError`` if a score or a loss is NaN.
    One host synchronisation."""
    if not all(isinstance(s, torch.Tensor) and s.dim() == 1 for s in (scores, losses)):
        raise ValueError("scores and losses must be 1-d tensors")
    n = scores.shape[0]
    if losses.shape[0] != n:
        raise ValueError(f"{n} scores but {losses.shape[0]} losses")
    if not 0 < n <= MAX_ROWS:
        raise ValueError(f"{n} rows: 1 .. {MAX_ROWS} are supported")
    _cuda(scores, "scores")
    _cuda(losses, "losses")
    if scores.device != losses.device:
        raise ValueError("scores and losses are on different devices")
    dev = scores.device
    scores = scores.to(torch.float64).contiguous()
    losses = losses.to(torch.float64).contiguous()
    risk = torch.empty((2, n), dtype=torch.float64, device=dev)
    out = torch.empty((2, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        oracle = -losses
        perm = _order(scores, n, 1, 1, 0)
        perm_oracle = _order(oracle, n, 1, 1, 0)
        for i, (s, p) in enumerate(((scores, perm), (oracle, perm_oracle))):
            _hip.check(_hip.lib().sgmcmc_risk_coverage(s.data_ptr(), losses.data_ptr(), p.data_ptr(), n,
                                                       risk[i].data_ptr(), out[i].data_ptr(), _stream()),
                       "sgmcmc_risk_coverage")
        (aurc, _, has_nan), (best, _, _) = out.cpu().tolist()
    if has_nan:
        raise ValueError("Input contains NaN.")
    return RiskCoverage(aurc, aurc - best, risk[0], perm[0].flip(0).to(torch.int64))


def ood_scores(u):
    """The out-of-distribution scores of an ``Uncertainty``, each with higher = more in-distribution, ready for
    ``calibration.auroc_auprc(scores_in, scores_out)``: the max-prob, the negated predictive entropy and the negated
    mutual information."""
    if not isinstance(u, Uncertainty):
        raise ValueError("ood_scores takes the Uncertainty that decompose returns")
    return {"max_prob": u.max_prob, "entropy": -u.entropy, "mutual_info": -u.mutual_info}
