"""Does the prior matter for this posterior, and for which quantities?  Power-scaling sensitivity from the draws already
stored, on the device (``csrc/powerscale_hip.inc``; C ABI ``sgmcmc_powerscale_sort`` / ``sgmcmc_powerscale_distance``;
Kallioinen, Paananen, Buerkner & Vehtari 2023, the R package priorsense).  The prior, or the likelihood, is raised to a
power alpha near 1 by importance-reweighting the draws (``power_scale_weights``: the log ratios ``(alpha - 1) log p``
smoothed by ``model_comparison.psis``); ``weighted_distance`` measures how far every quantity's weighted distribution
moves -- the normalised cumulative Jensen-Shannon distance between the unweighted and the weighted ECDF -- together
with the weighted mean and sd; ``power_scale_sensitivity`` turns two such distances, at ``1 / alpha`` and ``alpha``,
into the sensitivity psi and reads the pair (prior, likelihood) as the usual table:

    prior psi >= threshold, likelihood psi >= threshold    prior-data conflict
    prior psi >= threshold, likelihood psi below it        strong prior or weak likelihood
    prior psi below it                                     no prior sensitivity

``include/sgmcmc_hip.h`` states the definition and ``tests/powerscale_reference.py`` restates it in numpy.  The
reference has nothing of the kind.  Everything runs in fp64 in a fixed order: two calls give the same bits, a
quantity's result does not depend on which other quantities are in the call, and the chunking changes no bit.  Nothing
here synchronises with the host.  There is no moment matching: a Pareto-k above ``model_comparison.k_threshold(N)``
means that the draws cannot answer the question for that power -- rerun the chain under the scaled prior.
"""
import collections
import math

import torch

from . import _hip, model_comparison

__all__ = ("power_scale_weights", "weighted_distance", "power_scale_sensitivity", "power_scale_sequence", "sort_tile",
           "PowerScaleWeights", "WeightedDistance", "WeightedDistanceParts", "ComponentSensitivity",
           "PowerScaleSensitivity", "PowerScaleSequence", "NONE", "CONFLICT", "STRONG_PRIOR")

MIN_DRAWS, MAX_DRAWS = _hip.PSIS_MIN_DRAWS, _hip.POWERSCALE_MAX_DRAWS
TILE_CELLS = _hip.POWERSCALE_TILE_CELLS
MAX_TILE = 64                        # quantities per workgroup of the keyed sort, at most
MAX_VECTORS = 65535                  # weight vectors of one call
CHUNK = 64                           # the quantities are walked in multiples of the widest sort tile
DRAW_BYTES = 10                      # workspace per draw and quantity: the sorted value (fp64) and its draw index (uint16)
NONE, CONFLICT, STRONG_PRIOR = 0, 1, 2          # the diagnosis codes

PowerScaleWeights = collections.namedtuple("PowerScaleWeights", "log_weights pareto_k ess")
WeightedDistance = collections.namedtuple("WeightedDistance", "dist mean sd")
WeightedDistanceParts = collections.namedtuple("WeightedDistanceParts",
                                               WeightedDistance._fields + ("sorted", "order", "weights"))
ComponentSensitivity = collections.namedtuple("ComponentSensitivity", "psi mean_gradient sd_gradient pareto_k ess")
PowerScaleSensitivity = collections.namedtuple("PowerScaleSensitivity", "components diagnosis alpha threshold")
PowerScaleSequence = collections.namedtuple("PowerScaleSequence", "alphas dist mean sd pareto_k ess")


def sort_tile(N):
    """TQ, the quantities that one workgroup of the keyed sort stages at N draws (``sgmcmc_powerscale_tile_quantities``
    restated): min(64, 8192 / N_pad), N_pad the next power of two"""
    if not MIN_DRAWS <= N <= MAX_DRAWS:
        raise ValueError(f"N = {N} is outside [{MIN_DRAWS}, {MAX_DRAWS}]")
    return min(TILE_CELLS // max(8, 1 << (N - 1).bit_length()), MAX_TILE)


def _check_draws(N, what):
    if not MIN_DRAWS <= N <= MAX_DRAWS:
        raise ValueError(f"{what}: {N} draws; between {MIN_DRAWS} and {MAX_DRAWS} are supported")


def _need_cuda(t, what):
    if not t.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor (there is no CPU path)")


def _check_component(lc, what="log_component", device=True):
    """-> N of a valid log density per draw ([N] or [M, S], CUDA, fp64); ValueError otherwise (``device=False``: the caller
    has more to check before the last test, that it is on the device)"""
    if not isinstance(lc, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if lc.dtype != torch.float64:
        raise ValueError(f"{what} must be float64, not {lc.dtype}")
    if lc.dim() not in (1, 2):
        raise ValueError(f"{what} must be [draws] or [chains, draws]")
    _check_draws(lc.numel(), what)
    if device:
        _need_cuda(lc, what)
    return lc.numel()


def _check_alphas(alphas, what="alphas", not_one=False):
    try:
        alphas = tuple(float(a) for a in alphas)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a sequence of positive powers") from None
    if not alphas or not all(a > 0.0 and math.isfinite(a) for a in alphas):
        raise ValueError(f"{what} must be a non-empty sequence of positive finite powers, not {alphas!r}")
    if len(alphas) > MAX_VECTORS:
        raise ValueError(f"{what}: at most {MAX_VECTORS} powers are supported")
    if not_one and any(a == 1.0 for a in alphas):
        raise ValueError(f"{what} must differ from 1")
    return alphas


def _check_x(x, workspace_bytes, device=True):
    "-> (M, S, N, shape, Q, quantities per chunk) of valid draws x [M, S, *shape]; ValueError otherwise"
    if not isinstance(x, torch.Tensor):
        raise ValueError("x must be a tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"x must be float32 or float64, not {x.dtype}")
    if x.dim() < 2:
        raise ValueError("x must be [chains, draws, ...]")
    M, S = x.shape[:2]
    N = M * S
    _check_draws(N, "x")
    try:
        workspace_bytes = int(workspace_bytes)
    except (TypeError, ValueError):
        raise ValueError("workspace_bytes must be an integer") from None
    chunk = workspace_bytes // (DRAW_BYTES * N) // CHUNK * CHUNK
    if chunk < CHUNK:
        raise ValueError(f"workspace_bytes = {workspace_bytes} is too small: {CHUNK} quantities of {N} draws need "
                         f"{CHUNK * DRAW_BYTES * N} bytes")
    if device:
        _need_cuda(x, "x")
    shape = tuple(x.shape[2:])
    return M, S, N, shape, math.prod(shape), chunk


def _check_log_weights(lw, N, dev, what="log_weights"):
    if not isinstance(lw, torch.Tensor) or lw.dtype != torch.float64 or lw.dim() != 2 or lw.shape[0] != N:
        raise ValueError(f"{what} must be a float64 tensor of shape [{N}, A]")
    if not 1 <= lw.shape[1] <= MAX_VECTORS:
        raise ValueError(f"{what}: between 1 and {MAX_VECTORS} weight vectors are supported, not {lw.shape[1]}")
    if lw.device != dev:
        raise ValueError(f"{what} must be on x's device")


def _ratios(log_component, alphas):
    "[N, A]: (alpha - 1) log p, the power's offset formed on the host in fp64"
    scale = torch.tensor([a - 1.0 for a in alphas], dtype=torch.float64, device=log_component.device)
    return log_component.reshape(-1, 1) * scale


def _weights(ratios):
    lw, k = model_comparison.psis(ratios, r_eff=None)
    w = torch.exp(lw)
    return PowerScaleWeights(lw, k, 1.0 / (w * w).sum(dim=0))


def power_scale_weights(log_component, alphas):
    """log_component [N] or [M, S] (CUDA, fp64): a component's log density at every draw, the draws in the order
    t = m S + s; alphas: positive powers -> ``PowerScaleWeights(log_weights [N, A], pareto_k [A], ess [A])``.  Column a
    holds the Pareto-smoothed, normalised log importance weights that turn the draws into draws of the posterior with
    that component raised to ``alphas[a]``: ``model_comparison.psis`` of the log ratios ``(alphas[a] - 1) log_component``
    with ``r_eff=None``; ``ess = 1 / sum_t w_t^2``.  ``alpha = 1`` gives uniform weights and ``pareto_k = +inf`` (an empty
    tail); a non-finite log density gives NaN."""
    _check_component(log_component, device=False)
    alphas = _check_alphas(alphas)
    _need_cuda(log_component, "log_component")
    return _weights(_ratios(log_component, alphas))


def _distance(x, w, workspace_bytes, parts):
    "x [M, S, *shape] and linear weights w [N, A] (contiguous) -> (res [3, A, Q], sorted, order); the checks are done"
    M, S, N, shape, Q, chunk = _check_x(x, workspace_bytes)
    dev, A = x.device, w.shape[1]
    res = torch.empty((3, A, Q), dtype=torch.float64, device=dev)
    ordered = torch.empty((N, Q), dtype=torch.float64, device=dev) if parts else None
    order = torch.empty((N, Q), dtype=torch.int16, device=dev) if parts else None
    if Q:
        if not x[0, 0].is_contiguous():          # the trailing dims are one contiguous run of Q elements, or are made so
            x = x.contiguous()
        chunk = min(chunk, (Q + CHUNK - 1) // CHUNK * CHUNK)
        work = torch.empty(chunk * DRAW_BYTES * N // 8, dtype=torch.float64, device=dev)
        item, is_f64 = x.element_size(), int(x.dtype == torch.float64)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            L = _hip.lib()
            for q0 in range(0, Q, chunk):
                Qc = min(chunk, Q - q0)
                values = work.data_ptr()                                      # [N][Qc] fp64: the sorted columns
                index = values + 8 * N * Qc                                   # [N][Qc] uint16: their draw indices
                _hip.check(L.sgmcmc_powerscale_sort(x.data_ptr() + q0 * item, is_f64, x.stride(0), x.stride(1), M, S, Qc,
                                                    values, index, stream), "sgmcmc_powerscale_sort")
                dist, mean, sd = (res[r].data_ptr() + 8 * q0 for r in range(3))
                _hip.check(L.sgmcmc_powerscale_distance(values, index, N, Qc, w.data_ptr(), A, Q, dist, mean, sd, stream),
                           "sgmcmc_powerscale_distance")
                if parts:
                    ordered[:, q0:q0 + Qc] = work[:N * Qc].view(N, Qc)
                    order[:, q0:q0 + Qc] = work[N * Qc:].view(torch.int16)[:N * Qc].view(N, Qc)
    return res, ordered, order


def weighted_distance(x, log_weights, workspace_bytes=256 << 20, parts=False):
    """x [M, S, *shape] (CUDA, fp32 or fp64; M chains of S draws, N = M S of them in the order t = m S + s, read in
    place) and log_weights [N, A] (fp64, on the same device; ``power_scale_weights``' or any other log importance
    weights) -> ``WeightedDistance(dist, mean, sd)``, each [A, *shape] fp64: for every weight vector and quantity the
    normalised cumulative Jensen-Shannon distance in [0, 1] between the ECDF of the draws and their weighted ECDF, and
    the weighted mean and sd, as ``include/sgmcmc_hip.h`` defines them.  The kernels take the linear weights
    ``exp(log_weights)``, which need not be normalised.

    Every column is sorted by an LDS sorting network that carries each draw's index, so at most 8192 draws enter.  The
    quantities are walked in chunks (multiples of 64) whose sorted columns fit ``workspace_bytes``: one workspace per
    call, 10 bytes per draw and quantity; the chunking changes no bit.  A quantity with a non-finite draw gives NaN, as
    does a weight vector with a non-finite entry; a constant quantity gives ``dist`` = 0, its value and ``sd`` = 0.
    ``parts=True``: a ``WeightedDistanceParts`` that also carries ``sorted`` [N, Q] (fp64), ``order`` [N, Q] (int16: the
    draw index at every rank) and ``weights`` [N, A], the linear weights that the kernel read.  Everything stays on the
    current stream."""
    _, _, N, shape, _, _ = _check_x(x, workspace_bytes, device=False)
    _check_log_weights(log_weights, N, x.device)
    _need_cuda(x, "x")
    w = torch.exp(log_weights).contiguous()
    res, ordered, order = _distance(x, w, workspace_bytes, parts)
    out = [t.reshape((w.shape[1],) + shape) for t in res]
    return WeightedDistanceParts(*out, ordered, order, w) if parts else WeightedDistance(*out)


def _components(components, N, dev):
    if not isinstance(components, dict) or not components:
        raise ValueError("components must be a non-empty dict {name: log density per draw}")
    for name, lc in components.items():
        if _check_component(lc, f"components[{name!r}]", device=False) != N:
            raise ValueError(f"components[{name!r}] holds {lc.numel()} draws, x {N}")
        if lc.device != dev:
            raise ValueError(f"components[{name!r}] must be on x's device")


def power_scale_sensitivity(x, components, alpha=1.01, threshold=0.05, workspace_bytes=256 << 20):
    """x [M, S, *shape] (CUDA, fp32 or fp64) and components {name: log density per draw, [N] or [M, S], CUDA, fp64} --
    typically ``{"prior": ..., "likelihood": ...}``; any further key is selective power-scaling, one key per prior module
    for instance -> ``PowerScaleSensitivity(components, diagnosis, alpha, threshold)``.

    Every component is scaled to the powers ``1 / alpha`` and ``alpha`` (``power_scale_weights``), all of them in one
    ``weighted_distance`` call, so the columns are sorted once.  ``components[name]`` is a ``ComponentSensitivity``:
    ``psi [*shape] = (dist_lo + dist_hi) / (2 log2 alpha)``, ``mean_gradient = (mean_hi - mean_lo) / (2 log2 alpha)``,
    ``sd_gradient`` likewise, and ``pareto_k``, ``ess`` [2]: of the lower and the upper power.  When both ``"prior"`` and
    ``"likelihood"`` are among the components, ``diagnosis [*shape]`` (int8) reads them as the table: ``CONFLICT`` = 1
    where both psi >= threshold (prior-data conflict), ``STRONG_PRIOR`` = 2 where the prior's is and the likelihood's is
    not (strong prior or weak likelihood), ``NONE`` = 0 elsewhere -- also where a psi is NaN; else it is None.  There is
    no moment matching: where ``pareto_k`` exceeds ``model_comparison.k_threshold(N)`` the draws cannot answer the
    question.  Nothing synchronises."""
    _, _, N, shape, _, _ = _check_x(x, workspace_bytes, device=False)
    (alpha,) = _check_alphas((alpha,), "alpha", not_one=True)
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("threshold must be a number") from None
    if not threshold > 0.0:
        raise ValueError(f"threshold = {threshold!r} must be positive")
    _components(components, N, x.device)
    _need_cuda(x, "x")
    names = list(components)
    powers = (1.0 / alpha, alpha)
    ratios = torch.cat([_ratios(components[n], powers) for n in names], dim=1)            # [N, 2 K]: (lo, hi) per component
    if ratios.shape[1] > MAX_VECTORS:
        raise ValueError(f"at most {MAX_VECTORS // 2} components are supported")
    weights = _weights(ratios)
    d = weighted_distance(x, weights.log_weights, workspace_bytes)
    # a 0-d tensor: torch divides by a Python number as a product with its reciprocal, by a tensor with one rounding
    scale = torch.full((), 2.0 * math.log2(alpha), dtype=torch.float64, device=x.device)
    out = {}
    for i, n in enumerate(names):
        lo, hi = 2 * i, 2 * i + 1
        out[n] = ComponentSensitivity((d.dist[lo] + d.dist[hi]) / scale, (d.mean[hi] - d.mean[lo]) / scale,
                                      (d.sd[hi] - d.sd[lo]) / scale, weights.pareto_k[lo:hi + 1], weights.ess[lo:hi + 1])
    diagnosis = None
    if "prior" in out and "likelihood" in out:
        p, l = out["prior"].psi >= threshold, out["likelihood"].psi >= threshold
        diagnosis = (p & l).to(torch.int8) * CONFLICT + (p & ~l).to(torch.int8) * STRONG_PRIOR
    return PowerScaleSensitivity(out, diagnosis, alpha, threshold)


def power_scale_sequence(x, log_component, alphas, workspace_bytes=256 << 20):
    """The three tables over a grid of powers, for the plot of priorsense's ``powerscale_sequence``: x [M, S, *shape],
    log_component [N] or [M, S], alphas [A] -> ``PowerScaleSequence(alphas, dist, mean, sd, pareto_k, ess)``, the tables
    [A, *shape] and ``pareto_k``, ``ess`` [A]."""
    _, _, N, _, _, _ = _check_x(x, workspace_bytes, device=False)
    alphas = _check_alphas(alphas)
    _components({"log_component": log_component}, N, x.device)
    _need_cuda(x, "x")
    weights = _weights(_ratios(log_component, alphas))
    d = weighted_distance(x, weights.log_weights, workspace_bytes)
    return PowerScaleSequence(alphas, d.dist, d.mean, d.sd, weights.pareto_k, weights.ess)
