"""Predictive scores of a regression posterior on the device (``csrc/regress_hip.inc``; C ABI ``sgmcmc_gmix_rows`` /
``sgmcmc_gmix_quantiles`` / ``sgmcmc_pit_calibration``, definitions in ``include/sgmcmc_hip.h``) -- what the reference
does not compute.  Per row and output the posterior predictive of a ``RegressionModel`` is the equal-weight mixture of
the samples' ``Normal(mean_e, scale_e)``, with the CDF ``F(x) = mean_e Phi((x - mean_e) / scale_e)``:

    predictive       its mean, its variance split into aleatoric (mean_e scale_e^2) and epistemic (the samples'
                     disagreement about the mean) and, with targets, the squared error, the log density, the PIT
                     ``F(y)`` and the CRPS by the mixture's closed form (Grimit et al. 2006): a sum over all pairs of
                     samples, tiled through LDS and split over workgroups, with no [N, E, E] table
    quantiles        ``q`` with ``F(q) = p``: bracketed by the components' own quantiles, refined to adjacent doubles
    pit_calibration  of PIT values: the Kolmogorov-Smirnov distance to the uniform, the calibration error of Kuleshov et
                     al. 2018 and the coverage of central intervals, counts in integers
    interval_score   the Winkler score of a central interval (Gneiting & Raftery 2007)

Everything runs in fp64 in an order fixed by the sizes (counts in integers), so two calls give the same bits;
``predictive`` and ``quantiles`` do not synchronise with the host, ``pit_calibration`` does once, when it reads its result.
"""
import collections

import torch

from . import _hip
from .calibration import MAX_ROWS, _cuda, _order, _stream

__all__ = ("GaussianMixture", "PitCalibration", "predictive", "quantiles", "pit_calibration", "interval_score",
           "normal_quantile", "pair_split")

TILE = _hip.GMIX_TILE                    # samples of one LDS tile of the pair sum
MAX_SAMPLES = _hip.GMIX_MAX_SAMPLES
MAX_QUANTILES = _hip.GMIX_MAX_QUANTILES
MAX_LEVELS = _hip.PIT_MAX_LEVELS
MAX_ENTRIES = 2 ** 30                    # rows x outputs
TARGET_GROUPS = 2048                     # workgroups the pair sum aims at
DEFAULT_LEVELS = tuple(k / 20 for k in range(1, 20))

GaussianMixture = collections.namedtuple("GaussianMixture", "mean var_aleatoric var_epistemic var sq_err lpd pit crps")
GaussianMixture.__doc__ = ("each [N, D] fp64: mean of the mixture; var_aleatoric = mean_e scale_e^2; var_epistemic = "
                           "mean_e (mean_e - mean)^2; var = their sum; with y sq_err = (y - mean)^2, lpd = the log "
                           "density of y, pit = F(y), crps (else None)")

PitCalibration = collections.namedtuple("PitCalibration", "ks calibration_error freq coverage")
PitCalibration.__doc__ = ("ks, calibration_error: floats; freq [J] = #{u <= levels[j]} / N and coverage [len(central)] = "
                          "#{(1 - c) / 2 <= u <= (1 + c) / 2} / N: fp64 tensors on the host, each the correctly rounded "
                          "quotient of an integer count by N")


def pair_split(E, N, D):
    """The workgroups one entry's triangle of tile pairs is cut into (``gmix_split`` of the kernels: a function of the
    sizes alone): enough for ``TARGET_GROUPS`` over the N D entries, at most half the tile pairs."""
    tiles = -(-E // TILE)
    pairs = tiles * (tiles + 1) // 2
    return min(-(-TARGET_GROUPS // (N * D)), (pairs + 1) // 2)


def _tables(mean, scale):
    "the checked fp64 tables: mean [E, N, D] contiguous, scale as a view expanded to [E, N, D] (strides may be 0)"
    if not isinstance(mean, torch.Tensor) or mean.dim() != 3:
        raise ValueError("mean must be an [E, N, D] tensor")
    E, N, D = mean.shape
    if E == 0 or N == 0 or D == 0:
        raise ValueError("mean needs at least one sample, one row and one output")
    if E > MAX_SAMPLES:
        raise ValueError(f"{E} samples: at most {MAX_SAMPLES} are supported")
    if N >= 2 ** 31 or N * D > MAX_ENTRIES:
        raise ValueError(f"{N} x {D} entries: at most {MAX_ENTRIES} are supported")
    if not isinstance(scale, torch.Tensor) or scale.dim() > 3:
        raise ValueError("scale must be a tensor of shape [E], [E, D] or one that broadcasts to mean's [E, N, D]")
    shape = tuple(scale.shape)
    if scale.dim() == 1:                            # one noise level per sample
        shape = shape + (1, 1)
    elif scale.dim() == 2:                          # ... per sample and output
        shape = (shape[0], 1, shape[1])
    elif scale.dim() == 0:
        shape = (1, 1, 1)
    if any(s not in (1, m) for s, m in zip(shape, (E, N, D))):
        raise ValueError(f"scale of shape {tuple(scale.shape)} does not broadcast to mean's {(E, N, D)}")
    _cuda(mean, "mean")
    _cuda(scale, "scale")
    if scale.device != mean.device:
        raise ValueError("scale and mean are on different devices")
    mean = mean.to(torch.float64).contiguous()
    scale = scale.to(torch.float64).reshape(shape).expand(E, N, D)
    return mean, scale, (E, N, D)


def predictive(mean, scale, y=None):
    """mean [E, N, D], scale ([E], [E, D], or broadcastable to [E, N, D]; read through its strides, never expanded in
    memory) and optionally y [N, D] -> ``GaussianMixture``.  A NaN among an entry's inputs, or a scale that is not > 0,
    makes that entry's fields NaN.  Two launches with y, one without; no host synchronisation."""
    mean, scale, (E, N, D) = _tables(mean, scale)
    dev = mean.device
    if y is not None:
        if not isinstance(y, torch.Tensor) or tuple(y.shape) != (N, D):
            raise ValueError(f"y must be an [N, D] = {(N, D)} tensor")
        _cuda(y, "y")
        if y.device != dev:
            raise ValueError("y and mean are on different devices")
        y = y.to(torch.float64).contiguous()
    out = torch.empty((8 if y is not None else 4, N, D), dtype=torch.float64, device=dev)
    ptr = [out[i].data_ptr() for i in range(out.shape[0])] + [0] * (8 - out.shape[0])
    with torch.cuda.device(dev):
        lib = _hip.lib()
        work, nbytes = None, 0
        if y is not None:
            nbytes = lib.sgmcmc_gmix_workspace_bytes(E, N, D)
            work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        err = lib.sgmcmc_gmix_rows(mean.data_ptr(), scale.data_ptr(), *scale.stride(), 0 if y is None else y.data_ptr(),
                                   E, N, D, 0 if work is None else work.data_ptr(), nbytes, *ptr, _stream())
    _hip.check(err, "sgmcmc_gmix_rows")
    return GaussianMixture(*out, *([None] * (8 - out.shape[0])))


def normal_quantile(probs):
    "z = Phi^-1(p) in fp64 on the host, a [Q] tensor: what ``quantiles`` hands the kernel to bracket with"
    return torch.special.ndtri(torch.as_tensor(probs, dtype=torch.float64).reshape(-1).cpu())


def quantiles(mean, scale, probs):
    """[Q, N, D] fp64: per level p of ``probs`` (floats in (0, 1), at most ``MAX_QUANTILES``) the q with F(q) = p, to
    adjacent doubles; E = 1 gives ``mean + scale * normal_quantile(p)``.  One launch, no host synchronisation."""
    try:
        levels = [float(p) for p in (probs.tolist() if isinstance(probs, torch.Tensor) else probs)]
    except TypeError:
        raise ValueError("probs must be a sequence of levels") from None
    if not 0 < len(levels) <= MAX_QUANTILES:
        raise ValueError(f"{len(levels)} levels: 1 .. {MAX_QUANTILES} are supported")
    if not all(0.0 < p < 1.0 for p in levels):
        raise ValueError("every level must lie strictly between 0 and 1")
    mean, scale, (E, N, D) = _tables(mean, scale)
    dev = mean.device
    p = torch.tensor(levels, dtype=torch.float64)
    pz = torch.stack([p, normal_quantile(p)]).to(dev)
    out = torch.empty((len(levels), N, D), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        err = _hip.lib().sgmcmc_gmix_quantiles(mean.data_ptr(), scale.data_ptr(), *scale.stride(), E, N, D,
                                               pz[0].data_ptr(), pz[1].data_ptr(), len(levels), out.data_ptr(), _stream())
    _hip.check(err, "sgmcmc_gmix_quantiles")
    return out


def _levels(values, what, least):
    try:
        values = [float(v) for v in (values.tolist() if isinstance(values, torch.Tensor) else values)]
    except TypeError:
        raise ValueError(f"{what} must be a sequence of numbers") from None
    if not least <= len(values) <= MAX_LEVELS:
        raise ValueError(f"{len(values)} {what}: {least} .. {MAX_LEVELS} are supported")
    if not all(0.0 < v < 1.0 for v in values):
        raise ValueError(f"every one of {what} must lie strictly between 0 and 1")
    return values


def _pit_columns(pit, levels, central):
    "pit [N, D] on the device -> the kernel's [D, 3 + J + len(central)] table on the host (one synchronisation)"
    N, D = pit.shape
    dev = pit.device
    pit = pit.to(torch.float64).contiguous()
    J, Cn = len(levels), len(central)
    args = torch.tensor(levels + central, dtype=torch.float64).to(dev)
    out = torch.empty((D, 3 + J + Cn), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        perm = _order(pit, N, D, D, 1)
        _hip.check(_hip.lib().sgmcmc_pit_calibration(pit.data_ptr(), D, 1, perm.data_ptr(), N, D, args.data_ptr(), J,
                                                     args[J:].data_ptr() if Cn else 0, Cn, out.data_ptr(), _stream()),
                   "sgmcmc_pit_calibration")
        table = out.cpu()
    if table[:, 2].any():
        raise ValueError("Input contains NaN.")
    return table


def _check_pit(pit, dims):
    if not isinstance(pit, torch.Tensor) or pit.dim() != dims:
        raise ValueError("pit must be an [N] tensor" if dims == 1 else "pit must be an [N, D] tensor")
    if not 0 < pit.shape[0] <= MAX_ROWS:
        raise ValueError(f"{pit.shape[0]} rows: 1 .. {MAX_ROWS} are supported")
    if dims == 2 and not 0 < pit.shape[1] <= 65535:
        raise ValueError(f"{pit.shape[1]} outputs: 1 .. 65535 are supported")
    _cuda(pit, "pit")


def pit_calibration(pit, levels=DEFAULT_LEVELS, central=(0.5, 0.9, 0.95)):
    """pit [N]: the PIT values of one output (``predictive(...).pit[:, d]``) -> ``PitCalibration``: ``ks`` =
    max_k max(k / N - u_(k), u_(k) - (k - 1) / N); ``freq[j]`` = #{u <= levels[j]} / N; ``calibration_error`` =
    mean_j (freq[j] - levels[j])^2 (Kuleshov et al. 2018); ``coverage[i]`` = #{(1 - c_i) / 2 <= u <= (1 + c_i) / 2} / N.
    ``levels`` (at least one) and ``central`` lie in (0, 1).  Raises ``ValueError`` if a value is NaN.  One host
    synchronisation."""
    _check_pit(pit, 1)
    levels, central = _levels(levels, "levels", 1), _levels(central, "central levels", 0)
    n = pit.shape[0]
    row = _pit_columns(pit.reshape(n, 1), levels, central)[0]
    return PitCalibration(row[0].item(), row[1].item(), row[3:3 + len(levels)] / n, row[3 + len(levels):] / n)


def interval_score(lo, hi, y, c):
    """The Winkler score of the central c-interval [lo, hi] at y (Gneiting & Raftery 2007, eq. 43):
    (hi - lo) + 2 / (1 - c) [(lo - y)+ + (y - hi)+], elementwise, on the tensors' device."""
    if not all(isinstance(t, torch.Tensor) for t in (lo, hi, y)):
        raise ValueError("lo, hi and y must be tensors")
    if not 0.0 < float(c) < 1.0:
        raise ValueError("the level c must lie strictly between 0 and 1")
    return (hi - lo) + (2.0 / (1.0 - float(c))) * ((lo - y).clamp_min(0) + (y - hi).clamp_min(0))

