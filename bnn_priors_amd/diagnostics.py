"""Between-chain diagnostics of stored draws on the device (``csrc/diag_hip.inc``; C ABI ``sgmcmc_chain_rhat`` /
``sgmcmc_chain_ess``): split-R-hat and the effective sample size, per quantity, of ``M`` chains x ``S`` draws -- in
weight space (``weight_space``) or in function space, on the per-sample predictive probabilities
(``function_space``).  The reference has no such function; ``include/sgmcmc_hip.h`` states the definition (Gelman et
al., BDA3 section 11.4-11.5; Geyer's initial monotone sequence; no rank normalisation).

Everything runs in fp64 in an order fixed by ``(M, S, split)``: two calls give the same bits, and a quantity's result
does not depend on which other quantities are in the call.  Nothing here synchronises with the host except
``summary``.  Chains that live on several ranks go through ``evaluation.gather_samples`` first.
"""
import math

import torch

from . import _hip

__all__ = ("split_rhat", "ess", "rhat_ess", "weight_space", "function_space", "summary")

MAX_SEQ = _hip.DIAG_MAX_SEQ          # draws per sequence (n)
MAX_CHAINS = _hip.DIAG_MAX_CHAINS    # sequences (J): 2 M with split
LAG_BLOCK = _hip.DIAG_LAG_BLOCK
TILE = _hip.DIAG_TILE                # quantities per workgroup of the ESS kernel
SKIP_KEYS = ("steps", "timestamps")


def _check(x, split):
    "-> (M, S, shape, Q) of a valid input; ValueError otherwise, before the library is touched"
    if not isinstance(x, torch.Tensor):
        raise ValueError("x must be a tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"x must be float32 or float64, not {x.dtype}")
    if x.dim() < 2:
        raise ValueError("x must be [chains, draws, ...]")
    M, S = x.shape[:2]
    n, J = (S // 2, 2 * M) if split else (S, M)
    if M < 1:
        raise ValueError("x needs at least one chain")
    if n < 4:
        raise ValueError(f"{S} draws give sequences of {n}: at least 4 are needed")
    if n > MAX_SEQ:
        raise ValueError(f"{S} draws give sequences of {n}: at most {MAX_SEQ} are supported")
    if J > MAX_CHAINS:
        raise ValueError(f"{M} chains give {J} sequences: at most {MAX_CHAINS} are supported")
    if not x.is_cuda:
        raise ValueError("x must be a CUDA tensor")
    shape = tuple(x.shape[2:])
    return M, S, shape, math.prod(shape)


def _run(x, split, want_ess, want_pairs=False):
    split = bool(split)
    M, S, shape, Q = _check(x, split)
    dev = x.device
    rhat = torch.empty(shape, dtype=torch.float64, device=dev)
    if not want_ess:
        out = (rhat,)
    else:
        out = (rhat, torch.empty(shape, dtype=torch.float64, device=dev))
        if want_pairs:
            out += (torch.empty(shape, dtype=torch.int32, device=dev),)
    if Q == 0:
        return out
    if not x[0, 0].is_contiguous():          # the trailing dims are one contiguous run of Q elements, or are made so
        x = x.contiguous()
    args = (x.data_ptr(), int(x.dtype == torch.float64), x.stride(0), x.stride(1), M, S, Q, int(split))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        if want_ess:
            err = _hip.lib().sgmcmc_chain_ess(*args, out[1].data_ptr(), rhat.data_ptr(),
                                              out[2].data_ptr() if want_pairs else 0, stream)
            _hip.check(err, "sgmcmc_chain_ess")
        else:
            _hip.check(_hip.lib().sgmcmc_chain_rhat(*args, rhat.data_ptr(), stream), "sgmcmc_chain_rhat")
    return out


def split_rhat(x, split=True):
    """x [M, S, *shape] (CUDA, fp32 or fp64; M chains, S draws) -> R-hat [*shape] fp64 of the 2 M half-chains
    (``split=False``: of the M chains).  One streaming pass pair over the data."""
    return _run(x, split, False)[0]


def rhat_ess(x, split=True, pairs=False):
    """x [M, S, *shape] -> (R-hat, ESS), each [*shape] fp64; with ``pairs=True`` also K [*shape] int32, the number of
    Geyer pairs that entered the autocorrelation time.  A quantity with a non-finite draw, or whose draws do not vary,
    gives NaN for both."""
    return _run(x, split, True, pairs)


def ess(x, split=True):
    "x [M, S, *shape] -> the effective sample size [*shape] fp64 of the M S draws (with ``split``: of 2 M (S // 2))"
    return _run(x, split, True)[1]


def _diagnosable(name, v):
    return (name not in SKIP_KEYS and isinstance(v, torch.Tensor) and v.is_floating_point()
            and not name.endswith("num_batches_tracked"))


def weight_space(samples, chains=None, split=True):
    """R-hat and ESS of every stored weight: ``{name: (rhat, ess)}``, each shaped like the weight.

    ``samples``: a list of per-chain sample dicts (``runner.get_samples()``: name -> [S, ...]), stacked chain by chain;
    or ONE dict in ``evaluation.gather_samples``' layout (name -> [M S, ...], chain by chain) with ``chains=M``, viewed
    as [M, S, ...] without a copy.  The bookkeeping keys (``steps``, ``timestamps``), integer tensors and the BatchNorm
    counters are skipped."""
    if isinstance(samples, dict):
        if chains is None or int(chains) < 1:
            raise ValueError("one dict of gathered samples needs chains=M")
        M = int(chains)
        stacked = {}
        for name, v in samples.items():
            if not _diagnosable(name, v):
                continue
            if v.dim() < 1 or v.shape[0] % M:
                raise ValueError(f"{name}: {tuple(v.shape)} does not hold {M} chains of equal length")
            stacked[name] = v.unflatten(0, (M, v.shape[0] // M))
    else:
        samples = list(samples)
        if chains is not None and int(chains) != len(samples):
            raise ValueError(f"chains={chains} but {len(samples)} sample dicts were given")
        if not samples or not all(isinstance(s, dict) for s in samples):
            raise ValueError("samples must be a dict or a non-empty list of dicts")
        names = [k for k, v in samples[0].items() if _diagnosable(k, v)]
        stacked = {}
        for name in names:
            vs = [s.get(name) for s in samples]
            if any(not isinstance(v, torch.Tensor) or v.shape != vs[0].shape or v.dtype != vs[0].dtype for v in vs):
                raise ValueError(f"{name}: the chains' samples differ in shape or dtype")
            stacked[name] = torch.stack(vs)
    for name, v in stacked.items():
        _check(v, bool(split))                   # every tensor is checked before the first launch
    return {name: rhat_ess(v, split) for name, v in stacked.items()}


def function_space(tables, split=True):
    """``tables``: a list of per-chain ``acc`` [S, N, C] (``evaluation.predictive_tables``: normalised
    log-probabilities per sample) -> (R-hat, ESS) of the predictive probabilities ``exp(acc)``, each [N, C]."""
    tables = list(tables)
    if not tables or any(not isinstance(a, torch.Tensor) or a.dim() != 3 or a.shape != tables[0].shape
                         or a.dtype != tables[0].dtype for a in tables):
        raise ValueError("tables must be a non-empty list of [S, N, C] tensors of one shape and dtype")
    return rhat_ess(torch.stack(tables).exp(), split)


def summary(rhat, ess):
    """Plain floats after one synchronisation: ``rhat_max``, ``rhat_q99``, ``rhat_above_1_01`` / ``rhat_above_1_1``
    (shares of the quantities), ``ess_min``, ``ess_median`` and ``nan`` (how many quantities have a NaN in either
    tensor).  NaNs are excluded from the other statistics (all NaN: those statistics are NaN)."""
    if not all(isinstance(v, torch.Tensor) for v in (rhat, ess)) or rhat.shape != ess.shape:
        raise ValueError("rhat and ess must be tensors of one shape")
    r, e = rhat.reshape(-1).to(torch.float64), ess.reshape(-1).to(torch.float64)
    ok = ~(torch.isnan(r) | torch.isnan(e))
    count = ok.sum()
    nan = float("nan")
    keys = ("rhat_max", "rhat_q99", "rhat_above_1_01", "rhat_above_1_1", "ess_min", "ess_median", "nan")
    if r.numel() == 0:
        return dict(zip(keys, (nan,) * 6 + (0,)))
    # NaN -> a filler that cannot win; quantiles over the sorted finite part, by position (count is still on the device)
    rs = torch.where(ok, r, torch.full_like(r, math.inf)).sort().values
    es = torch.where(ok, e, torch.full_like(e, math.inf)).sort().values
    last = (count - 1).clamp(min=0)
    pos = last.to(torch.float64) * 0.99                       # np.quantile's linear interpolation
    lo = pos.floor().long()
    hi = torch.minimum(lo + 1, last)
    frac = pos - lo.to(torch.float64)
    q99 = rs[lo] + (rs[hi] - rs[lo]) * frac
    mid_lo, mid_hi = last // 2, (last + 1) // 2               # np.median: the mean of the two middle values
    cnt = count.to(torch.float64)
    above = [((r > bound) & ok).sum().to(torch.float64) / cnt for bound in (1.01, 1.1)]
    stats = torch.stack([rs[last], q99, above[0], above[1], es[0], (es[mid_lo] + es[mid_hi]) / 2,
                         r.numel() - cnt]).cpu().tolist()
    if stats[6] == r.numel():
        stats[:6] = [nan] * 6
    return dict(zip(keys, stats[:6] + [int(stats[6])]))
