"""Between-chain diagnostics of stored draws on the device (``csrc/diag_hip.inc``, ``csrc/rank_hip.inc``; C ABI
``sgmcmc_chain_rhat`` / ``sgmcmc_chain_ess`` and ``sgmcmc_chain_rank_scores`` / ``sgmcmc_chain_quantiles`` /
``sgmcmc_chain_tail_indicators``): split-R-hat and the effective sample size, per quantity, of ``M`` chains x ``S``
draws -- in weight space (``weight_space``) or in function space, on the per-sample predictive probabilities
(``function_space``).  The reference has no such function; ``include/sgmcmc_hip.h`` states both definitions: the
moment-based one (Gelman et al., BDA3 section 11.4-11.5; Geyer's initial monotone sequence; ``rhat_ess``) and the
rank-normalised one with bulk and tail ESS (Vehtari et al. 2021; ``rank_rhat_ess``), which is the one to read for
heavy-tailed weights.

Everything runs in fp64 in an order fixed by ``(M, S, split)``: two calls give the same bits, and a quantity's result
does not depend on which other quantities are in the call.  Nothing here synchronises with the host except
``summary``.  Chains that live on several ranks go through ``evaluation.gather_samples`` first.
"""
import collections
import ctypes
import math

import torch

from . import _hip

__all__ = ("split_rhat", "ess", "rhat_ess", "rank_rhat_ess", "weight_space", "function_space", "summary")

MAX_SEQ = _hip.DIAG_MAX_SEQ          # draws per sequence (n)
MAX_CHAINS = _hip.DIAG_MAX_CHAINS    # sequences (J): 2 M with split
LAG_BLOCK = _hip.DIAG_LAG_BLOCK
TILE = _hip.DIAG_TILE                # quantities per workgroup of the ESS kernel
RANK_CHUNK = 64                      # rank_rhat_ess walks the quantities in multiples of the score kernel's 64 lanes
RANK_DRAW_BYTES = 16                 # workspace per draw and quantity: z (fp64) and the two indicators (fp32)
RANK_QUANTITY_BYTES = 72             # ... and per quantity: six order statistics and three quantiles (fp64)
SKIP_KEYS = ("steps", "timestamps")

RankDiagnostics = collections.namedtuple("RankDiagnostics", "rhat ess_bulk ess_tail")
RankDiagnosticsParts = collections.namedtuple(
    "RankDiagnosticsParts", RankDiagnostics._fields + ("rhat_bulk", "rhat_folded", "ess_lower", "ess_upper", "median",
                                                       "q_lower", "q_upper"))


def _check(x, split, device=True):
    """-> (M, S, shape, Q) of a valid input; ValueError otherwise, before the library is touched (``device=False``: the
    caller has more to check before the last test, that x is on the device)"""
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
    if device and not x.is_cuda:
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


def _check_rank(x, split, tail_probs, workspace_bytes):
    "-> (M, S, shape, Q, probs, quantities per chunk) of a valid rank_rhat_ess call; ValueError otherwise"
    M, S, shape, Q = _check(x, split, device=False)
    try:
        probs = tuple(float(p) for p in tail_probs)
    except (TypeError, ValueError):
        raise ValueError("tail_probs must be two probabilities") from None
    if len(probs) != 2 or not all(0.0 < p < 1.0 for p in probs):
        raise ValueError(f"tail_probs must be two probabilities inside (0, 1), not {tail_probs!r}")
    if not probs[0] < probs[1]:
        raise ValueError(f"tail_probs must be increasing, not {tail_probs!r}")
    n, J = (S // 2, 2 * M) if split else (S, M)
    per_quantity = RANK_DRAW_BYTES * J * n + RANK_QUANTITY_BYTES
    chunk = int(workspace_bytes) // per_quantity // RANK_CHUNK * RANK_CHUNK
    if chunk < RANK_CHUNK:
        raise ValueError(f"workspace_bytes = {workspace_bytes} is too small: {RANK_CHUNK} quantities of {J * n} draws "
                         f"need {RANK_CHUNK * per_quantity} bytes")
    _check(x, split)
    return M, S, shape, Q, probs, chunk


def rank_rhat_ess(x, split=True, tail_probs=(0.05, 0.95), workspace_bytes=256 << 20, parts=False):
    """x [M, S, *shape] (CUDA, fp32 or fp64) -> ``RankDiagnostics(rhat, ess_bulk, ess_tail)``, each [*shape] fp64: the
    rank-normalised R-hat (the larger of the bulk and the folded part), the bulk ESS and the tail ESS of Vehtari et al.
    (2021), as ``include/sgmcmc_hip.h`` defines them.  Unlike ``rhat_ess`` they need no finite mean or variance of the
    draws, and the folded part and the tail ESS see chains that differ in scale or mix badly in the tails.

    ``tail_probs``: the two quantile probabilities of the tail ESS.  ``parts=True``: a ``RankDiagnosticsParts`` that
    also carries ``rhat_bulk``, ``rhat_folded``, ``ess_lower``, ``ess_upper``, ``median``, ``q_lower``, ``q_upper``.
    The quantities are walked in chunks (multiples of 64) whose scores and indicators fit ``workspace_bytes``: one
    workspace per call, 16 bytes per draw and quantity plus 72 per quantity; the chunking changes no bit.  A quantity
    with a non-finite draw gives NaN in all three; a constant quantity a NaN ``rhat``; a constant tail indicator (enough
    draws tied at an extreme) a NaN ``ess_tail``.  Everything stays on the current stream."""
    split = bool(split)
    M, S, shape, Q, probs, chunk = _check_rank(x, split, tail_probs, workspace_bytes)
    dev = x.device
    n, J = (S // 2, 2 * M) if split else (S, M)
    N = J * n
    res = torch.empty((10, Q), dtype=torch.float64, device=dev)
    rhat, ess_bulk, ess_tail, rhat_bulk, rhat_folded, ess_lower, ess_upper = res[:7]
    quantiles = res[7:]                                      # median, q_lower, q_upper
    if Q:
        if not x[0, 0].is_contiguous():
            x = x.contiguous()
        chunk = min(chunk, (Q + RANK_CHUNK - 1) // RANK_CHUNK * RANK_CHUNK)
        work = torch.empty(chunk * (RANK_DRAW_BYTES * N + RANK_QUANTITY_BYTES) // 8, dtype=torch.float64, device=dev)
        item, is_f64 = x.element_size(), int(x.dtype == torch.float64)
        all_probs = (ctypes.c_double * 3)(0.5, *probs)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            L = _hip.lib()
            for q0 in range(0, Q, chunk):
                Qc = min(chunk, Q - q0)
                z = work.data_ptr()                                           # [J][n][Qc] fp64
                lower, upper = z + 8 * N * Qc, z + 12 * N * Qc                # [J][n][Qc] fp32 each
                ostat = z + 16 * N * Qc                                       # [6][Qc] fp64
                quant = ostat + 48 * Qc                                       # [3][Qc] fp64
                seqs = (x.data_ptr() + q0 * item, is_f64, x.stride(0), x.stride(1), M, S, Qc, int(split))
                out = [t.data_ptr() + 8 * q0 for t in res]
                _hip.check(L.sgmcmc_chain_rank_scores(*seqs, None, all_probs, 3, z, ostat, stream),
                           "sgmcmc_chain_rank_scores")
                _hip.check(L.sgmcmc_chain_quantiles(ostat, M, S, int(split), all_probs, 3, Qc, quant, stream),
                           "sgmcmc_chain_quantiles")
                _hip.check(L.sgmcmc_chain_ess(z, 1, n * Qc, Qc, J, n, Qc, 0, out[1], out[3], None, stream),
                           "sgmcmc_chain_ess")
                _hip.check(L.sgmcmc_chain_rank_scores(*seqs, quant, None, 0, z, None, stream),
                           "sgmcmc_chain_rank_scores")
                _hip.check(L.sgmcmc_chain_rhat(z, 1, n * Qc, Qc, J, n, Qc, 0, out[4], stream), "sgmcmc_chain_rhat")
                _hip.check(L.sgmcmc_chain_tail_indicators(*seqs, quant + 8 * Qc, quant + 16 * Qc, lower, upper,
                                                          stream), "sgmcmc_chain_tail_indicators")
                for ind, o in ((lower, out[5]), (upper, out[6])):
                    _hip.check(L.sgmcmc_chain_ess(ind, 0, n * Qc, Qc, J, n, Qc, 0, o, None, None, stream),
                               "sgmcmc_chain_ess")
                quantiles[:, q0:q0 + Qc].copy_(work[(16 * N * Qc + 48 * Qc) // 8:][:3 * Qc].view(3, Qc))
        torch.maximum(rhat_bulk, rhat_folded, out=rhat)                       # both propagate a NaN of either part
        torch.minimum(ess_lower, ess_upper, out=ess_tail)
    out = [t.reshape(shape) for t in res]
    return RankDiagnosticsParts(*out) if parts else RankDiagnostics(*out[:3])


def _diagnosable(name, v):
    return (name not in SKIP_KEYS and isinstance(v, torch.Tensor) and v.is_floating_point()
            and not name.endswith("num_batches_tracked"))


def weight_space(samples, chains=None, split=True, rank_normalised=False):
    """R-hat and ESS of every stored weight: ``{name: (rhat, ess)}``, each shaped like the weight; with
    ``rank_normalised=True`` ``{name: rank_rhat_ess(...)}``, the ``(rhat, ess_bulk, ess_tail)`` that heavy-tailed
    weights need.

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
    if rank_normalised:
        return {name: rank_rhat_ess(v, split) for name, v in stacked.items()}
    return {name: rhat_ess(v, split) for name, v in stacked.items()}


def function_space(tables, split=True, rank_normalised=False):
    """``tables``: a list of per-chain ``acc`` [S, N, C] (``evaluation.predictive_tables``: normalised
    log-probabilities per sample) -> (R-hat, ESS) of the predictive probabilities ``exp(acc)``, each [N, C]; with
    ``rank_normalised=True`` their ``rank_rhat_ess``: ``(rhat, ess_bulk, ess_tail)``."""
    tables = list(tables)
    if not tables or any(not isinstance(a, torch.Tensor) or a.dim() != 3 or a.shape != tables[0].shape
                         or a.dtype != tables[0].dtype for a in tables):
        raise ValueError("tables must be a non-empty list of [S, N, C] tensors of one shape and dtype")
    if rank_normalised:
        return rank_rhat_ess(torch.stack(tables).exp(), split)
    return rhat_ess(torch.stack(tables).exp(), split)


def summary(rhat, ess, ess_tail=None):
    """Plain floats after one synchronisation: ``rhat_max``, ``rhat_q99``, ``rhat_above_1_01`` / ``rhat_above_1_1``
    (shares of the quantities), ``ess_min``, ``ess_median`` and ``nan`` (how many quantities have a NaN in either
    tensor).  NaNs are excluded from the other statistics (all NaN: those statistics are NaN).  ``ess`` may be
    ``rank_rhat_ess``' ``ess_bulk``; its ``ess_tail`` adds ``ess_tail_min``, the smallest that is not NaN (NaN if all
    are), and changes nothing else."""
    if not all(isinstance(v, torch.Tensor) for v in (rhat, ess)) or rhat.shape != ess.shape:
        raise ValueError("rhat and ess must be tensors of one shape")
    if ess_tail is not None and (not isinstance(ess_tail, torch.Tensor) or ess_tail.shape != rhat.shape):
        raise ValueError("ess_tail must be a tensor shaped like rhat")
    r, e = rhat.reshape(-1).to(torch.float64), ess.reshape(-1).to(torch.float64)
    ok = ~(torch.isnan(r) | torch.isnan(e))
    count = ok.sum()
    nan = float("nan")
    keys = ("rhat_max", "rhat_q99", "rhat_above_1_01", "rhat_above_1_1", "ess_min", "ess_median", "nan")
    if r.numel() == 0:
        return dict(zip(keys, (nan,) * 6 + (0,)), **({} if ess_tail is None else {"ess_tail_min": nan}))
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
    stats = [rs[last], q99, above[0], above[1], es[0], (es[mid_lo] + es[mid_hi]) / 2, r.numel() - cnt]
    if ess_tail is not None:
        t = ess_tail.reshape(-1).to(torch.float64)
        stats.append(torch.where(torch.isnan(t), torch.full_like(t, math.inf), t).min())
    stats = torch.stack(stats).cpu().tolist()
    if stats[6] == r.numel():
        stats[:6] = [nan] * 6
    out = dict(zip(keys, stats[:6] + [int(stats[6])]))
    if ess_tail is not None:
        out["ess_tail_min"] = nan if math.isinf(stats[7]) else stats[7]
    return out
