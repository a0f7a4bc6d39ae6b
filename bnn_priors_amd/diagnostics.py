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

__all__ = ("split_rhat", "ess", "rhat_ess", "rank_rhat_ess", "weight_space", "function_space", "summary",
           "posterior_summary", "weight_space_summary", "function_space_summary", "summary_tile", "PosteriorSummary",
           "PosteriorSummaryParts")

MAX_SEQ = _hip.DIAG_MAX_SEQ          # draws per sequence (n)
MAX_CHAINS = _hip.DIAG_MAX_CHAINS    # sequences (J): 2 M with split
LAG_BLOCK = _hip.DIAG_LAG_BLOCK
TILE = _hip.DIAG_TILE                # quantities per workgroup of the ESS kernel
RANK_CHUNK = 64                      # rank_rhat_ess walks the quantities in multiples of the score kernel's 64 lanes
RANK_DRAW_BYTES = 16                 # workspace per draw and quantity: z (fp64) and the two indicators (fp32)
RANK_QUANTITY_BYTES = 72             # ... and per quantity: six order statistics and three quantiles (fp64)
SUMMARY_MAX_DRAWS = _hip.SUMMARY_MAX_DRAWS   # draws (N = J n) that posterior_summary's column sort takes
SUMMARY_CHUNK = 64                   # posterior_summary walks the quantities in multiples of the widest sort tile
SUMMARY_DRAW_BYTES = 16              # workspace per draw and quantity: the sorted column (fp64) and c^2 (fp64), whose
#                                      place the two indicators (fp32) take once its ESS is out
SUMMARY_QUANTITY_BYTES = 0           # ... and per quantity: nothing, every result is written where it is returned
SKIP_KEYS = ("steps", "timestamps")

RankDiagnostics = collections.namedtuple("RankDiagnostics", "rhat ess_bulk ess_tail")
RankDiagnosticsParts = collections.namedtuple(
    "RankDiagnosticsParts", RankDiagnostics._fields + ("rhat_bulk", "rhat_folded", "ess_lower", "ess_upper", "median",
                                                       "q_lower", "q_upper"))
PosteriorSummary = collections.namedtuple(
    "PosteriorSummary", "mean sd mcse_mean mcse_sd ess_mean ess_sd quantiles mcse_quantile ess_quantile hdi_lower "
                        "hdi_upper")
PosteriorSummaryParts = collections.namedtuple("PosteriorSummaryParts",
                                               PosteriorSummary._fields + ("m2", "m4", "a", "b", "lo", "hi"))


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


def summary_tile(N):
    """TQ, the quantities that one workgroup of the column sort stages at N draws (``sgmcmc_summary_tile_quantities``
    restated): the most columns of N_pad fp64, N_pad the next power of two, that fit 128 KiB, at most 64"""
    if not 4 <= N <= SUMMARY_MAX_DRAWS:
        raise ValueError(f"N = {N} is outside [4, {SUMMARY_MAX_DRAWS}]")
    return min(SUMMARY_MAX_DRAWS // max(4, 1 << (N - 1).bit_length()), _hip.SUMMARY_MAX_TILE)


def _check_summary(x, split, probs, hdi_prob, workspace_bytes):
    "-> (M, S, shape, Q, probs, hdi_prob, quantities per chunk) of a valid posterior_summary call; ValueError otherwise"
    M, S, shape, Q = _check(x, split, device=False)
    try:
        probs = tuple(float(p) for p in probs)
    except (TypeError, ValueError):
        raise ValueError("probs must be a sequence of probabilities") from None
    if not all(0.0 < p < 1.0 for p in probs):
        raise ValueError(f"probs must lie inside (0, 1), not {probs!r}")
    try:
        hdi_prob = float(hdi_prob)
    except (TypeError, ValueError):
        raise ValueError("hdi_prob must be a probability") from None
    if not 0.0 < hdi_prob < 1.0:
        raise ValueError(f"hdi_prob must lie inside (0, 1), not {hdi_prob!r}")
    n, J = (S // 2, 2 * M) if split else (S, M)
    N = J * n
    if N > SUMMARY_MAX_DRAWS:
        raise ValueError(f"{J} sequences of {n} draws are {N} draws: at most {SUMMARY_MAX_DRAWS} are supported")
    if not 1 <= math.floor(hdi_prob * N) <= N - 1:
        raise ValueError(f"hdi_prob = {hdi_prob!r} covers none of the {N} draws")
    per_quantity = SUMMARY_DRAW_BYTES * N + SUMMARY_QUANTITY_BYTES
    chunk = int(workspace_bytes) // per_quantity // SUMMARY_CHUNK * SUMMARY_CHUNK
    if chunk < SUMMARY_CHUNK:
        raise ValueError(f"workspace_bytes = {workspace_bytes} is too small: {SUMMARY_CHUNK} quantities of {N} draws "
                         f"need {SUMMARY_CHUNK * per_quantity} bytes")
    _check(x, split)
    return M, S, shape, Q, probs, hdi_prob, chunk


def posterior_summary(x, probs=(0.05, 0.5, 0.95), hdi_prob=0.94, split=True, workspace_bytes=256 << 20, parts=False):
    """x [M, S, *shape] (CUDA, fp32 or fp64) -> ``PosteriorSummary``: what the posterior of every quantity is and how
    precisely the M S stored draws pin it down, as ``include/sgmcmc_hip.h`` defines it (Vehtari et al. 2021; the R package
    posterior; ArviZ's unimodal HDI).  ``mean``, ``sd``, their Monte Carlo standard errors ``mcse_mean``, ``mcse_sd`` and
    the effective sample sizes behind those, ``ess_mean``, ``ess_sd``, each [*shape]; ``quantiles``, ``mcse_quantile``
    and ``ess_quantile``, each [P, *shape], for the P probabilities ``probs``; ``hdi_lower``, ``hdi_upper``: the
    narrowest interval that holds ``hdi_prob`` of the draws.  All fp64.  Next to ``rhat_ess`` / ``rank_rhat_ess`` this
    is the usual summary table; whether two priors differ by more than the sampler's noise is a question about
    ``mcse_mean``.

    ``parts=True``: a ``PosteriorSummaryParts`` that also carries ``m2``, ``m4`` (the central moments), ``a``, ``b``
    (the beta quantiles behind ``mcse_quantile``, [P, *shape]) and ``lo``, ``hi`` (its two ranks, int32, [P, *shape]).
    ``split`` chooses the sequences of the effective sample sizes as in ``rhat_ess`` (with an odd S a chain's middle
    draw enters nothing).  The columns are sorted by an LDS sorting network, so at most 16384 draws enter.  The
    quantities are walked in chunks (multiples of 64) whose sorted columns and scratch fit ``workspace_bytes``: one
    workspace per call, 16 bytes per draw and quantity; the chunking changes no bit.  A quantity with a non-finite draw
    gives NaN in everything; a constant one its mean and quantiles, ``sd`` = 0 and NaN for every ess and mcse.
    Everything stays on the current stream."""
    split = bool(split)
    M, S, shape, Q, probs, hdi_prob, chunk = _check_summary(x, split, probs, hdi_prob, workspace_bytes)
    dev = x.device
    n, J = (S // 2, 2 * M) if split else (S, M)
    N, P = J * n, len(probs)
    res = torch.empty((10 + 5 * P, Q), dtype=torch.float64, device=dev)
    ranks = torch.empty((2 * P, Q), dtype=torch.int32, device=dev)
    if Q:
        if not x[0, 0].is_contiguous():
            x = x.contiguous()
        chunk = min(chunk, (Q + SUMMARY_CHUNK - 1) // SUMMARY_CHUNK * SUMMARY_CHUNK)
        work = torch.empty(chunk * (SUMMARY_DRAW_BYTES * N + SUMMARY_QUANTITY_BYTES) // 8, dtype=torch.float64,
                           device=dev)
        item, is_f64 = x.element_size(), int(x.dtype == torch.float64)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            L = _hip.lib()

            def run(name, *args):
                _hip.check(getattr(L, name)(*args, stream), name)

            for q0 in range(0, Q, chunk):
                Qc = min(chunk, Q - q0)
                ordered = work.data_ptr()                                     # [N][Qc] fp64: the sorted columns
                csq = ordered + 8 * N * Qc                                    # [J][n][Qc] fp64: c^2, and after its ESS ...
                ind = (csq, csq + 4 * N * Qc)                                 # ... [J][n][Qc] fp32 twice: two indicators
                seqs = (x.data_ptr() + q0 * item, is_f64, x.stride(0), x.stride(1), M, S, Qc, int(split))
                mean, sd, mcse_mean, mcse_sd, ess_mean, ess_sd, hdi_lower, hdi_upper, m2, m4 = (
                    res[r].data_ptr() + 8 * q0 for r in range(10))
                quant, mcse_q, ess_q, a, b = ([res[10 + g * P + k].data_ptr() + 8 * q0 for k in range(P)]
                                              for g in range(5))
                lo, hi = ([ranks[g * P + k].data_ptr() + 4 * q0 for k in range(P)] for g in range(2))
                shape_args = (M, S, int(split))
                run("sgmcmc_summary_sort", *seqs, ordered)
                run("sgmcmc_summary_moments", *seqs, mean, sd, m2, m4, csq)
                run("sgmcmc_chain_ess", *seqs, ess_mean, None, None)
                run("sgmcmc_chain_ess", csq, 1, n * Qc, Qc, J, n, Qc, 0, ess_sd, None, None)
                run("sgmcmc_summary_mcse", sd, m2, m4, ess_mean, ess_sd, Qc, mcse_mean, mcse_sd)
                run("sgmcmc_summary_hdi", ordered, *shape_args, hdi_prob, Qc, hdi_lower, hdi_upper)
                for k in range(P):
                    run("sgmcmc_summary_quantile", ordered, *shape_args, probs[k], Qc, quant[k])
                for k in range(0, P, 2):                                      # the indicators of two thresholds at once
                    k2 = min(k + 1, P - 1)
                    run("sgmcmc_chain_tail_indicators", *seqs, quant[k], quant[k2], *ind)
                    for kk, src in ((k, ind[0]), (k2, ind[1]))[:k2 - k + 1]:
                        run("sgmcmc_chain_ess", src, 0, n * Qc, Qc, J, n, Qc, 0, ess_q[kk], None, None)
                for k in range(P):
                    run("sgmcmc_summary_mcse_quantile", ordered, *shape_args, probs[k], ess_q[k], Qc, mcse_q[k], a[k],
                        b[k], lo[k], hi[k])
    one = [t.reshape(shape) for t in res[:10]]
    many = [res[10 + g * P:10 + (g + 1) * P].reshape((P,) + shape) for g in range(5)]
    lo, hi = (ranks[g * P:(g + 1) * P].reshape((P,) + shape) for g in range(2))
    out = one[:6] + many[:3] + one[6:8]
    return PosteriorSummaryParts(*out, one[8], one[9], many[3], many[4], lo, hi) if parts else PosteriorSummary(*out)


def _diagnosable(name, v):
    return (name not in SKIP_KEYS and isinstance(v, torch.Tensor) and v.is_floating_point()
            and not name.endswith("num_batches_tracked"))


def _stacked(samples, chains):
    "``weight_space``' input -> {name: [M, S, ...]} of the tensors that are diagnosed; ValueError for a malformed one"
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
    return stacked


def weight_space(samples, chains=None, split=True, rank_normalised=False):
    """R-hat and ESS of every stored weight: ``{name: (rhat, ess)}``, each shaped like the weight; with
    ``rank_normalised=True`` ``{name: rank_rhat_ess(...)}``, the ``(rhat, ess_bulk, ess_tail)`` that heavy-tailed
    weights need.

    ``samples``: a list of per-chain sample dicts (``runner.get_samples()``: name -> [S, ...]), stacked chain by chain;
    or ONE dict in ``evaluation.gather_samples``' layout (name -> [M S, ...], chain by chain) with ``chains=M``, viewed
    as [M, S, ...] without a copy.  The bookkeeping keys (``steps``, ``timestamps``), integer tensors and the BatchNorm
    counters are skipped."""
    stacked = _stacked(samples, chains)
    for name, v in stacked.items():
        _check(v, bool(split))                   # every tensor is checked before the first launch
    if rank_normalised:
        return {name: rank_rhat_ess(v, split) for name, v in stacked.items()}
    return {name: rhat_ess(v, split) for name, v in stacked.items()}


def function_space(tables, split=True, rank_normalised=False):
    """``tables``: a list of per-chain ``acc`` [S, N, C] (``evaluation.predictive_tables``: normalised
    log-probabilities per sample) -> (R-hat, ESS) of the predictive probabilities ``exp(acc)``, each [N, C]; with
    ``rank_normalised=True`` their ``rank_rhat_ess``: ``(rhat, ess_bulk, ess_tail)``."""
    tables = _tables(tables)
    if rank_normalised:
        return rank_rhat_ess(torch.stack(tables).exp(), split)
    return rhat_ess(torch.stack(tables).exp(), split)


def _tables(tables):
    tables = list(tables)
    if not tables or any(not isinstance(a, torch.Tensor) or a.dim() != 3 or a.shape != tables[0].shape
                         or a.dtype != tables[0].dtype for a in tables):
        raise ValueError("tables must be a non-empty list of [S, N, C] tensors of one shape and dtype")
    return tables


def weight_space_summary(samples, chains=None, split=True, **kw):
    """``posterior_summary`` of every stored weight: ``{name: PosteriorSummary}``, every field shaped like the weight
    (the per-probability ones with a leading P).  ``samples`` and ``chains`` are ``weight_space``'s, with the same skips;
    ``kw`` goes to ``posterior_summary`` (``probs``, ``hdi_prob``, ``workspace_bytes``, ``parts``)."""
    stacked = _stacked(samples, chains)
    args = (kw.get("probs", (0.05, 0.5, 0.95)), kw.get("hdi_prob", 0.94), kw.get("workspace_bytes", 256 << 20))
    for name, v in stacked.items():
        _check_summary(v, bool(split), *args)    # every tensor is checked before the first launch
    return {name: posterior_summary(v, split=split, **kw) for name, v in stacked.items()}


def function_space_summary(tables, split=True, **kw):
    """``tables``: a list of per-chain ``acc`` [S, N, C] (``evaluation.predictive_tables``) -> the ``posterior_summary``
    of the predictive probabilities ``exp(acc)``, every field [N, C] (or [P, N, C]).  Its ``mean`` is the ensemble's
    predictive probability, its ``mcse_mean`` how well the S draws per chain determine that probability."""
    return posterior_summary(torch.stack(_tables(tables)).exp(), split=split, **kw)


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
