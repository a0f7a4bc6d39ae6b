"""Model comparison from the pointwise log-likelihoods of the stored draws, on the device (``csrc/psis_hip.inc``; C ABI
``sgmcmc_psis_loo`` / ``sgmcmc_psis_totals``): Pareto-smoothed importance-sampling leave-one-out cross-validation
(PSIS-LOO: Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024) and WAIC (Watanabe 2010), each
with a standard error, the Pareto-k of every observation, and paired differences between models (``compare``).  The
input is what ``evaluation.predictive_tables`` produces, ``lps [E, N]`` in fp64; ``include/sgmcmc_hip.h`` states the
definition and ``tests/psis_reference.py`` restates it in numpy.  The reference has nothing of the kind.

Everything runs in fp64 in a fixed order: two calls give the same bits, an observation's result does not depend on
which other observations are in the call, and the chunking changes no bit.  Only the totals cross to the host (one
synchronisation per ``loo`` / ``waic`` / ``compare``).

Model averaging from the same pointwise rows (``csrc/weights_hip.inc``; Yao, Vehtari, Simpson & Gelman 2018):
``stacking_weights``, ``pseudo_bma_weights``, ``bb_pseudo_bma_weights`` (pseudo-BMA+ with the Bayesian bootstrap),
``mixture_lpd`` and ``model_weights`` on ``compare``'s input; ``tests/weights_reference.py`` restates them.
"""
import collections
import math

import torch

from . import _hip, diagnostics

__all__ = ("psis", "relative_eff", "loo", "waic", "loo_waic", "compare", "LooResult", "WaicResult", "CompareRow",
           "pointwise_matrix", "stacking_weights", "pseudo_bma_weights", "bb_pseudo_bma_weights", "mixture_lpd",
           "model_weights", "StackingResult", "BootstrapResult")

MIN_DRAWS, MAX_DRAWS, MAX_TAIL = _hip.PSIS_MIN_DRAWS, _hip.PSIS_MAX_DRAWS, _hip.PSIS_MAX_TAIL
CHUNK = 64                           # a chunk of observations is a multiple of the kernels' 64 lanes
EFF_CHUNK_BYTES = 64 << 20           # relative_eff: the exp table of one chunk of observations
ROWS = ("pareto_k", "elpd_loo", "lppd", "p_loo", "p_waic", "elpd_waic")                 # of the pointwise table
TOTALS = ("elpd_loo", "se_loo", "p_loo", "lppd", "elpd_waic", "se_waic", "p_waic", "n_bad", "k_max")

LooResult = collections.namedtuple("LooResult", "elpd_loo se p_loo lppd pointwise pareto_k k_threshold n_bad k_max")
WaicResult = collections.namedtuple("WaicResult", "elpd_waic se p_waic pointwise")
CompareRow = collections.namedtuple("CompareRow", "name elpd se elpd_diff dse")


def tail_rows(S, has_r_eff):
    "rows of the tail workspace: an upper bound of every observation's M"
    fifth = 0.2 * S
    return min(math.ceil(fifth if has_r_eff else min(fifth, 3.0 * math.sqrt(S))), MAX_TAIL)


def bytes_per_observation(S, has_r_eff):
    "workspace per observation: the tail's rows (fp64), the column record, and a uint16 per draw"
    return 8 * tail_rows(S, has_r_eff) + 64 + 2 * S


def k_threshold(S):
    "the Pareto-k above which S draws do not give a reliable estimate (Vehtari et al. 2024)"
    return min(1.0 - 1.0 / math.log10(S), 0.7)


def _check(x, r_eff, workspace_bytes, what="lps"):
    "-> (table [E, N] as a view where possible, E, N); ValueError otherwise, before the library is touched"
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be float32 or float64, not {x.dtype}")
    if x.dim() not in (2, 3):
        raise ValueError(f"{what} must be [draws, observations] or [chains, draws, observations]")
    E, N = math.prod(x.shape[:-1]), x.shape[-1]
    if not MIN_DRAWS <= E <= MAX_DRAWS:
        raise ValueError(f"{E} draws: between {MIN_DRAWS} and {MAX_DRAWS} are supported")
    if N < 1:
        raise ValueError(f"{what} needs at least one observation")
    if r_eff is not None:
        if not isinstance(r_eff, torch.Tensor) or r_eff.dtype != torch.float64 or tuple(r_eff.shape) != (N,):
            raise ValueError(f"r_eff must be a float64 tensor of shape [{N}]")
        if r_eff.device != x.device:
            raise ValueError(f"r_eff must be on {what}'s device")
    per = bytes_per_observation(E, r_eff is not None)
    if int(workspace_bytes) < per * min(N, CHUNK):
        raise ValueError(f"workspace_bytes = {workspace_bytes} is too small: {min(N, CHUNK)} observations of {E} draws "
                         f"need {per * min(N, CHUNK)} bytes")
    if not x.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor")
    if x.dim() == 3:
        # [M, S, N] read in place as M S draws when the chains lie one draw stride apart
        if x.stride(2) == 1 and x.stride(1) >= N and x.stride(0) == x.shape[1] * x.stride(1):
            x = x.as_strided((E, N), (x.stride(1), 1))
        else:
            x = x.reshape(E, N)
    if x.stride(1) != 1 or x.stride(0) < N:
        x = x.contiguous()
    return x, E, N


def _run(x, r_eff, workspace_bytes, is_ratio=False, want_lw=False, what="lps"):
    "-> (pointwise [6, N], totals [9] or None, lw [E, N] or None), all on the device"
    x, E, N = _check(x, r_eff, workspace_bytes, what)
    dev = x.device
    per = bytes_per_observation(E, r_eff is not None)
    chunk = N if per * N <= int(workspace_bytes) else int(workspace_bytes) // per // CHUNK * CHUNK
    work = torch.empty((per * chunk + 7) // 8, dtype=torch.float64, device=dev)
    pointwise = torch.empty((len(ROWS), N), dtype=torch.float64, device=dev)
    lw = torch.empty((E, N), dtype=torch.float64, device=dev) if want_lw else None
    totals = None if is_ratio else torch.empty(len(TOTALS), dtype=torch.float64, device=dev)
    if r_eff is not None:
        r_eff = r_eff.contiguous()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        L = _hip.lib()
        _hip.check(L.sgmcmc_psis_loo(x.data_ptr(), int(x.dtype == torch.float64), int(is_ratio), x.stride(0), E, N,
                                     r_eff.data_ptr() if r_eff is not None else None, work.data_ptr(),
                                     work.numel() * 8, pointwise.data_ptr(), None, None,
                                     lw.data_ptr() if want_lw else None, stream), "sgmcmc_psis_loo")
        if totals is not None:
            _hip.check(L.sgmcmc_psis_totals(pointwise.data_ptr(), N, k_threshold(E), totals.data_ptr(), stream),
                       "sgmcmc_psis_totals")
    return pointwise, totals, lw


def psis(log_ratios, r_eff=None, workspace_bytes=256 << 20):
    """log_ratios [E, N], or [M, S, N] read in place as E = M S draws (CUDA, fp32 or fp64) -> (log_weights [E, N],
    pareto_k [N]), fp64: the Pareto-smoothed, truncated and normalised log importance weights of every column
    (``logsumexp`` over the draws is 0) and the shape khat of the generalised Pareto distribution fitted to its tail
    (+inf where the tail has at most four draws).  ``r_eff [N]`` (fp64, on the same device): the relative efficiency
    that sets the tail's length M = ceil(min(0.2 E, 3 sqrt(E / r_eff))); None means 1.  The observations are walked in
    chunks (multiples of 64) whose workspace -- 8 M + 64 + 2 E bytes per observation -- fits ``workspace_bytes``; the
    chunking changes no bit.  A column with a non-finite value gives NaN."""
    pointwise, _, lw = _run(log_ratios, r_eff, workspace_bytes, is_ratio=True, want_lw=True, what="log_ratios")
    return lw, pointwise[0]


def relative_eff(lps):
    """lps [M, S, N] (CUDA) -> r_eff [N] fp64 = ``diagnostics.ess(exp(lps), split=False) / (M S)``: the efficiency of
    the draws for the likelihood of each observation, relative to independent ones.  It inherits ``diagnostics.ess``'
    limits (4 <= S <= 512, M <= 64) and its NaN for a constant or non-finite column.  The observations are walked in
    chunks, so the exp table is never whole."""
    if not isinstance(lps, torch.Tensor) or lps.dim() != 3:
        raise ValueError("lps must be a [chains, draws, observations] tensor")
    M, S = diagnostics._check(lps, False)[:2]
    N = lps.shape[2]
    out = torch.empty(N, dtype=torch.float64, device=lps.device)
    step = max(1, EFF_CHUNK_BYTES // (8 * M * S))
    for a in range(0, N, step):
        out[a:a + step] = diagnostics.ess(lps[:, :, a:a + step].exp(), split=False)
    return out.div_(M * S)


def _loo_result(pointwise, totals, E):
    t = dict(zip(TOTALS, totals))
    return LooResult(t["elpd_loo"], t["se_loo"], t["p_loo"], t["lppd"], pointwise[1], pointwise[0], k_threshold(E),
                     int(t["n_bad"]), t["k_max"])


def _waic_result(pointwise, totals):
    t = dict(zip(TOTALS, totals))
    return WaicResult(t["elpd_waic"], t["se_waic"], t["p_waic"], pointwise[5])


def loo_waic(lps, r_eff=None, workspace_bytes=256 << 20):
    "lps, r_eff as for ``loo`` -> (LooResult, WaicResult) from one pass over the table (``evaluation.evaluate_loo``)"
    pointwise, totals, _ = _run(lps, r_eff, workspace_bytes)
    totals = totals.cpu().tolist()
    return _loo_result(pointwise, totals, math.prod(lps.shape[:-1])), _waic_result(pointwise, totals)


def loo(lps, r_eff=None, workspace_bytes=256 << 20):
    """lps [E, N] or [M, S, N] (CUDA, fp32 or fp64): log p(y_i | theta_s) -> ``LooResult``: ``elpd_loo`` (the sum of the
    pointwise PSIS-LOO log predictive densities), its standard error ``se`` = sqrt(N var_i), ``p_loo``, ``lppd``
    (floats); ``pointwise [N]`` and ``pareto_k [N]`` (device tensors); ``k_threshold`` = min(1 - 1 / log10(E), 0.7),
    ``n_bad`` (how many khat exceed it: their observations' estimates are not to be trusted) and ``k_max``."""
    return loo_waic(lps, r_eff, workspace_bytes)[0]


def waic(lps, workspace_bytes=256 << 20):
    """lps as for ``loo`` -> ``WaicResult(elpd_waic, se, p_waic, pointwise [N])``: lppd minus the sample variance of the
    log-likelihood over the draws, per observation and in total."""
    return loo_waic(lps, None, workspace_bytes)[1]


def compare(results):
    """{name: LooResult | WaicResult} -> ``CompareRow(name, elpd, se, elpd_diff, dse)`` per model, best elpd first:
    ``elpd_diff`` to the best model (<= 0) and ``dse`` = sqrt(N var_i(pointwise - pointwise_best, ddof=1)), the
    standard error of that paired difference (0 for the best).  All results must be of one kind and of one N."""
    if not isinstance(results, dict) or not results:
        raise ValueError("results must be a non-empty dict of LooResult or WaicResult")
    kinds = {type(r) for r in results.values()}
    if len(kinds) != 1 or not kinds <= {LooResult, WaicResult}:
        raise ValueError("results must all be LooResult or all be WaicResult")
    sizes = {tuple(r.pointwise.shape) for r in results.values()}
    if len(sizes) != 1 or len(next(iter(sizes))) != 1:
        raise ValueError(f"the models differ in their observations: {sorted(sizes)}")
    N = next(iter(sizes))[0]
    elpd = {name: r[0] for name, r in results.items()}
    names = sorted(results, key=lambda n: -elpd[n] if not math.isnan(elpd[n]) else math.inf)
    best = results[names[0]].pointwise
    dse = torch.stack([(results[n].pointwise.to(best.device) - best).var(unbiased=True).mul(N).sqrt() if N > 1
                       else torch.full((), math.nan, dtype=best.dtype, device=best.device) for n in names])
    dse = dse.cpu().tolist()
    return [CompareRow(n, elpd[n], results[n].se, elpd[n] - elpd[names[0]], 0.0 if i == 0 else dse[i])
            for i, n in enumerate(names)]


# ---- model averaging -------------------------------------------------------------------------------------------------

MAX_MODELS, SLICE, STATE = _hip.WEIGHTS_MAX_MODELS, _hip.WEIGHTS_SLICE, _hip.WEIGHTS_STATE
S_ITER, S_CONVERGED, S_FROZEN, S_GAP, S_LPD, S_W, S_R = 0, 1, 2, 3, 4, 8, 8 + MAX_MODELS    # of the state record
CACHE_Q = True                       # stacking: q = exp(P - m) formed once into the workspace (measured)
BOOT_WORKSPACE_BYTES = 256 << 20     # bootstrap: the partial sums of one launch's replicates
METHODS = ("stacking", "pseudo-bma", "bb-pseudo-bma")

StackingResult = collections.namedtuple("StackingResult", "weights gap iterations converged lpd")
BootstrapResult = collections.namedtuple("BootstrapResult", "weights se z w", defaults=(None, None))


def weights_workspace_bytes(K, N, replicates=0, cache_q=False):
    "``sgmcmc_weights_workspace_bytes``: the stacking / mixture / pseudo-BMA need or that of ``replicates`` at once"
    if not (1 <= K <= MAX_MODELS and N >= 1 and replicates >= 0):
        return -1
    slices = -(-N // SLICE)
    nbytes = max(8 * (slices * (K + 1) + ((K + 1) * N if cache_q else 0)), replicates * 8 * slices * (K + 1))
    return nbytes if nbytes < 1 << 63 else -1


def _check_table(P, what="P"):
    "-> (P, K, N) for a [K, N] fp64 tensor within the limits; ValueError otherwise.  ``_place`` checks the device"
    if not isinstance(P, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if P.dtype != torch.float64:
        raise ValueError(f"{what} must be float64, not {P.dtype}")
    if P.dim() != 2:
        raise ValueError(f"{what} must be [models, observations]")
    K, N = P.shape
    if not 1 <= K <= MAX_MODELS:
        raise ValueError(f"{K} models: between 1 and {MAX_MODELS} are supported")
    if N < 1:
        raise ValueError(f"{what} needs at least one observation")
    return P, K, N


def _place(P, what="P"):
    """the last check, after every other argument's: P is on the device; -> P with unit observation stride and model
    stride >= N, as a view where possible"""
    if not P.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor")
    K, N = P.shape
    if P.stride(1) != 1 and N > 1 or P.stride(0) < N and K > 1:
        return P.contiguous()
    # a dimension of size 1 has no stride to speak of (torch keeps whatever the view had): give it the plain one
    return P.as_strided((K, N), (P.stride(0) if K > 1 else N, 1))


def _int(v, name, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}], not {v!r}")
    return v


def _workspace(nbytes, dev):
    return torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=dev)


def stacking_state(P, tol=1e-8, max_iter=100_000, check_every=64, cache_q=None):
    """The stacking run of ``stacking_weights`` -> its state record [72] on the host (fp64: updates applied, converged,
    frozen, gap, lpd, tol, max_iter, -, w [32], r [32]) and on the device."""
    P, K, N = _check_table(P)
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not 0.0 <= tol < math.inf:
        raise ValueError(f"tol must be a finite number >= 0, not {tol!r}")
    _int(max_iter, "max_iter", 0, 1 << 52)
    _int(check_every, "check_every", 1, 1 << 20)
    cache_q = int(CACHE_Q if cache_q is None else bool(cache_q))
    P = _place(P)
    dev = P.device
    work = _workspace(weights_workspace_bytes(K, N, 0, cache_q), dev)
    state = torch.empty(STATE, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        L = _hip.lib()
        _hip.check(L.sgmcmc_stacking_init(P.data_ptr(), P.stride(0), K, N, float(tol), max_iter, cache_q,
                                          work.data_ptr(), work.numel() * 8, state.data_ptr(), stream),
                   "sgmcmc_stacking_init")
        while True:
            _hip.check(L.sgmcmc_stacking_iterate(P.data_ptr(), P.stride(0), K, N, cache_q, check_every,
                                                 work.data_ptr(), work.numel() * 8, state.data_ptr(), stream),
                       "sgmcmc_stacking_iterate")
            host = state.cpu()
            if host[S_FROZEN] != 0.0:
                return host, state


def stacking_weights(P, tol=1e-8, max_iter=100_000, check_every=64):
    """P [K, N] (CUDA, fp64; model stride >= N is read in place): pointwise elpd of K <= 32 models -> ``StackingResult``:
    the ``weights [K]`` (device) that maximise f(w) = (1/N) sum_i log sum_k w_k exp(P[k, i]) over the simplex, by the EM
    update of mixture proportions from w = 1/K; ``gap`` = max_k r_k - 1 at the returned w, a certificate:
    f(w*) - f(w) <= gap; ``iterations`` (updates applied); ``converged`` (gap <= tol before ``max_iter`` updates); ``lpd``
    = N f(w).  Batches of ``check_every`` iterations are enqueued and the state record is read once per batch; the result
    does not depend on ``check_every``.  A non-finite entry of P gives NaN everywhere."""
    host, state = stacking_state(P, tol, max_iter, check_every)
    return StackingResult(state[S_W:S_W + P.shape[0]].clone(), host[S_GAP].item(), int(host[S_ITER].item()),
                          bool(host[S_CONVERGED].item()), host[S_LPD].item())


def pseudo_bma_weights(P):
    "P as for ``stacking_weights`` -> weights [K] (device) = softmax_k(sum_i P[k, i]); NaN if P has a non-finite entry"
    P, K, N = _check_table(P)
    P = _place(P)
    dev = P.device
    work = _workspace(weights_workspace_bytes(K, N), dev)
    out = torch.empty((2, K), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().sgmcmc_pseudo_bma(P.data_ptr(), P.stride(0), K, N, work.data_ptr(), work.numel() * 8,
                                                out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "sgmcmc_pseudo_bma")
    return out[0]


def bb_pseudo_bma_weights(P, B=1000, seed=0, stream=0, replicates=False):
    """P as for ``stacking_weights`` -> ``BootstrapResult(weights [K], se [K])`` (device): pseudo-BMA+ -- for each of B
    Bayesian-bootstrap replicates b, z_{b,k} = N sum_i g_i P[k, i] / sum_i g_i with g = -log u, u the Philox uniforms of
    (seed, stream, draw b, purpose 4), and w_b = softmax(z_b); ``weights`` = mean_b w_b, ``se`` = sqrt(var_b z, ddof 1).
    ``replicates=True`` adds the tables ``z`` and ``w`` [B, K].  Replicate b depends on (seed, stream, b) only."""
    P, K, N = _check_table(P)
    _int(B, "B", 1, 1 << 31)
    _int(seed, "seed", 0, (1 << 64) - 1)
    _int(stream, "stream", 0, 0xFFF)
    P = _place(P)
    dev = P.device
    per = weights_workspace_bytes(K, N, 1)
    work = _workspace(per * max(1, min(B, BOOT_WORKSPACE_BYTES // per)), dev)
    z = torch.empty((B, K), dtype=torch.float64, device=dev)
    w = torch.empty((B, K), dtype=torch.float64, device=dev)
    out = torch.empty((2, K), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().sgmcmc_bb_pseudo_bma(P.data_ptr(), P.stride(0), K, N, B, seed, stream, work.data_ptr(),
                                                   work.numel() * 8, z.data_ptr(), w.data_ptr(), out.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream), "sgmcmc_bb_pseudo_bma")
    return BootstrapResult(out[0], out[1], z, w) if replicates else BootstrapResult(out[0], out[1])


def mixture_lpd(P, weights):
    """P [K, N] as for ``stacking_weights`` (any pointwise log densities, e.g. the test rows' lppd of each model),
    ``weights`` [K] (a tensor or a sequence of floats) -> (sum_i log sum_k w_k exp(P[k, i]) as a float, pointwise [N] on
    the device).  An observation with a non-finite entry gives NaN there and in the total."""
    P, K, N = _check_table(P)
    if not isinstance(weights, torch.Tensor):
        try:
            weights = torch.tensor([float(v) for v in weights], dtype=torch.float64)
        except (TypeError, ValueError):
            raise ValueError("weights must be a tensor or a sequence of floats") from None
    if weights.dtype != torch.float64 or tuple(weights.shape) != (K,):
        raise ValueError(f"weights must be float64 of shape [{K}]")
    P = _place(P)
    dev = P.device
    weights = weights.to(dev).contiguous()
    work = _workspace(weights_workspace_bytes(K, N), dev)
    pointwise = torch.empty(N, dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().sgmcmc_mixture_lpd(P.data_ptr(), P.stride(0), K, N, weights.data_ptr(), work.data_ptr(),
                                                 work.numel() * 8, pointwise.data_ptr(), total.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "sgmcmc_mixture_lpd")
    return total.item(), pointwise


def pointwise_matrix(results):
    """{name: LooResult | WaicResult} -> (names, P [K, N] fp64): the models' pointwise rows, in ``compare``'s order (best
    elpd first).  As for ``compare`` the results must be of one kind and one N; here also on one device."""
    if not isinstance(results, dict) or not results:
        raise ValueError("results must be a non-empty dict of LooResult or WaicResult")
    kinds = {type(r) for r in results.values()}
    if len(kinds) != 1 or not kinds <= {LooResult, WaicResult}:
        raise ValueError("results must all be LooResult or all be WaicResult")
    sizes = {tuple(r.pointwise.shape) for r in results.values()}
    if len(sizes) != 1 or len(next(iter(sizes))) != 1:
        raise ValueError(f"the models differ in their observations: {sorted(sizes)}")
    if len({r.pointwise.device for r in results.values()}) != 1:
        raise ValueError("the models' pointwise rows must be on one device")
    if len(results) > MAX_MODELS:
        raise ValueError(f"{len(results)} models: at most {MAX_MODELS} are supported")
    elpd = {name: r[0] for name, r in results.items()}
    names = sorted(results, key=lambda n: -elpd[n] if not math.isnan(elpd[n]) else math.inf)
    return names, torch.stack([results[n].pointwise.to(torch.float64) for n in names])


def model_weights(results, method="stacking", **kw):
    """{name: LooResult | WaicResult} -> {name: weight} (floats, in ``compare``'s order) by ``method``: "stacking"
    (``stacking_weights``), "pseudo-bma" or "bb-pseudo-bma" (``bb_pseudo_bma_weights``); ``kw`` goes to that function.
    The weights cross to the host in one copy (stacking reads its state record once per batch before that)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    names, P = pointwise_matrix(results)
    if method == "stacking":
        w = stacking_weights(P, **kw).weights
    elif method == "pseudo-bma":
        w = pseudo_bma_weights(P, **kw)
    else:
        w = bb_pseudo_bma_weights(P, **kw).weights
    return dict(zip(names, w.cpu().tolist()))
