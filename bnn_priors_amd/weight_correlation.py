"""Are the weights of a layer correlated -- between which units, and compared with what null?  The correlation half of the
study of trained weights, on the device (``csrc/corr_hip.inc``; C ABI ``sgmcmc_corr_*``, definitions in
``include/sgmcmc_hip.h``), for the stacks ``[S, *shape]`` that ``storage.load_samples`` returns:

    covariance          mean, covariance and correlation between the V indices of one axis (the rows or the columns of a
                        dense layer, the output or input channels of a convolution), every other axis -- S included --
                        indexing the n observations; V up to 1,024 (``prior_fit.moments`` stops at 25 positions)
    offdiag_stats       the off-diagonal summary of a correlation matrix: mean r, mean |r|, rms r, max |r| and its pair,
                        sum r^2
    independence_test   a permutation test of "the variables are mutually independent" on rms r and max |r|, with the
                        closed-form Gaussian references (the expected rms 1 / sqrt(n - 1), Schott's z for sum r^2)
    layer_correlations  all of it for every tensor of a dict of samples, on axes 0 and 1

A stack is read in place through its strides (fp32 or fp64, any view).  The centred Gram matrix runs in fp64 on the matrix
pipe (``v_mfma_f64_16x16x4_f64``); every sum runs in an order fixed by (V, n) and ``workspace_bytes`` -- not by the strides
-- so two calls, or a view and its contiguous copy, give the same bits.  No floating-point atomics.  ``covariance`` and
``offdiag_stats`` do not synchronise with the host.  CPU tensors are refused: there is no CPU path.
"""
import collections
import math

import torch

from . import _gram_pass, _hip
from .calibration import _stream
from .prior_fit import _collapse

__all__ = ("Correlation", "OffDiag", "IndependenceTest", "LayerCorrelations", "covariance", "offdiag_stats",
           "independence_test", "layer_correlations", "schott", "splits", "mean_blocks", "TILE", "CHUNK", "MAX_V",
           "MAX_SPLITS", "MAX_N", "MAX_OBS_DIMS", "WORKSPACE_BYTES")

TILE = _hip.CORR_TILE                    # G is formed in TILE x TILE blocks (SGMCMC_CORR_TILE)
CHUNK = _hip.CORR_CHUNK                  # observations of one staged chunk, "KC" (SGMCMC_CORR_CHUNK)
MAX_V = _hip.CORR_MAX_V
MAX_SPLITS = _hip.CORR_MAX_SPLITS
MAX_N = 2 ** 31 - 1
MAX_OBS_DIMS = 4
WORKSPACE_BYTES = 256 << 20

Correlation = collections.namedtuple("Correlation", "n mean cov corr zero_variance nonfinite")
Correlation.__doc__ = ("n: the number of observations (int); on the device: mean [V], cov [V, V] (divided by n - ddof), "
                       "corr [V, V] in fp64; zero_variance [V] (bool): variables whose cov row is 0 and whose corr row "
                       "and column are NaN; nonfinite (0-d int64): the NaN / Inf elements, which make mean, cov and "
                       "corr NaN")
OffDiag = collections.namedtuple("OffDiag", "pairs mean mean_abs rms max_abs argmax sum_sq")
OffDiag.__doc__ = ("over the pairs i < j of variables with variance, per matrix (device tensors of length R): pairs "
                   "(int64), mean r, mean |r|, rms r, max |r| (fp64), argmax [R, 2] (int64: its pair, the smallest in "
                   "row-major order on a tie, (-1, -1) without a pair), sum_sq = sum r^2; NaN without a pair")
IndependenceTest = collections.namedtuple("IndependenceTest", "n V observed null p_rms p_max expected_rms schott_mean "
                                                              "schott_var schott_z")
IndependenceTest.__doc__ = ("n, V: ints; observed: the ``OffDiag`` of the data (R = 1); null [B, 2]: (rms r, max |r|) of "
                            "every permuted replicate; p_rms, p_max = (1 + #{null_b >= observed}) / (B + 1); "
                            "expected_rms = 1 / sqrt(n - 1) (float); schott_mean, schott_var, schott_z: the moments of "
                            "sum r^2 under independent Gaussian variables and its standard score (0-d fp64 tensors)")
LayerCorrelations = collections.namedtuple("LayerCorrelations", "layers skipped")
LayerCorrelations.__doc__ = ("layers: {(name, axis): IndependenceTest}; skipped: [(name, axis, reason)] of the axes "
                             "that were left out")


def splits(V, n, workspace_bytes=WORKSPACE_BYTES):
    """Workgroups that share the chunks of one block pair of the Gram pass (``corr::splits``): workgroup b walks chunks
    b, b + splits, ...  A function of (V, n, workspace_bytes) alone; 0 if the workspace holds no V x V doubles."""
    return _gram_pass.splits(V, n, workspace_bytes, TILE, CHUNK, MAX_SPLITS, _hip.CORR_TARGET_BLOCKS)


def mean_blocks(V, n):
    "workgroups that share the chunks of one variable tile in the mean pass (``corr::mean_blocks``)"
    return min(-(-n // CHUNK), _hip.CORR_MEAN_BLOCKS // -(-V // TILE))


def _geometry(w, var_dim):
    "sgmcmc_corr_geometry of the stack w [S, *shape] with the variables on axis var_dim of shape; every limit is checked here"
    if not isinstance(w, torch.Tensor) or w.dim() < 2 or w.dtype not in (torch.float32, torch.float64):
        raise ValueError("w must be a float32 or float64 [S, *shape] tensor")
    if w.numel() == 0:
        raise ValueError("w is empty")
    nd = w.dim() - 1
    if isinstance(var_dim, bool) or not isinstance(var_dim, int) or not -nd <= var_dim < nd:
        raise ValueError(f"var_dim = {var_dim!r}: an axis of the shape {tuple(w.shape[1:])}, in [{-nd}, {nd}), is needed")
    axis = 1 + var_dim % nd
    V = w.shape[axis]
    if not 1 <= V <= MAX_V:
        raise ValueError(f"V = {V} variables: 1 .. {MAX_V} are supported")
    n = w.numel() // V
    if not 2 <= n <= MAX_N:
        raise ValueError(f"n = {n} observations: 2 .. {MAX_N} are supported")
    obs = _collapse([(w.shape[a], w.stride(a)) for a in range(w.dim()) if a != axis])
    if len(obs) > MAX_OBS_DIMS:
        raise ValueError(f"the observations span {len(obs)} strided dimensions: at most {MAX_OBS_DIMS} are supported")
    g = _hip.CorrGeometry()
    g.V, g.n, g.v_stride = V, n, w.stride(axis)
    g.v_major = int(V > 1 and g.v_stride < obs[-1][1])
    for k, (size, stride) in enumerate([(1, 0)] * (MAX_OBS_DIMS - len(obs)) + obs):
        g.size[k], g.stride[k] = size, stride
    return g


def _contiguous_geometry(V, n):
    "the geometry of one [V, n] matrix of a contiguous batch [R, V, n]"
    g = _hip.CorrGeometry()
    g.V, g.n, g.v_stride, g.v_major = V, n, n, 0
    for k in range(MAX_OBS_DIMS):
        g.size[k], g.stride[k] = (n, 1) if k == MAX_OBS_DIMS - 1 else (1, 0)
    return g


def _check_common(g, ddof, workspace_bytes):
    if isinstance(ddof, bool) or not isinstance(ddof, int) or not 0 <= ddof < g.n:
        raise ValueError(f"ddof = {ddof!r}: 0 .. n - 1 = {g.n - 1} is supported")
    _gram_pass.check_workspace_bytes(workspace_bytes)
    sp = splits(g.V, g.n, workspace_bytes)
    if sp < 1:
        raise ValueError(f"workspace_bytes = {workspace_bytes} holds no {g.V} x {g.V} matrix of doubles "
                         f"({8 * g.V * g.V} bytes)")
    return sp


def _on_device(w):
    if not w.is_cuda:
        raise ValueError("w must be a CUDA tensor (there is no CPU path)")
    return w.device


def _dtype(w):
    return _hip.F32 if w.dtype == torch.float32 else _hip.F64


def _mean(w, g):
    "-> (mean [V], nonfinite [1]) of the stack behind g"
    dev, lib = w.device, _hip.lib()
    segs, nb = mean_blocks(g.V, g.n), -(-g.V // TILE)
    assert segs == lib.sgmcmc_corr_mean_blocks(g.V, g.n)
    part = torch.empty(segs * g.V, dtype=torch.float64, device=dev)
    counts = torch.empty(segs * nb, dtype=torch.int64, device=dev)
    mean = torch.empty(g.V, dtype=torch.float64, device=dev)
    bad = torch.empty(1, dtype=torch.int64, device=dev)
    _hip.check(lib.sgmcmc_corr_mean(w.data_ptr(), _dtype(w), g, part.data_ptr(), counts.data_ptr(), mean.data_ptr(),
                                    bad.data_ptr(), _stream()), "sgmcmc_corr_mean")
    return mean, bad


def _gram(x, g, R, batch_stride, mean, bad, sp, ddof, want_cov):
    "-> (cov [R, V, V] or None, corr [R, V, V], zero_variance [R, V]) of the R matrices at x"
    dev, lib, V = x.device, _hip.lib(), g.V
    slabs = torch.empty(sp * R * V * V, dtype=torch.float64, device=dev)
    cov = torch.empty((R, V, V), dtype=torch.float64, device=dev) if want_cov else None
    corr = torch.empty((R, V, V), dtype=torch.float64, device=dev)
    zero = torch.empty((R, V), dtype=torch.uint8, device=dev)
    _hip.check(lib.sgmcmc_corr_gram(x.data_ptr(), _dtype(x), g, R, batch_stride, mean.data_ptr(), sp, slabs.data_ptr(),
                                    _stream()), "sgmcmc_corr_gram")
    _hip.check(lib.sgmcmc_corr_finish(slabs.data_ptr(), sp, R, V, g.n, ddof, bad.data_ptr(),
                                      None if cov is None else cov.data_ptr(), corr.data_ptr(), zero.data_ptr(),
                                      _stream()), "sgmcmc_corr_finish")
    return cov, corr, zero.to(torch.bool)


def covariance(w, var_dim, ddof=1, workspace_bytes=WORKSPACE_BYTES):
    """w [S, *shape] -> ``Correlation`` between the V indices of axis ``var_dim`` of ``shape``; every other axis, S
    included, indexes the n = S numel(shape) / V observations.  Two passes: the means (compensated sums about each
    variable's first observation), then G = d d^T of d = x - mean in 64 x 64 blocks on the fp64 matrix pipe; cov = G /
    (n - ddof), corr_ij = G_ij / sqrt(G_ii G_jj).  The partial Gram slabs take ``splits(V, n, workspace_bytes)`` V^2
    doubles.  A variable without variance is flagged, its cov row 0 and its corr row and column NaN (the policy of
    ``prior_fit.moments``); a NaN or Inf anywhere makes every floating output NaN.  No host synchronisation."""
    g = _geometry(w, var_dim)
    sp = _check_common(g, ddof, workspace_bytes)
    dev = _on_device(w)
    assert sp == _hip.lib().sgmcmc_corr_splits(g.V, g.n, workspace_bytes)
    with torch.cuda.device(dev):
        mean, bad = _mean(w, g)
        cov, corr, zero = _gram(w, g, 1, 0, mean, bad, sp, ddof, True)
    return Correlation(g.n, mean, cov[0], corr[0], zero[0], bad[0])


def offdiag_stats(corr):
    """corr: ``[V, V]`` or ``[R, V, V]`` fp64 device tensor -> ``OffDiag`` of each matrix, over the pairs i < j of the
    variables whose diagonal entry is not NaN (``covariance`` writes NaN there for a variable without variance).
    Deterministic; no host synchronisation."""
    if not isinstance(corr, torch.Tensor) or corr.dtype != torch.float64 or corr.dim() not in (2, 3) \
            or corr.shape[-1] != corr.shape[-2]:
        raise ValueError("corr must be a float64 [V, V] or [R, V, V] tensor")
    V = corr.shape[-1]
    R = corr.shape[0] if corr.dim() == 3 else 1
    if not 1 <= V <= MAX_V:
        raise ValueError(f"V = {V} variables: 1 .. {MAX_V} are supported")
    if R < 1:
        raise ValueError("corr holds no matrix")
    if not corr.is_cuda:
        raise ValueError("corr must be a CUDA tensor (there is no CPU path)")
    corr = corr.contiguous()
    with torch.cuda.device(corr.device):
        stats = torch.empty((R, _hip.CORR_STATS), dtype=torch.float64, device=corr.device)
        counts = torch.empty((R, 3), dtype=torch.int64, device=corr.device)
        _hip.check(_hip.lib().sgmcmc_corr_offdiag(corr.data_ptr(), R, V, stats.data_ptr(), counts.data_ptr(), _stream()),
                   "sgmcmc_corr_offdiag")
    return OffDiag(counts[:, 0], stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], counts[:, 1:], stats[:, 4])


def schott(sum_sq, pairs, n):
    """(mean, variance, z) of sum_{i<j} r^2 under independent Gaussian variables (Schott 2005): with nu = n - 1 and
    ``pairs`` = V (V - 1) / 2, every r^2 ~ Beta(1/2, (n - 2) / 2) and the pairs are uncorrelated, so the mean is pairs / nu
    = V (V - 1) / (2 nu) and the variance 2 pairs (nu - 1) / (nu^2 (nu + 2)) = V (V - 1) (nu - 1) / (nu^2 (nu + 2)).
    Numbers or tensors."""
    nu = n - 1
    mean = pairs / nu
    var = 2 * pairs * (nu - 1) / (nu * nu * (nu + 2))
    return mean, var, (sum_sq - mean) / var ** 0.5


def _batch_replicates(V, n, sp, itemsize, B, workspace_bytes):
    "replicates of one launch: their slabs, permutation tables, keys and gathered copies fit workspace_bytes"
    per = 8 * sp * V * V + V * n * (8 + 4 + itemsize)
    return max(1, min(B, _hip.CORR_MAX_BATCH, workspace_bytes // per))


def independence_test(w, var_dim, replicates=199, seed=0, perms=None, workspace_bytes=WORKSPACE_BYTES):
    """Permutation test of "the V variables of axis ``var_dim`` are mutually independent, and each variable's observations
    are exchangeable" -> ``IndependenceTest``.  Each replicate permutes every variable's n observations independently
    (which changes neither a mean nor a variance) and recomputes the off-diagonal statistics of its correlation matrix.

    The stack is materialised once as a contiguous [V, n]; R permutation tables at a time are drawn as
    ``torch.argsort(torch.rand(R, V, n, generator=g), dim=-1, stable=True)`` on a device generator seeded with ``seed``,
    ``torch.gather`` makes [R, V, n], and the Gram kernel runs with the batch R riding in its grid and the means of the
    data; R is what ``workspace_bytes`` holds of slabs, tables, keys and copies.  ``perms`` gives the tables instead: int64
    [B, V, n] on the device, every row a permutation of 0 .. n - 1 (``replicates`` and ``seed`` are then unused).  The
    result is a function of (w, seed, replicates, workspace_bytes), or of (w, perms, workspace_bytes)."""
    g = _geometry(w, var_dim)
    sp = _check_common(g, 1, workspace_bytes)
    V, n = g.V, g.n
    if perms is None:
        if isinstance(replicates, bool) or not isinstance(replicates, int) or not 1 <= replicates <= 2 ** 24:
            raise ValueError(f"replicates = {replicates!r}: 1 .. 2^24 are supported")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed = {seed!r} must be an integer")
        B = replicates
    else:
        if not isinstance(perms, torch.Tensor) or perms.dtype != torch.int64 or perms.dim() != 3 \
                or tuple(perms.shape[1:]) != (V, n) or perms.shape[0] < 1:
            raise ValueError(f"perms must be an int64 [B, V = {V}, n = {n}] tensor with B >= 1")
        if not perms.is_cuda:
            raise ValueError("perms must be a CUDA tensor (there is no CPU path)")
        B = perms.shape[0]
    dev = _on_device(w)
    axis = 1 + var_dim % (w.dim() - 1)
    with torch.cuda.device(dev):
        mean, bad = _mean(w, g)
        _, corr, _ = _gram(w, g, 1, 0, mean, bad, sp, 1, False)
        observed = offdiag_stats(corr)
        x = w.movedim(axis, 0).reshape(V, n).contiguous()
        gc = _contiguous_geometry(V, n)
        R = _batch_replicates(V, n, sp, x.element_size(), B, workspace_bytes)
        gen = None
        if perms is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(seed)
        null = torch.empty((B, 2), dtype=torch.float64, device=dev)
        for b in range(0, B, R):
            r = min(R, B - b)
            table = (torch.argsort(torch.rand((r, V, n), generator=gen, device=dev), dim=-1, stable=True)
                     if perms is None else perms[b:b + r])
            xp = torch.gather(x.unsqueeze(0).expand(r, V, n), 2, table)
            _, cr, _ = _gram(xp, gc, r, V * n, mean, bad, sp, 1, False)
            od = offdiag_stats(cr)
            null[b:b + r, 0], null[b:b + r, 1] = od.rms, od.max_abs
        p_rms = (1 + (null[:, 0] >= observed.rms[0]).sum()).to(torch.float64) / (B + 1)
        p_max = (1 + (null[:, 1] >= observed.max_abs[0]).sum()).to(torch.float64) / (B + 1)
        s_mean, s_var, z = schott(observed.sum_sq[0], observed.pairs[0].to(torch.float64), n)
    return IndependenceTest(n, V, observed, null, p_rms, p_max, 1.0 / math.sqrt(n - 1), s_mean, s_var, z)


def layer_correlations(samples, chains=None, **kw):
    """samples: the dict of ``storage.load_samples`` ({name: [S, *shape]}), or a list of such dicts, one per chain, whose
    samples are pooled; ``chains``: the number of equally long chains a single dict holds (checked, as
    ``diagnostics.weight_space`` does; the test pools them) -> ``LayerCorrelations``: for every floating-point tensor with
    at least two non-sample axes, ``independence_test(stack, axis, **kw)`` on axes 0 and 1 of its shape (the rows and
    columns of a dense layer, the output and input channels of a convolution) under the key (name, axis).  The
    book-keeping entries that ``diagnostics`` skips are skipped; an axis with V > 1,024 or V = 1 is named in ``skipped``.
    Host tensors are moved to the current device, other floating types converted to float32."""
    from .diagnostics import _diagnosable
    if isinstance(samples, dict):
        stacks = {k: v for k, v in samples.items() if _diagnosable(k, v)}
        if chains is not None:
            if isinstance(chains, bool) or not isinstance(chains, int) or chains < 1:
                raise ValueError(f"chains = {chains!r} must be a positive integer")
            for k, v in stacks.items():
                if v.dim() < 1 or v.shape[0] % chains:
                    raise ValueError(f"{k}: {tuple(v.shape)} does not hold {chains} chains of equal length")
    else:
        samples = list(samples)
        if not samples or not all(isinstance(s, dict) for s in samples):
            raise ValueError("samples must be a dict or a non-empty list of dicts")
        if chains is not None and int(chains) != len(samples):
            raise ValueError(f"chains={chains} but {len(samples)} sample dicts were given")
        stacks = {k: torch.cat([s[k] for s in samples]) for k, v in samples[0].items() if _diagnosable(k, v)}
    layers, skipped = {}, []
    for name, v in stacks.items():
        if v.dim() < 3:
            continue
        if v.dtype not in (torch.float32, torch.float64):
            v = v.to(torch.float32)
        if not v.is_cuda:
            v = v.to("cuda")
        for axis in (0, 1):
            V = v.shape[1 + axis]
            if V == 1 or V > MAX_V:
                skipped.append((name, axis, f"V = {V}: 2 .. {MAX_V} variables are analysed"))
                continue
            layers[(name, axis)] = independence_test(v, axis, **kw)
    return LayerCorrelations(layers, skipped)
