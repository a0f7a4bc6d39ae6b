"""Do the draws target the right distribution?  The kernel Stein discrepancy (KSD) with the inverse multiquadric kernel
(Gorham & Mackey 2017), its wild-bootstrap goodness-of-fit test (Chwialkowski, Strathmann & Gretton 2016) and Stein
thinning (Riabiz et al. 2022), on the device (``csrc/stein_hip.inc``; C ABI ``sgmcmc_stein_*``, definitions in
``include/sgmcmc_hip.h``).  All of it needs the draws and the gradient of the log target at each draw only:

    scores               {name: [S, *shape]}: the gradient of -potential / temperature at every stored sample (autograd)
    kernel_matrix        the Stein matrix K [S, S] and the squared distances r2 from samples and scores
    ksd                  v_stat = sum K / S^2, u_stat (without the diagonal), ksd = sqrt(v_stat), the row means of K
    quadratic_forms      Q_r = W_r^T K W_r / S^2 for a batch of weight vectors
    wild_bootstrap_test  the null of v_stat under sign flips, and its p-value
    thin                 the m samples that Stein thinning keeps, and the KSD of every prefix

R-hat and ESS say whether chains agree and the temperature diagnostics what the momenta do; none of them sees a bias that
all chains share (step size, minibatch noise without a Metropolis-Hastings test).  The KSD does.  It loses power as the
dimension grows: it is for comparing runs of the same model, for thinning, and for the small targets.

The Gram matrix of the 2S rows [X - x_0; G] runs in fp64 on the matrix pipe (``v_mfma_f64_16x16x4_f64``); every sum runs in
an order fixed by (S, D) and ``workspace_bytes`` -- not by the strides -- so two calls, a view and its contiguous copy, or a
batch of weight vectors and its single calls give the same bits.  No floating-point atomics.  ``kernel_matrix``, ``ksd``,
``quadratic_forms`` and ``thin`` do not synchronise with the host.  CPU tensors are refused (``scores`` is plain torch).
"""
import collections
import math

import torch

from . import _gram_pass, _hip
from .calibration import _stream

__all__ = ("SteinKernel", "KSD", "SteinTest", "Thinning", "scores", "kernel_matrix", "ksd", "quadratic_forms",
           "wild_bootstrap_test", "thin", "splits", "TILE", "CHUNK", "MAX_S", "MAX_SPLITS", "MAX_D", "MAX_PICKS",
           "MAX_BATCH", "WORKSPACE_BYTES")

TILE = _hip.STEIN_TILE                   # the Gram matrix is formed in TILE x TILE blocks (SGMCMC_STEIN_TILE)
CHUNK = _hip.STEIN_CHUNK                 # coordinates of one staged chunk, "KC" (SGMCMC_STEIN_CHUNK)
MAX_S = _hip.STEIN_MAX_S
MAX_SPLITS = _hip.STEIN_MAX_SPLITS
MAX_D = 2 ** 31 - 1
MAX_PICKS = _hip.STEIN_MAX_PICKS
MAX_BATCH = _hip.STEIN_MAX_BATCH
WORKSPACE_BYTES = 256 << 20

SteinKernel = collections.namedtuple("SteinKernel", "K r2 c beta d nonfinite")
SteinKernel.__doc__ = ("on the device, fp64: K [S, S] the Stein matrix, r2 [S, S] the squared distances (exactly 0 on the "
                       "diagonal); c (a float, or a 0-d tensor for c = 'median'), beta (float), d (int: the total "
                       "dimension); nonfinite (0-d int64): the NaN / Inf elements of x and score, which make K and r2 NaN")
KSD = collections.namedtuple("KSD", "v_stat u_stat ksd row_mean")
KSD.__doc__ = ("0-d fp64 device tensors v_stat = sum_ij K_ij / S^2, u_stat = sum_{i != j} K_ij / (S (S - 1)), ksd = "
               "sqrt(v_stat); row_mean [S]: sum_j K_ij / S")
SteinTest = collections.namedtuple("SteinTest", "v_stat null p")
SteinTest.__doc__ = ("v_stat (0-d), null [R]: Q_r of every sign vector, p = (1 + #{Q_r >= v_stat}) / (R + 1) (0-d), fp64 "
                     "device tensors")
Thinning = collections.namedtuple("Thinning", "indices ksd_path")
Thinning.__doc__ = ("indices [m] (int64): the kept samples in the order they were picked (picks may repeat); ksd_path [m] "
                    "(fp64): the KSD of the first 1 .. m picks")


def splits(S, D, workspace_bytes=WORKSPACE_BYTES):
    """Workgroups that share the chunks of one block pair of the Gram pass (``stein::splits``): workgroup b walks chunks
    b, b + splits, ...  A function of (S, D, workspace_bytes) alone; 0 if the workspace holds no 2S x 2S doubles."""
    return _gram_pass.splits(2 * S, D, workspace_bytes, TILE, CHUNK, MAX_SPLITS, _hip.STEIN_TARGET_BLOCKS)


# ---------------------------------------------------------------------------------------------------------------- scores

def scores(model, samples, x=None, y=None, temperature=1., batch_size=None):
    """{name: [S, *shape]}: the gradient of ``-model.potential(x, y, eff_num_data=len(x)) / temperature`` -- the score of
    the tempered posterior -- at every one of the S samples, for the model's parameters that occur in ``samples`` (the
    other entries of ``samples``, buffers for instance, are loaded too).  Autograd; the model's train / eval mode and its
    state are left as they were found.  With ``batch_size`` the likelihood gradients of the batches are summed and the
    prior's gradient is added once.  ``x = y = None`` is for a ``PriorOnlyModel``."""
    if not isinstance(samples, dict) or not samples:
        raise ValueError("samples must be a non-empty dict of [S, *shape] stacks")
    if not temperature > 0:
        raise ValueError(f"temperature = {temperature!r} must be positive")
    if (x is None) != (y is None):
        raise ValueError("x and y are given together, or neither")
    if batch_size is not None and (isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1):
        raise ValueError(f"batch_size = {batch_size!r} must be a positive integer")
    params = collections.OrderedDict((n, p) for n, p in model.named_parameters() if n in samples)
    if not params:
        raise ValueError("none of the model's parameters occurs in samples")
    state = model.state_dict()
    missing = sorted(k for k in samples if k not in state)
    if missing:
        raise ValueError(f"samples has entries the model does not: {missing}")
    S = min(len(v) for v in samples.values())
    n = 1 if x is None else len(x)
    kept = {k: v.detach().clone() for k, v in state.items() if k in samples}
    need = [p.requires_grad for p in params.values()]
    out = {k: torch.empty((S, *p.shape), dtype=p.dtype, device=p.device) for k, p in params.items()}
    plist = list(params.values())
    try:
        for p in plist:
            p.requires_grad_(True)
        for s in range(S):
            model.load_state_dict({k: v[s] for k, v in samples.items()}, strict=False)
            if x is None or batch_size is None or batch_size >= n:
                grads = torch.autograd.grad(model.potential(x, y, n), plist, allow_unused=True)
            else:
                grads = torch.autograd.grad(-model.log_prior(), plist, allow_unused=True)
                grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, plist)]
                for b in range(0, n, batch_size):
                    xb, yb = x[b:b + batch_size], y[b:b + batch_size]
                    # log_likelihood scales its batch's sum by eff_num_data / len(batch): eff_num_data = len(batch)
                    # leaves the plain sum, and the sums of the batches add up to the full-data term
                    gb = torch.autograd.grad(-model.log_likelihood(xb, yb, len(xb)), plist, allow_unused=True)
                    grads = [g if q is None else g + q for g, q in zip(grads, gb)]
            for (k, p), g in zip(params.items(), grads):
                out[k][s] = 0 if g is None else -g / temperature
    finally:
        model.load_state_dict(kept, strict=False)
        for p, r in zip(plist, need):
            p.requires_grad_(r)
    return out


# ---------------------------------------------------------------------------------------------------------------- checks

def _as_matrix(t, what):
    "[S, *shape] -> a [S, D] view with unit column stride (a copy only where no view exists)"
    if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be a float32 or float64 [S, *shape] tensor")
    if t.numel() == 0:
        raise ValueError(f"{what} is empty")
    if t.dim() == 2:
        m = t
    else:
        S = t.shape[0]
        try:
            m = t.view(S, -1)
        except RuntimeError:
            m = t.reshape(S, -1)
    if m.shape[1] > 1 and m.stride(1) != 1 or m.stride(0) < 0:
        m = m.contiguous()
    return m


def _pairs(x, score):
    "-> [(x [S, D_t], score [S, D_t])] in key order, every limit checked"
    if isinstance(x, dict) != isinstance(score, dict):
        raise ValueError("x and score must both be tensors or both be dicts")
    if isinstance(x, dict):
        if not x or sorted(x) != sorted(score):
            raise ValueError(f"x and score must be non-empty dicts with the same keys: {sorted(x)} / {sorted(score)}")
        names = sorted(x)
        pairs = [(_as_matrix(x[k], f"x[{k!r}]"), _as_matrix(score[k], f"score[{k!r}]")) for k in names]
    else:
        if isinstance(x, torch.Tensor) and x.dim() != 2:
            raise ValueError("x must be a float32 or float64 [S, D] tensor (or a dict of [S, *shape] stacks)")
        names = [None]
        pairs = [(_as_matrix(x, "x"), _as_matrix(score, "score"))]
    S = pairs[0][0].shape[0]
    for name, (a, b) in zip(names, pairs):
        label = "" if name is None else f" [{name!r}]"
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError(f"x and score{label} differ in shape or dtype: {tuple(a.shape)} {a.dtype} / "
                             f"{tuple(b.shape)} {b.dtype}")
        if a.shape[0] != S:
            raise ValueError(f"x{label} holds {a.shape[0]} samples, the first tensor {S}")
        if not 1 <= a.shape[1] <= MAX_D:
            raise ValueError(f"D = {a.shape[1]} coordinates{label}: 1 .. {MAX_D} are supported per tensor")
    if not 2 <= S <= MAX_S:
        raise ValueError(f"S = {S} samples: 2 .. {MAX_S} are supported")
    return pairs


def _check_beta(beta):
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not -1.0 < beta < 0.0:
        raise ValueError(f"beta = {beta!r}: -1 < beta < 0 is needed")
    return float(beta)


def _check_c(c):
    if isinstance(c, str):
        if c != "median":
            raise ValueError(f"c = {c!r}: a positive number or 'median'")
        return None
    if isinstance(c, bool) or not isinstance(c, (int, float)) or not 0.0 < c < math.inf:
        raise ValueError(f"c = {c!r}: a positive number or 'median'")
    return float(c)


def _check_workspace(workspace_bytes, S):
    _gram_pass.check_workspace_bytes(workspace_bytes)
    if workspace_bytes < 32 * S * S:
        raise ValueError(f"workspace_bytes = {workspace_bytes} holds no {2 * S} x {2 * S} matrix of doubles "
                         f"({32 * S * S} bytes)")


def _on_device(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise ValueError("x, score, K and W must be CUDA tensors (there is no CPU path)")
    if len({t.device for t in tensors}) != 1:
        raise ValueError("the tensors are on different devices")
    return tensors[0].device


def _K_of(k):
    K = k.K if isinstance(k, SteinKernel) else k
    if not isinstance(K, torch.Tensor) or K.dtype != torch.float64 or K.dim() != 2 or K.shape[0] != K.shape[1]:
        raise ValueError("k must be a SteinKernel or a float64 [S, S] tensor")
    if not 2 <= K.shape[0] <= MAX_S:
        raise ValueError(f"S = {K.shape[0]} samples: 2 .. {MAX_S} are supported")
    _on_device(K)
    return K.contiguous()


# --------------------------------------------------------------------------------------------------------------- kernels

def _gram(x, score, workspace_bytes=WORKSPACE_BYTES):
    "x, score [S, D] (unit column stride) -> (gram [2S, 2S] of the rows [x - x_0; score], nonfinite [1]) on the device"
    S, D = x.shape
    # (the kernel walks S rows of D elements of one type from both pointers: checked again where they are taken)
    assert x.shape == score.shape and x.dtype == score.dtype and x.dtype in (torch.float32, torch.float64)
    assert x.is_cuda and x.device == score.device and all(t.stride(1) == 1 or D == 1 for t in (x, score))
    dev, lib = x.device, _hip.lib()
    sp = splits(S, D, workspace_bytes)
    assert sp >= 1 and sp == lib.sgmcmc_stein_splits(S, D, workspace_bytes)
    V, nb = 2 * S, -(-2 * S // TILE)
    slabs = torch.empty(sp * V * V, dtype=torch.float64, device=dev)
    counts = torch.empty(sp * nb, dtype=torch.int64, device=dev)
    gram = torch.empty((V, V), dtype=torch.float64, device=dev)
    bad = torch.empty(1, dtype=torch.int64, device=dev)
    dtype = _hip.F32 if x.dtype == torch.float32 else _hip.F64
    _hip.check(lib.sgmcmc_stein_gram(x.data_ptr(), score.data_ptr(), dtype, S, D, x.stride(0), score.stride(0), sp,
                                     slabs.data_ptr(), counts.data_ptr(), _stream()), "sgmcmc_stein_gram")
    _hip.check(lib.sgmcmc_stein_reduce(slabs.data_ptr(), counts.data_ptr(), sp, S, gram.data_ptr(), bad.data_ptr(),
                                       _stream()), "sgmcmc_stein_reduce")
    return gram, bad


def _finish(gram, bad, d, c2, beta, want_K=True):
    "-> (K or None, r2) of a Gram matrix; c2: a float, or a 1-element device tensor"
    S = gram.shape[0] // 2
    assert gram.dtype == torch.float64 and gram.shape == (2 * S, 2 * S) and gram.is_contiguous() and bad.dtype == torch.int64
    assert not isinstance(c2, torch.Tensor) or (c2.dtype == torch.float64 and c2.numel() == 1 and c2.device == gram.device)
    K = torch.empty((S, S), dtype=torch.float64, device=gram.device) if want_K else None
    r2 = torch.empty((S, S), dtype=torch.float64, device=gram.device)
    on_device = isinstance(c2, torch.Tensor)
    _hip.check(_hip.lib().sgmcmc_stein_finish(gram.data_ptr(), S, float(d), 1.0 if on_device else c2,
                                              c2.data_ptr() if on_device else None, beta, bad.data_ptr(),
                                              None if K is None else K.data_ptr(), r2.data_ptr(), _stream()),
               "sgmcmc_stein_finish")
    return K, r2


def kernel_matrix(x, score, c=1., beta=-0.5, workspace_bytes=WORKSPACE_BYTES):
    """x, score: ``[S, D]`` tensors, or dicts of ``[S, *shape]`` stacks with the same keys (what ``storage.load_samples``
    and ``scores`` return) -> ``SteinKernel``.  Rows may have any stride (every second sample of a longer stack, a column
    slice of a wider matrix); a tensor of a dict is reshaped to [S, D_t] and copied only where that is no view.  For dicts
    the Gram matrices of the tensors are added in key order in fp64 and d is the total dimension.  ``c="median"`` sets c^2
    to the median of r2 over i < j (``torch.median``: the lower of the two middle values), at the cost of a second finish
    launch.  The partial Gram slabs take ``splits(S, D, workspace_bytes)`` (2S)^2 doubles.  No host synchronisation."""
    pairs = _pairs(x, score)
    beta, cval = _check_beta(beta), _check_c(c)
    S = pairs[0][0].shape[0]
    _check_workspace(workspace_bytes, S)
    dev = _on_device(*(t for p in pairs for t in p))
    with torch.cuda.device(dev):
        gram = bad = None
        for a, b in pairs:
            g1, b1 = _gram(a, b, workspace_bytes)
            gram, bad = (g1, b1) if gram is None else (gram + g1, bad + b1)
        d = sum(a.shape[1] for a, _ in pairs)
        if cval is None:
            _, r2 = _finish(gram, bad, d, 1.0, beta, want_K=False)
            iu = torch.triu_indices(S, S, 1, device=dev)
            c2 = torch.median(r2[iu[0], iu[1]]).reshape(1)
            K, r2 = _finish(gram, bad, d, c2, beta)
            cout = torch.sqrt(c2[0])
        else:
            K, r2 = _finish(gram, bad, d, cval * cval, beta)
            cout = cval
    return SteinKernel(K, r2, cout, beta, d, bad[0])


def _forms(K, W):
    "-> (stats [R, 3], row_mean [R, S]) of K and the weight vectors W [R, S] (None: one vector of ones)"
    S = K.shape[0]
    R = 1 if W is None else W.shape[0]
    # (the kernels read R S doubles: what the wrappers checked is checked again where the pointer is taken)
    assert W is None or (W.dtype == torch.float64 and W.shape == (R, S) and W.is_contiguous() and W.device == K.device)
    with torch.cuda.device(K.device):
        rowsum = torch.empty((R, S), dtype=torch.float64, device=K.device)
        row_mean = torch.empty((R, S), dtype=torch.float64, device=K.device)
        stats = torch.empty((R, _hip.STEIN_STATS), dtype=torch.float64, device=K.device)
        _hip.check(_hip.lib().sgmcmc_stein_forms(K.data_ptr(), S, None if W is None else W.data_ptr(), R,
                                                 rowsum.data_ptr(), row_mean.data_ptr(), stats.data_ptr(), _stream()),
                   "sgmcmc_stein_forms")
    return stats, row_mean


def ksd(k):
    "k: a ``SteinKernel`` or a float64 [S, S] device tensor -> ``KSD``.  Deterministic; no host synchronisation."
    stats, row_mean = _forms(_K_of(k), None)
    return KSD(stats[0, 0], stats[0, 1], stats[0, 2], row_mean[0])


def _check_W(W, S, what="W"):
    if not isinstance(W, torch.Tensor) or W.dtype != torch.float64 or W.dim() not in (1, 2) or W.shape[-1] != S:
        raise ValueError(f"{what} must be a float64 [S = {S}] or [R, S = {S}] tensor")
    if W.dim() == 2 and not 1 <= W.shape[0] <= MAX_BATCH:
        raise ValueError(f"R = {W.shape[0]} weight vectors: 1 .. {MAX_BATCH} are supported")


def quadratic_forms(k, W):
    """Q_r = sum_ij W_ri W_rj K_ij / S^2 for W ``[R, S]`` (or ``[S]``: a 0-d result) in fp64 on the device.  The replicates
    ride in the grid; a batch gives the bits of its single calls, and W = 1 gives ``ksd(k).v_stat``."""
    K = _K_of(k)
    _check_W(W, K.shape[0])
    _on_device(K, W)
    stats, _ = _forms(K, W.reshape(-1, K.shape[0]).contiguous())
    return stats[0, 0] if W.dim() == 1 else stats[:, 0]


def wild_bootstrap_test(k, replicates=999, flip_prob=0.5, seed=0, signs=None):
    """The wild bootstrap test of "the draws come from the target" -> ``SteinTest``.  Each replicate is a +-1 Markov chain
    W_r: W_r0 is a fair sign and W_rt = -W_r,t-1 with probability ``flip_prob`` (0.5: independent signs, for independent
    draws; smaller for an autocorrelated chain), drawn as ``torch.rand`` on a device generator seeded with ``seed`` and a
    ``cumprod``.  ``signs`` gives them instead: float64 [R, S] on the device with entries +-1 (``replicates``,
    ``flip_prob`` and ``seed`` are then unused).  p = (1 + #{Q_r >= v_stat}) / (R + 1)."""
    K = _K_of(k)
    S = K.shape[0]
    if signs is None:
        if isinstance(replicates, bool) or not isinstance(replicates, int) or not 1 <= replicates <= MAX_BATCH:
            raise ValueError(f"replicates = {replicates!r}: 1 .. {MAX_BATCH} are supported")
        if isinstance(flip_prob, bool) or not isinstance(flip_prob, (int, float)) or not 0.0 < flip_prob <= 1.0:
            raise ValueError(f"flip_prob = {flip_prob!r}: 0 < flip_prob <= 1 is needed")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed = {seed!r} must be an integer")
        gen = torch.Generator(device=K.device)
        gen.manual_seed(seed)
        u = torch.rand((replicates, S), generator=gen, device=K.device, dtype=torch.float64)
        p = torch.full((S,), float(flip_prob), dtype=torch.float64, device=K.device)
        p[0] = 0.5
        signs = torch.cumprod(torch.where(u < p, -1.0, 1.0).to(torch.float64), dim=1)
    else:
        _check_W(signs, S, "signs")
        if signs.dim() != 2:
            raise ValueError(f"signs must be a float64 [R, S = {S}] tensor")
        _on_device(K, signs)
    v = _forms(K, None)[0][0, 0]
    null = _forms(K, signs.contiguous())[0][:, 0]
    p = (1 + (null >= v).sum()).to(torch.float64) / (null.shape[0] + 1)
    return SteinTest(v, null, p)


def thin(k, m):
    """Stein thinning -> ``Thinning``: pi_1 = argmin_j K_jj, pi_m = argmin_j [K_jj / 2 + sum_{a < m} K(pi_a, j)] (ties go to
    the smaller index, picks may repeat), and the KSD of every prefix.  One workgroup, exactly m trips; no host
    synchronisation."""
    K = _K_of(k)
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= MAX_PICKS:
        raise ValueError(f"m = {m!r}: 1 .. {MAX_PICKS} picks are supported")
    with torch.cuda.device(K.device):
        indices = torch.empty(m, dtype=torch.int64, device=K.device)
        path = torch.empty(m, dtype=torch.float64, device=K.device)
        _hip.check(_hip.lib().sgmcmc_stein_thin(K.data_ptr(), K.shape[0], m, indices.data_ptr(), path.data_ptr(), _stream()),
                   "sgmcmc_stein_thin")
    return Thinning(indices, path)
