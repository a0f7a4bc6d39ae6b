"""How many directions of weight space do the data determine?  The effective dimensionality N_eff(alpha) = sum_i lambda_i /
(lambda_i + alpha) of a Hessian's eigenvalues (MacKay 1992; Maddox et al. 2020), from Lanczos with full reorthogonalisation
on the device (``csrc/lanczos_hip.inc``; C ABI ``sgmcmc_lanczos_*``, ``sgmcmc_tridiag_eig``, ``sgmcmc_effdim``, definitions
in ``include/sgmcmc_hip.h``).  The reference's ``testing/test_eff_dim.py`` expects a module ``bnn_priors.eff_dim`` that its
tree does not have; this is that module.

    unflatten_like, hess_vec_prod, hessian        autograd: Hessian-vector products and the dense Hessian of small problems
    model_hvp                                     v -> H v of a model's -log_likelihood or potential on (x, y)
    lanczos                                       m steps on a matrix or a callable -> ``Lanczos``
    symeig_positive_lanczos                       eigenvalues (and vectors) of a matrix, the reference's "positive" rule
    hessian_eigs_positive_lanczos                 the same on ``hess_vec_prod``
    effective_dimensionality                      N_eff of raw Ritz values for a list of alphas

One step is two passes of classical Gram-Schmidt against every stored row (which subsumes the three-term recurrence); every
dot product and norm is a sum over D in an order fixed by (D, ``workspace_bytes``) -- not by the row stride of V or by the
step -- without floating-point atomics, so two calls, or a strided V and its contiguous copy, give the same bits.  The host
reads one flag per step (the breakdown test); on a breakdown it supplies a random restart vector, T becomes block diagonal
and repeated or zero eigenvalues are found with their multiplicities.  CPU tensors are refused by the device part (the
autograd helpers are plain torch).
"""
import collections
import math

import torch

from . import _hip
from .calibration import _stream

__all__ = ("Lanczos", "unflatten_like", "hess_vec_prod", "hessian", "model_hvp", "lanczos", "tridiag_eig",
           "symeig_positive_lanczos", "hessian_eigs_positive_lanczos", "effective_dimensionality", "splits", "CHUNK", "ROWS",
           "MAX_M", "MAX_SPLITS", "MAX_BATCH", "MAX_D", "MAX_DENSE", "WORKSPACE_BYTES")

CHUNK = _hip.LANCZOS_CHUNK               # coordinates of one chunk of a dot product (SGMCMC_LANCZOS_CHUNK)
ROWS = _hip.LANCZOS_ROWS                 # rows of V one workgroup of the dots pass takes (SGMCMC_LANCZOS_ROWS)
MAX_M = _hip.LANCZOS_MAX_M               # Lanczos vectors, and the order of a tridiagonal matrix
MAX_SPLITS = _hip.LANCZOS_MAX_SPLITS
MAX_BATCH = _hip.LANCZOS_MAX_BATCH       # tridiagonal matrices of one launch; alphas of one launch
MAX_D = 2 ** 31 - 1
MAX_DENSE = 4096                         # ``hessian`` refuses more parameters
WORKSPACE_BYTES = 256 << 20
EPS = 2.0 ** -52

Lanczos = collections.namedtuple("Lanczos", "alpha beta V m restarts theta Y residual nonfinite")
Lanczos.__doc__ = ("fp64 device tensors: alpha [m], beta [m] the tridiagonal T (beta[i] couples i and i + 1; beta[m - 1] is "
                   "the norm left after the last step; exactly 0 where a restart happened), V [m, D] the orthonormal rows, "
                   "theta [m] the Ritz values ascending, Y [m, m] their vectors in columns, residual [m] = |beta[m - 1] "
                   "Y[m - 1, i]|; m, restarts (ints); nonfinite (int): NaN / Inf elements met, which make the outputs NaN")


def splits(D, workspace_bytes=WORKSPACE_BYTES):
    """Workgroups that share the chunks of a dot product (``lanczos::splits``): workgroup b walks chunks b, b + splits, ...
    A function of (D, workspace_bytes) alone; 0 if the workspace holds no row of partial sums."""
    return max(0, min(-(-D // CHUNK), MAX_SPLITS, workspace_bytes // (8 * _hip.LANCZOS_WIDTH)))


# -------------------------------------------------------------------------------------------------------------- autograd

def unflatten_like(vec_flat, parameters):
    "views of the flat vector shaped like the parameters, in their order"
    parameters = list(parameters)
    n = sum(p.numel() for p in parameters)
    if vec_flat.dim() != 1 or vec_flat.numel() != n:
        raise ValueError(f"vec_flat has shape {tuple(vec_flat.shape)}, the parameters hold {n} elements")
    out, at = [], 0
    for p in parameters:
        out.append(vec_flat[at:at + p.numel()].view(p.shape))
        at += p.numel()
    return out


def _flat64(tensors, like):
    return torch.cat([(torch.zeros_like(p) if t is None else t).reshape(-1).to(torch.float64) for t, p in zip(tensors, like)])


def hess_vec_prod(vec_all, parameters, fn, dataloader):
    """H v for H the Hessian of sum over the batches of ``fn(*batch)`` (a scalar) in the parameters: the products of the
    batches are summed, stored in ``p.grad`` of every parameter (in its dtype) and returned as a flat fp64 vector.
    ``vec_all``: flat, or a list shaped like the parameters."""
    parameters = list(parameters)
    vecs = unflatten_like(vec_all, parameters) if isinstance(vec_all, torch.Tensor) else list(vec_all)
    vecs = [v.to(device=p.device, dtype=p.dtype) for v, p in zip(vecs, parameters)]
    total = [torch.zeros_like(p) for p in parameters]
    for batch in dataloader:
        with torch.enable_grad():
            loss = fn(*batch)
            grads = torch.autograd.grad(loss, parameters, create_graph=True, allow_unused=True)
            dot = sum((g * v).sum() for g, v in zip(grads, vecs) if g is not None)
            hv = torch.autograd.grad(dot, parameters, allow_unused=True) if isinstance(dot, torch.Tensor) and \
                dot.requires_grad else [None] * len(parameters)
        total = [t if h is None else t + h for t, h in zip(total, hv)]
    for p, t in zip(parameters, total):
        p.grad = t.detach()
    return _flat64(total, parameters).detach()


def hessian(parameters, fn, dataloader):
    "the dense [D, D] Hessian (fp64) of sum over the batches of ``fn(*batch)``, column by column; D <= MAX_DENSE"
    parameters = list(parameters)
    D = sum(p.numel() for p in parameters)
    if D > MAX_DENSE:
        raise ValueError(f"D = {D} parameters: the dense Hessian is for D <= {MAX_DENSE}")
    dev = parameters[0].device
    H = torch.zeros((D, D), dtype=torch.float64, device=dev)
    for batch in dataloader:
        with torch.enable_grad():
            grads = torch.autograd.grad(fn(*batch), parameters, create_graph=True, allow_unused=True)
            flat = torch.cat([(torch.zeros_like(p) if g is None else g).reshape(-1) for g, p in zip(grads, parameters)])
            for i in range(D):
                if not flat.requires_grad:
                    break
                row = torch.autograd.grad(flat[i], parameters, retain_graph=True, allow_unused=True)
                H[i] += _flat64(row, parameters)
    return H


def model_hvp(model, x, y, what="likelihood", batch_size=None):
    """A callable ``v [D] fp64 -> H v [D] fp64`` on the model's parameters in ``named_parameters()`` order, H the Hessian of
    the full-data ``-log_likelihood`` ("likelihood") or of the potential ("potential": ``-log_prior`` added once).  With
    ``batch_size`` the batches are summed as ``stein.scores`` sums them.  Every call runs on the plain torch layers (the
    custom-kernel autograd functions cannot be differentiated twice) and leaves the switches, the train / eval mode and the
    ``requires_grad`` flags as it found them."""
    if what not in ("likelihood", "potential"):
        raise ValueError(f"what = {what!r}: 'likelihood' or 'potential'")
    if batch_size is not None and (isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1):
        raise ValueError(f"batch_size = {batch_size!r} must be a positive integer")
    if len(x) != len(y):
        raise ValueError(f"x holds {len(x)} rows, y {len(y)}")
    plist = [p for _, p in model.named_parameters()]
    if not plist:
        raise ValueError("the model has no parameters")
    n = len(x)
    step = n if batch_size is None or batch_size >= n else batch_size

    def hvp(v):
        from . import bnlink
        from .evaluation import _plain_torch_layers
        if not isinstance(v, torch.Tensor) or v.dim() != 1 or v.numel() != sum(p.numel() for p in plist):
            raise ValueError("v must be a flat vector with one element per parameter")
        vecs = [u.to(device=p.device, dtype=p.dtype) for u, p in zip(unflatten_like(v, plist), plist)]
        need = [p.requires_grad for p in plist]
        link = bnlink.ENABLED
        total = [torch.zeros_like(p) for p in plist]

        def add(loss):
            grads = torch.autograd.grad(loss, plist, create_graph=True, allow_unused=True)
            dot = sum((g * u).sum() for g, u in zip(grads, vecs) if g is not None)
            if isinstance(dot, torch.Tensor) and dot.requires_grad:
                for t, h in zip(total, torch.autograd.grad(dot, plist, allow_unused=True)):
                    if h is not None:
                        t += h

        try:
            bnlink.ENABLED = False
            for p in plist:
                p.requires_grad_(True)
            with _plain_torch_layers(), torch.enable_grad():
                if what == "potential":
                    add(-model.log_prior())
                for b in range(0, n, step):
                    xb, yb = x[b:b + step], y[b:b + step]
                    # eff_num_data = len(batch) leaves the plain sum over the batch (see stein.scores)
                    add(-model.log_likelihood(xb, yb, len(xb)))
        finally:
            bnlink.ENABLED = link
            for p, r in zip(plist, need):
                p.requires_grad_(r)
        return _flat64(total, plist).detach()

    return hvp


# ---------------------------------------------------------------------------------------------------------------- device

def _check_int(value, name, lo, hi=None):
    if isinstance(value, bool) or not isinstance(value, int) or value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name} = {value!r}: an integer {lo} .. {'' if hi is None else hi} is needed")
    return value


def _check_workspace(workspace_bytes):
    _check_int(workspace_bytes, "workspace_bytes", 0)
    if workspace_bytes < 8 * _hip.LANCZOS_WIDTH:
        raise ValueError(f"workspace_bytes = {workspace_bytes} holds no row of partial sums ({8 * _hip.LANCZOS_WIDTH} bytes)")


class _Step:
    """The buffers and launches of one Lanczos step on V [rows, D] (fp64, unit column stride, any row stride): ``run(j, w)``
    orthogonalises w (fp64, contiguous, in place) against rows 0 .. j twice, finishes alpha[j] and beta[j] and writes row
    j + 1 if V has one.  ``state`` as include/sgmcmc_hip.h describes it."""

    def __init__(self, V, workspace_bytes=WORKSPACE_BYTES, rtol=None):
        assert V.is_cuda and V.dtype == torch.float64 and V.dim() == 2 and (V.stride(1) == 1 or V.shape[1] == 1)
        assert V.stride(0) >= 0 and 1 <= V.shape[0] <= MAX_M and 1 <= V.shape[1] <= MAX_D
        self.V, self.D, self.dev = V, V.shape[1], V.device
        self.rtol = 64 * EPS * math.sqrt(self.D) if rtol is None else float(rtol)
        self.splits = splits(self.D, workspace_bytes)
        lib = self.lib = _hip.lib()
        assert self.splits >= 1 and self.splits == lib.sgmcmc_lanczos_splits(self.D, workspace_bytes)
        assert self.splits * _hip.LANCZOS_WIDTH * 8 == lib.sgmcmc_lanczos_workspace_bytes(self.D, workspace_bytes)
        with torch.cuda.device(self.dev):
            self.ws = torch.zeros(self.splits * _hip.LANCZOS_WIDTH, dtype=torch.float64, device=self.dev)
            self.coef = torch.zeros((2, MAX_M), dtype=torch.float64, device=self.dev)
            self.state = torch.zeros(_hip.LANCZOS_STATE, dtype=torch.float64, device=self.dev)
            self.alpha = torch.zeros(MAX_M, dtype=torch.float64, device=self.dev)
            self.beta = torch.zeros(MAX_M, dtype=torch.float64, device=self.dev)

    def run(self, j, w, restart=False):
        V, D, lib, sp = self.V, self.D, self.lib, self.splits
        # (the kernels read j + 1 rows of D doubles and write D doubles: checked where the pointers are taken)
        assert 0 <= j < V.shape[0] and w.dtype == torch.float64 and w.shape == (D,) and w.is_contiguous()
        assert w.device == self.dev
        rows, vs = j + 1, V.stride(0)
        nxt = V[j + 1] if j + 1 < V.shape[0] else None
        with torch.cuda.device(self.dev):
            st = _stream()
            for p in (0, 1):
                _hip.check(lib.sgmcmc_lanczos_dots(V.data_ptr(), vs, rows, w.data_ptr(), D, sp, self.ws.data_ptr(), st),
                           "sgmcmc_lanczos_dots")
                _hip.check(lib.sgmcmc_lanczos_reduce(self.ws.data_ptr(), sp, rows, p, j, int(restart), self.rtol,
                                                     self.coef.data_ptr(), None, None, self.state.data_ptr(), st),
                           "sgmcmc_lanczos_reduce")
                _hip.check(lib.sgmcmc_lanczos_update(V.data_ptr(), vs, rows, w.data_ptr(), D, sp, self.coef[p].data_ptr(), 0,
                                                     None, None, self.ws.data_ptr(), st), "sgmcmc_lanczos_update")
            _hip.check(lib.sgmcmc_lanczos_reduce(self.ws.data_ptr(), sp, rows, 2, j, int(restart), self.rtol,
                                                 self.coef.data_ptr(), self.alpha.data_ptr(), self.beta.data_ptr(),
                                                 self.state.data_ptr(), st), "sgmcmc_lanczos_reduce")
            if nxt is not None:
                _hip.check(lib.sgmcmc_lanczos_update(None, 0, rows, w.data_ptr(), D, sp, None, 1, self.state.data_ptr(),
                                                     nxt.data_ptr(), None, st), "sgmcmc_lanczos_update")


def tridiag_eig(alpha, beta):
    """Eigenvalues and vectors of a batch of symmetric tridiagonal matrices in ONE launch: alpha [B, m] (or [m]) the
    diagonals, beta [B, m] the off-diagonals (beta[:, m - 1] is not read), fp64 on the device -> (theta [B, m] ascending,
    Y [B, m, m] with the vectors in columns, sweeps [B] int32, failed [B] int32: an eigenvalue not deflated after 60 sweeps
    or NaN, with NaN outputs)."""
    single = isinstance(alpha, torch.Tensor) and alpha.dim() == 1
    if single:
        alpha, beta = alpha[None], beta[None] if isinstance(beta, torch.Tensor) else beta
    for t, name in ((alpha, "alpha"), (beta, "beta")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 2:
            raise ValueError(f"{name} must be a float64 [B, m] or [m] tensor")
        if not t.is_cuda:
            raise ValueError("alpha and beta must be CUDA tensors (there is no CPU path)")
    if alpha.shape != beta.shape or alpha.device != beta.device:
        raise ValueError(f"alpha {tuple(alpha.shape)} and beta {tuple(beta.shape)} differ in shape or device")
    B, m = alpha.shape
    if not 1 <= m <= MAX_M or not 1 <= B <= MAX_BATCH:
        raise ValueError(f"B = {B} matrices of order m = {m}: 1 .. {MAX_BATCH} of 1 .. {MAX_M} are supported")
    alpha, beta = alpha.contiguous(), beta.contiguous()
    dev = alpha.device
    with torch.cuda.device(dev):
        theta = torch.empty((B, m), dtype=torch.float64, device=dev)
        Y = torch.empty((B, m, m), dtype=torch.float64, device=dev)
        work = torch.empty((B, m, m), dtype=torch.float64, device=dev)
        sweeps = torch.empty(B, dtype=torch.int32, device=dev)
        failed = torch.empty(B, dtype=torch.int32, device=dev)
        _hip.check(_hip.lib().sgmcmc_tridiag_eig(alpha.data_ptr(), beta.data_ptr(), B, m, m, theta.data_ptr(), Y.data_ptr(),
                                                 work.data_ptr(), sweeps.data_ptr(), failed.data_ptr(), _stream()),
                   "sgmcmc_tridiag_eig")
    return (theta[0], Y[0], sweeps[0], failed[0]) if single else (theta, Y, sweeps, failed)


def _iterate(A, n_steps, v0, seed, workspace_bytes, breakdown_rtol):
    "-> (_Step with alpha, beta, V filled; m, restarts, nonfinite): the Lanczos loop without the eigensolve"
    if callable(A) and not isinstance(A, torch.Tensor):
        if v0 is None:
            raise ValueError("a callable A needs v0 (its size and device)")
        matvec = A
    else:
        if not isinstance(A, torch.Tensor) or A.dim() != 2 or A.shape[0] != A.shape[1] or \
                A.dtype not in (torch.float32, torch.float64):
            raise ValueError("A must be a float32 or float64 [D, D] tensor or a callable v -> A v")
        if not A.is_cuda:
            raise ValueError("A must be a CUDA tensor (there is no CPU path)")
        A64 = A.to(torch.float64)
        matvec = lambda v: torch.mv(A64, v)     # noqa: E731
    if v0 is not None:
        if not isinstance(v0, torch.Tensor) or v0.dim() != 1 or v0.dtype not in (torch.float32, torch.float64):
            raise ValueError("v0 must be a float32 or float64 [D] tensor")
        if not v0.is_cuda:
            raise ValueError("v0 must be a CUDA tensor (there is no CPU path)")
        if isinstance(A, torch.Tensor) and (v0.shape[0] != A.shape[0] or v0.device != A.device):
            raise ValueError("v0 does not match A in size or device")
    D = A.shape[0] if isinstance(A, torch.Tensor) else v0.shape[0]
    dev = A.device if isinstance(A, torch.Tensor) else v0.device
    _check_int(n_steps, "n_steps", 1, MAX_M)
    _check_int(seed, "seed", 0)
    _check_workspace(workspace_bytes)
    if not 1 <= D <= MAX_D:
        raise ValueError(f"D = {D}: 1 .. {MAX_D} coordinates are supported")
    if breakdown_rtol is not None and not 0.0 <= breakdown_rtol < 1.0:
        raise ValueError(f"breakdown_rtol = {breakdown_rtol!r}: 0 <= rtol < 1 is needed")
    m = min(n_steps, D)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    with torch.cuda.device(dev):
        V = torch.zeros((m, D), dtype=torch.float64, device=dev)
        step = _Step(V, workspace_bytes, breakdown_rtol)
        fresh = lambda: torch.randn(D, generator=gen, device=dev, dtype=torch.float64)     # noqa: E731
        start = fresh() if v0 is None else v0.to(torch.float64)
        norm = torch.linalg.vector_norm(start)
        if float(norm) == 0.0:
            raise ValueError("the start vector is zero")
        V[0] = start / norm
        restarts = 0
        for j in range(m):
            w = matvec(V[j]).to(torch.float64).contiguous()
            if w.shape != (D,) or w.device != dev:
                raise ValueError(f"A v has shape {tuple(w.shape)} on {w.device}: [{D}] on {dev} is needed")
            if w.data_ptr() == V[j].data_ptr():
                w = w.clone()
            step.run(j, w)
            state = step.state.tolist()                 # the one synchronisation of a step
            if state[4] != 0 or not math.isfinite(state[2]):
                return step, m, restarts, max(int(state[4]), 1)
            if state[3] != 0 and j + 1 < m:
                for _ in range(3):
                    step.run(j, fresh(), restart=True)
                    if step.state[3].item() == 0:
                        break
                else:
                    raise RuntimeError(f"Lanczos: no restart vector survived the orthogonalisation at step {j}")
                restarts += 1
        bad = 0 if bool(torch.isfinite(V).all()) else 1
    return step, m, restarts, bad


def lanczos(A, n_steps, v0=None, seed=0, workspace_bytes=WORKSPACE_BYTES, breakdown_rtol=None):
    """``n_steps`` Lanczos steps with full reorthogonalisation -> ``Lanczos``.  ``A``: a float32 or float64 ``[D, D]`` device
    tensor (the product is ``torch.mv`` in fp64) or a callable ``v [D] fp64 -> A v`` on the device, which needs ``v0``.
    m = min(n_steps, D) <= MAX_M.  The start vector is ``v0`` (normalised) or ``torch.randn`` from a device generator seeded
    with ``seed``; the same generator supplies a restart vector when beta_j <= breakdown_rtol * scale (the default rtol is
    64 eps sqrt(D), scale the running max of |alpha| and beta): up to three candidates, each orthogonalised by the step
    kernels, the first whose norm survives by more than rtol is kept.  The host reads one small state vector per step."""
    step, m, restarts, bad = _iterate(A, n_steps, v0, seed, workspace_bytes, breakdown_rtol)
    alpha, beta, V = step.alpha[:m].clone(), step.beta[:m].clone(), step.V
    if bad:
        nan = torch.full_like(alpha, math.nan)
        return Lanczos(nan, nan.clone(), torch.full_like(V, math.nan), m, restarts, nan.clone(),
                       torch.full((m, m), math.nan, dtype=torch.float64, device=V.device), nan.clone(), bad)
    theta, Y, _, failed = tridiag_eig(alpha, beta)
    if int(failed):
        raise RuntimeError("sgmcmc_tridiag_eig: an eigenvalue was not deflated after 60 sweeps")
    return Lanczos(alpha, beta, V, m, restarts, theta, Y, (beta[m - 1] * Y[m - 1]).abs(), 0)


def _ritz(V, theta, Y, k, positive):
    "U [D, k] of the k largest Ritz values (sign rule, 'positive' zeroing) on the matrix pipe"
    m, D = V.shape
    assert V.dtype == torch.float64 and V.is_cuda and (V.stride(1) == 1 or D == 1) and 1 <= k <= m <= MAX_M
    assert theta.shape == (m,) and Y.shape == (m, m) and theta.is_contiguous() and Y.is_contiguous()
    assert theta.dtype == Y.dtype == torch.float64 and theta.device == Y.device == V.device
    with torch.cuda.device(V.device):
        U = torch.empty((D, k), dtype=torch.float64, device=V.device)
        _hip.check(_hip.lib().sgmcmc_lanczos_ritz(V.data_ptr(), V.stride(0), m, D, Y.data_ptr(), theta.data_ptr(), m - k, k,
                                                  int(positive), U.data_ptr(), _stream()), "sgmcmc_lanczos_ritz")
    return U


def symeig_positive_lanczos(A, n_eigs=-1, vecs=False, n_steps=None, **kw):
    """Eigenvalues of a symmetric matrix (or callable, see ``lanczos``) by Lanczos -> ``(vals [k], vecs [D, k] or None)``,
    ascending as ``eigh`` returns them.  ``n_eigs = -1``: all D (D <= MAX_M); otherwise the largest ``n_eigs`` Ritz values of
    ``n_steps`` steps (default ``n_eigs``).  The "positive" rule of the reference's test: a Ritz value <= m eps max|theta| is
    returned as exactly 1.0 and its vector as exact zeros.  Each vector's sign makes its component along the start vector
    non-negative."""
    D = A.shape[0] if isinstance(A, torch.Tensor) else (kw["v0"].shape[0] if kw.get("v0") is not None else None)
    if D is None:
        raise ValueError("a callable A needs v0 (its size and device)")
    if n_eigs == -1:
        if D > MAX_M:
            raise ValueError(f"n_eigs = -1 needs D <= {MAX_M}; D = {D}")
        n_eigs = D
        steps = D
    else:
        _check_int(n_eigs, "n_eigs", 1, min(D, MAX_M))
        steps = n_eigs if n_steps is None else _check_int(n_steps, "n_steps", n_eigs, MAX_M)
    res = lanczos(A, steps, **kw)
    k = min(n_eigs, res.m)
    raw = res.theta[res.m - k:]
    top = res.theta.abs().max()
    small = raw <= res.m * EPS * top
    vals = torch.where(small, torch.ones_like(raw), raw)
    U = _ritz(res.V, res.theta, res.Y, k, True) if vecs and not res.nonfinite else None
    if vecs and U is None:
        U = torch.full((D, k), math.nan, dtype=torch.float64, device=raw.device)
    return vals, U


def hessian_eigs_positive_lanczos(parameters, fn, dataloader, n_eigs=-1, vecs=False, **kw):
    "``symeig_positive_lanczos`` on ``hess_vec_prod(., parameters, fn, dataloader)``; the parameters must be on the device"
    parameters = list(parameters)
    D = sum(p.numel() for p in parameters)
    dev = parameters[0].device
    if dev.type != "cuda":
        raise ValueError("the parameters must be CUDA tensors (there is no CPU path)")
    if kw.get("v0") is None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(kw.get("seed", 0))
        kw["v0"] = torch.randn(D, generator=gen, device=dev, dtype=torch.float64)
    grads = [p.grad for p in parameters]
    try:
        return symeig_positive_lanczos(lambda v: hess_vec_prod(v, parameters, fn, dataloader), n_eigs, vecs, **kw)
    finally:
        for p, g in zip(parameters, grads):
            p.grad = g


def effective_dimensionality(eigs, alpha):
    """N_eff = sum over eigs > 0 of eigs / (eigs + alpha) -> ``(n_eff [..., A] fp64, nonpositive [...], nonfinite [...]
    int64)`` on the device.  ``eigs [..., k]``: RAW Ritz values (float32 or float64), not the "positive" ones; ``alpha``: a
    positive number or a list / tensor of A of them (a number gives ``[..., 1]``).  Entries <= 0 and NaN / Inf entries are
    left out of the sum and counted.  Compensated sums in a fixed order; rows and alphas ride in the grid, so a batch gives
    the bits of its single calls."""
    if not isinstance(eigs, torch.Tensor) or eigs.dim() < 1 or eigs.dtype not in (torch.float32, torch.float64):
        raise ValueError("eigs must be a float32 or float64 [..., k] tensor")
    if eigs.numel() == 0:
        raise ValueError("eigs is empty")
    if not eigs.is_cuda:
        raise ValueError("eigs must be a CUDA tensor (there is no CPU path)")
    al = torch.as_tensor(alpha, dtype=torch.float64).reshape(-1)
    if al.numel() < 1 or al.numel() > MAX_BATCH or not bool((al > 0).all()) or not bool(torch.isfinite(al).all()):
        raise ValueError(f"alpha = {alpha!r}: 1 .. {MAX_BATCH} positive finite numbers are needed")
    k = eigs.shape[-1]
    flat = eigs.reshape(-1, k).to(torch.float64).contiguous()
    B, A = flat.shape[0], al.numel()
    dev = eigs.device
    with torch.cuda.device(dev):
        al = al.to(dev)
        out = torch.empty((B, A), dtype=torch.float64, device=dev)
        nonpos = torch.empty(B, dtype=torch.int64, device=dev)
        nonfin = torch.empty(B, dtype=torch.int64, device=dev)
        _hip.check(_hip.lib().sgmcmc_effdim(flat.data_ptr(), B, k, al.data_ptr(), A, out.data_ptr(), nonpos.data_ptr(),
                                            nonfin.data_ptr(), _stream()), "sgmcmc_effdim")
    lead = eigs.shape[:-1]
    return out.reshape(*lead, A), nonpos.reshape(lead), nonfin.reshape(lead)
