"""The marginal likelihood of the Rao-Blackwellised regression model on the device (``csrc/raob_hip.inc``; C ABI
``sgmcmc_raob_gram`` / ``sgmcmc_raob_factor`` / ``sgmcmc_raob_grad`` / ``sgmcmc_raob_predict``, definitions in
``include/sgmcmc_hip.h``).  The reference's ``RaoBRegressionModel`` (``models/base.py:194-311``) gives the last layer an
iid Normal(0, ``last_layer_var``) prior and integrates it out; with f [N, F] the features of the training rows,
G = f^T f, c = f^T y and A = last_layer_var G + noise_var I = L L^T, b = A^-1 c:

    gram                     (G, c, yy) in fp64
    marginal_log_likelihood  log p(y | f), differentiable in f and in ``noise_var`` by the closed forms (an
                             ``autograd.Function``: forward is the Gram pass and one workgroup that factors A, backward
                             one launch); what a sampler differentiates
    posterior                the state record of one factorisation: the scalars, b, L^-1, A^-1, G, c, L
    predictive               mean and variance of the posterior predictive at the rows of f*

Everything is fp64 in an order fixed by (N, F), so two calls give the same bits; fp32 inputs are widened in the kernels
and the results rounded once.  Nothing synchronises with the host: a ``noise_var`` that is a device tensor is read on the
device.  An A that is not positive definite (an overflowed Gram matrix) makes every result NaN; nothing raises.
"""
import collections
import math

import torch

from . import _hip
from .calibration import _stream

__all__ = ("RaoBPosterior", "MAX_FEATURES", "gram", "marginal_log_likelihood", "posterior", "predictive")

MAX_FEATURES = _hip.RAOB_MAX_F
MAX_ROWS = 2 ** 31 - 1

RaoBPosterior = collections.namedtuple(
    "RaoBPosterior", "log_likelihood dnoise_var noise_var last_layer_var b Linv Ainv G c yy L state")
RaoBPosterior.__doc__ = ("views of one fp64 state record on the device: log_likelihood, dnoise_var = d log p / d noise_var, "
                         "noise_var, last_layer_var, yy: 0-dim; b [F] = A^-1 c; Linv, Ainv, G, L [F, F] with A = "
                         "last_layer_var G + noise_var I = L L^T; c [F]; state: the record itself")


def _is_f64(x):
    return _hip.F64 if x.dtype == torch.float64 else _hip.F32


def _features(f, what="f"):
    if not isinstance(f, torch.Tensor) or f.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be a float32 or float64 tensor")
    if f.dim() != 2:
        raise ValueError(f"{what} must be an [N, F] tensor, not of shape {tuple(f.shape)}")
    N, F = f.shape
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError(f"{what} has {F} features: 1 .. {MAX_FEATURES} are supported")
    if not 1 <= N <= MAX_ROWS:
        raise ValueError(f"{what} has {N} rows: 1 .. {MAX_ROWS} are supported")
    return N, F


def _on_device(t, what):
    if not t.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor (there is no CPU path)")


def _targets(y, f):
    N = f.shape[0]
    if not isinstance(y, torch.Tensor) or tuple(y.shape) != (N, 1):
        raise ValueError(f"y must be an [N, 1] = {(N, 1)} tensor (one output, as in the reference)")
    if y.dtype != f.dtype:
        raise ValueError(f"y is {y.dtype}, f is {f.dtype}: they must agree")
    _on_device(f, "f")
    if y.device != f.device:
        raise ValueError("y must be on f's device")


def _positive(value, what):
    value = float(value)
    if not math.isfinite(value) or not value > 0.0:
        raise ValueError(f"{what} = {value} must be finite and > 0")
    return value


def _noise(noise_var, f):
    "-> (the float, or 0. with a device tensor; the 0-dim tensor or None)"
    if isinstance(noise_var, torch.Tensor):
        if not noise_var.is_cuda or noise_var.device != f.device:
            raise ValueError("a noise_var tensor must be on f's device")
        return 0.0, noise_var
    return _positive(noise_var, "noise_var"), None


def _factor(f, y, noise_float, noise_tensor, last_layer_var):
    "Gram pass and factor pass -> the state record (fp64, on f's device)"
    N, F = f.shape
    lib = _hip.lib()
    with torch.cuda.device(f.device):
        work = torch.empty(lib.sgmcmc_raob_workspace_doubles(N, F), dtype=torch.float64, device=f.device)
        state = torch.empty(_hip.raob_state_doubles(F), dtype=torch.float64, device=f.device)
        v64 = None if noise_tensor is None else noise_tensor.detach().to(torch.float64)
        _hip.check(lib.sgmcmc_raob_gram(f.data_ptr(), y.data_ptr(), _is_f64(f), N, F, work.data_ptr(), _stream()),
                   "sgmcmc_raob_gram")
        _hip.check(lib.sgmcmc_raob_factor(work.data_ptr(), N, F, last_layer_var, noise_float,
                                          0 if v64 is None else v64.data_ptr(), state.data_ptr(), _stream()),
                   "sgmcmc_raob_factor")
    return state


def _record(state, F):
    s, n = _hip.RAOB_SCALARS, F * F
    sq = lambda at: state[at:at + n].view(F, F)                                  # noqa: E731
    return RaoBPosterior(state[0], state[1], state[2], state[3], state[s:s + F], sq(s + F), sq(s + F + n),
                         sq(s + F + 2 * n), state[s + F + 3 * n:s + 2 * F + 3 * n], state[8], sq(s + 2 * F + 3 * n), state)


def _checked(f, y, noise_var, last_layer_var):
    "every check that needs no device comes before the ones that do"
    s2 = _positive(last_layer_var, "last_layer_var")
    if not isinstance(noise_var, torch.Tensor):
        _positive(noise_var, "noise_var")
    elif noise_var.dim() != 0 or not noise_var.dtype.is_floating_point:
        raise ValueError("noise_var must be a float or a 0-dim floating-point tensor")
    _features(f)
    _targets(y, f)
    noise_float, noise_tensor = _noise(noise_var, f)
    return f.contiguous(), y.contiguous(), noise_float, noise_tensor, s2


def gram(f, y):
    "f [N, F], y [N, 1] (fp32 or fp64 device tensors) -> (G [F, F], c [F], yy 0-dim) in fp64; no host synchronisation"
    f, y, *_ = _checked(f, y, 1.0, 1.0)
    rec = _record(_factor(f.detach(), y.detach(), 1.0, None, 1.0), f.shape[1])
    return rec.G, rec.c, rec.yy


class _MarginalLogLikelihood(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, y, noise_tensor, noise_float, last_layer_var):
        state = _factor(f, y, noise_float, noise_tensor, last_layer_var)
        ctx.save_for_backward(f, y, state)
        ctx.noise_dtype = None if noise_tensor is None else noise_tensor.dtype
        return state[0].to(f.dtype, copy=True)                 # (not a view of the saved record)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, upstream):
        f, y, state = ctx.saved_tensors
        N, F = f.shape
        want_v = ctx.noise_dtype is not None and ctx.needs_input_grad[2]
        with torch.cuda.device(f.device):
            upstream = upstream.to(f.dtype).contiguous()
            grad_f = torch.empty_like(f)
            grad_v = torch.empty(1, dtype=torch.float64, device=f.device) if want_v else None
            _hip.check(_hip.lib().sgmcmc_raob_grad(f.data_ptr(), y.data_ptr(), _is_f64(f), N, F, state.data_ptr(),
                                                   upstream.data_ptr(), grad_f.data_ptr(),
                                                   grad_v.data_ptr() if want_v else 0, _stream()), "sgmcmc_raob_grad")
        return (grad_f if ctx.needs_input_grad[0] else None, None,
                grad_v.reshape(()).to(ctx.noise_dtype) if want_v else None, None, None)


def marginal_log_likelihood(f, y, noise_var, last_layer_var):
    """log p(y | f) of the model with the last layer integrated out -> a 0-dim tensor of f's dtype (the fp64 value rounded
    once, as the reference does).  f [N, F] and y [N, 1] are device tensors of one dtype (fp32 or fp64), F <= 64;
    ``last_layer_var`` is a float; ``noise_var`` is a float or a 0-dim device tensor, which gets its gradient when it
    requires one.  y gets none.  Differentiable once."""
    f, y, noise_float, noise_tensor, s2 = _checked(f, y, noise_var, last_layer_var)
    return _MarginalLogLikelihood.apply(f, y.detach(), noise_tensor, noise_float, s2)


def posterior(f, y, noise_var, last_layer_var):
    "-> ``RaoBPosterior`` of the last layer's weights given (f, y); carries no gradient"
    f, y, noise_float, noise_tensor, s2 = _checked(f, y, noise_var, last_layer_var)
    return _record(_factor(f.detach(), y.detach(), noise_float, noise_tensor, s2), f.shape[1])


def predictive(posterior, f_star):
    """f_star [M, F] (fp32 or fp64) -> (mean [M], var [M]) in fp64: mean = last_layer_var f* . b, var = noise_var
    last_layer_var |L^-1 f*|^2 + noise_var, which is never below noise_var"""
    if not isinstance(posterior, RaoBPosterior):
        raise ValueError("posterior must be a RaoBPosterior (raob.posterior)")
    M, F = _features(f_star, "f_star")
    state = posterior.state
    if F != posterior.b.shape[0]:
        raise ValueError(f"f_star has {F} features, the posterior {posterior.b.shape[0]}")
    _on_device(f_star, "f_star")
    if f_star.device != state.device:
        raise ValueError("f_star and the posterior are on different devices")
    f_star = f_star.detach().contiguous()
    with torch.cuda.device(f_star.device):
        out = torch.empty((2, M), dtype=torch.float64, device=f_star.device)
        _hip.check(_hip.lib().sgmcmc_raob_predict(f_star.data_ptr(), _is_f64(f_star), M, F, state.data_ptr(),
                                                  out[0].data_ptr(), out[1].data_ptr(), _stream()), "sgmcmc_raob_predict")
    return out[0], out[1]
