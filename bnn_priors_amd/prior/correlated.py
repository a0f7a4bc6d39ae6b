"""Multivariate priors over a convolution filter's spatial positions (the last two dimensions of the weight).  None is an
element-wise family of the HIP hook, but each one with FIXED arguments is a constant linear
whitening of the filter's ``P = kh * kw`` positions followed by an element-wise base density: ``fused_filter_spec()``
hands that whitening (computed in float64) to the hook's SGMCMC_PRIOR_FILTER_WHITENED kind.  A learnable scale or
lengthscale (``ConvCorrNormalGamma``, ``convcorrnormal_empirical``) keeps the prior in autograd (``Potential.leftover``).

* ``ConvCorrelatedNormal``: a zero-mean-shifted Gaussian over the ``kh x kw`` positions with a squared-exponential
  covariance ``scale^2 exp(-d / lengthscale)`` of their Euclidean distances, independent across channels (reference:
  bnn_priors/prior/loc_scale.py:13-63); ``ConvCorrNormalGamma``: Gamma hyper-priors on scale and lengthscale
  (prior/hierarchical.py:32-39).
* ``FixedCovNormal`` / ``FixedCovLaplace`` / ``FixedCovDoubleGamma`` / ``FixedCovGenNorm``: an element-wise base density
  pushed through the PCA transform of a given covariance of the positions (prior/conv_loc_scale.py:16-140).
The reference calls ``torch.cholesky`` / ``torch.symeig``, which this image's torch no longer has; ``torch.linalg.cholesky``
and ``torch.linalg.eigh`` compute the same factors.
"""
import math
from numbers import Number

import numpy as np
import torch
import torch.distributions as td
from torch import nn

from .. import _hip
from .base import Prior
from .distributions import DoubleGamma, GeneralizedNormal

__all__ = ("ConvCorrelatedNormal", "ConvCorrNormalGamma", "ConvCovariance", "FixedCovNormal", "FixedCovLaplace",
           "FixedCovDoubleGamma", "FixedCovGenNorm")


_LOG_2PI = float(np.log(2.0 * np.pi))


def _fixed(v):
    "a number or a plain tensor (not learnable, not a hyper-prior): its value in float64, else None"
    if isinstance(v, Number):
        return torch.tensor(float(v), dtype=torch.float64)
    if isinstance(v, (Prior, nn.Parameter)) or not isinstance(v, torch.Tensor) or v.requires_grad:
        return None
    return v.detach().to("cpu", torch.float64)


def _filter_positions(prior):
    "P when ``p`` is a contiguous [..., kh, kw] tensor whose filters the hook can take, else None"
    p = prior.p
    if p.dim() < 2 or not p.is_contiguous():
        return None
    P = p.shape[-2] * p.shape[-1]
    return P if 1 <= P <= _hip.FILTER_MAX_P else None


def _locations(loc, P):
    loc = _fixed(loc)
    if loc is None or loc.numel() not in (1, P):
        return None
    return loc.reshape(-1).expand(P).numpy().copy()


class SquaredExponentialNormal(td.MultivariateNormal):
    def __init__(self, loc, scale, distance_matrix, lengthscale):
        cov = torch.exp(-distance_matrix / lengthscale) * scale ** 2.0
        super().__init__(loc=loc, scale_tril=torch.linalg.cholesky(cov))


class ConvCorrelatedNormal(Prior):
    _dist = SquaredExponentialNormal
    fused_kind = None

    def __init__(self, shape, loc, scale, *, lengthscale=1.0):
        # One location per spatial position.  The reference hands MultivariateNormal a ONE-element loc for a scalar
        # (loc_scale.py:41-43) and relies on its being broadcast against the covariance -- which torch >= 2 no longer does
        # (sampling and log_prob fail there with a shape error): the scalar is expanded here, the density is the same.
        loc = torch.as_tensor(loc, dtype=torch.get_default_dtype())
        if loc.dim() == 0 or loc.shape[-1] == 1:
            loc = loc.reshape(-1)[:1].expand(shape[-2] * shape[-1]).clone()
        pts = np.mgrid[:shape[-2], :shape[-1]].reshape(2, -1).T
        d = np.sum((pts[:, None, :] - pts[None, :, :]) ** 2.0, 2) ** 0.5
        super().__init__(shape, loc=loc, scale=scale, distance_matrix=d, lengthscale=lengthscale)

    def log_prob(self):
        return self._dist_obj().log_prob(self.p.reshape(self.p.shape[:-2] + (-1,))).sum()

    def _draw(self, shape):
        return torch.reshape(self._dist_obj().sample(sample_shape=shape[:-2]), shape)

    def fused_filter_spec(self):
        "z = (theta_f - mu) L^-T with Sigma = L L^T = scale^2 exp(-d / lengthscale); standard normal base"
        P = _filter_positions(self)
        scale, ls, d = _fixed(self.scale), _fixed(self.lengthscale), _fixed(self.distance_matrix)
        if P is None or scale is None or ls is None or d is None or scale.numel() != 1 or ls.numel() != 1:
            return None
        mu = _locations(self.loc, P)
        if mu is None or d.shape != (P, P):
            return None
        chol = torch.linalg.cholesky(torch.exp(-d / ls) * scale ** 2)
        W = torch.linalg.inv(chol).T
        lognorm = -0.5 * P * _LOG_2PI - float(torch.log(torch.diagonal(chol)).sum())
        return dict(kind=_hip.PRIOR_FILTER_WHITENED, P=P, base=_hip.FILTER_BASE_NORMAL, beta=2.0, base_scale=1.0, lognorm=lognorm,
                    mu=mu, W=W.numpy().copy())


class ConvCorrNormalGamma(ConvCorrelatedNormal):
    def __init__(self, shape, loc, scale, lengthscale=1., rate=1.):
        from .hierarchical import _gamma_scale
        super().__init__(shape, loc, scale=_gamma_scale(scale, rate), lengthscale=_gamma_scale(lengthscale, rate))


class _Whitening(td.Transform):
    "x -> x A + m on the flattened last two dimensions (A = the covariance's PCA factor); its log-determinant is constant"
    domain = td.constraints.real
    codomain = td.constraints.real
    event_dim = 2
    bijective = True

    def __init__(self, shift, factor, inverse_factor, log_det):
        super().__init__(cache_size=0)
        self.shift, self.factor, self.inverse_factor, self.log_det = shift, factor, inverse_factor, log_det

    def _flat(self, t):
        return t.view(t.shape[:-2] + (-1,))

    def _call(self, x):
        return (self._flat(x) @ self.factor + self.shift).view(x.shape)

    def _inverse(self, y):
        return ((self._flat(y) - self.shift) @ self.inverse_factor).view(y.shape)

    def log_abs_det_jacobian(self, x, y):
        return self.log_det


def _pca_factors(cov):
    "(A, A^-1, log det A) with A = diag(sqrt(lambda)) V^T of cov = V diag(lambda) V^T, computed in float64"
    lam, vec = torch.linalg.eigh(cov.to(torch.float64))
    root = lam.sqrt()
    return root.unsqueeze(-1) * vec.t(), vec / root, lam.log().sum().view((1, 1)) / 2


class ConvCovariance(Prior):
    """base of the fixed-covariance priors: an element-wise base density (``_base``) pushed through the whitening
    transform of a given covariance of the filter positions; the factors are buffers (``scale``, ``inv_scale``,
    ``log_sqrt_vals``: the reference's names, prior/conv_loc_scale.py:46-70).  A NUMBER as ``cov`` is a standard deviation."""
    fused_kind = None

    def __init__(self, shape, loc, cov, **kwargs):
        n_pos = shape[-2] * shape[-1]
        if isinstance(cov, Number) or len(cov.shape) == 0:
            cov, loc = torch.eye(n_pos) * cov ** 2, torch.zeros(n_pos) + loc
        dt = torch.get_default_dtype()
        factor, inverse, log_det = (t.to(dt) for t in _pca_factors(cov))
        super().__init__(shape, loc=loc, scale=factor, inv_scale=inverse, log_sqrt_vals=log_det, event_shape=shape[-2:],
                         **kwargs)

    def _base(self, zeros, **extra):
        raise NotImplementedError

    def _dist(self, loc, scale, inv_scale, log_sqrt_vals, event_shape, **extra):
        zeros = torch.zeros((), device=loc.device, dtype=loc.dtype).expand(event_shape)
        return td.TransformedDistribution(self._base(zeros, **extra), _Whitening(loc, scale, inv_scale, log_sqrt_vals))

    def assign_cov(self, cov):
        for buf, new in zip((self.scale, self.inv_scale, self.log_sqrt_vals), _pca_factors(cov)):
            buf.copy_(new)
        self.refresh_fused_filter()        # samplers that evaluate this prior in the HIP hook follow

    def _base_spec(self, P):
        "(base kind, beta, base_scale, the base density's log-normaliser over P positions) or None"
        raise NotImplementedError

    def fused_filter_spec(self):
        """z = (theta_f - loc) inv_scale, the base density element-wise, minus log |det scale| = log_sqrt_vals ONCE PER
        POSITION: the transformed distribution subtracts the (1, 1) log-determinant of ``_Whitening`` from every
        element's base log-density, as the reference's (prior/conv_loc_scale.py) does -- the fixtures hold that value"""
        P = _filter_positions(self)
        W, lsv = _fixed(self.inv_scale), _fixed(self.log_sqrt_vals)
        if P is None or W is None or lsv is None or W.shape != (P, P) or lsv.numel() != 1:
            return None
        mu, base = _locations(self.loc, P), self._base_spec(P)
        if mu is None or base is None:
            return None
        kind, beta, base_scale, base_norm = base
        return dict(kind=_hip.PRIOR_FILTER_WHITENED, P=P, base=kind, beta=beta, base_scale=base_scale,
                    lognorm=base_norm - P * float(lsv), mu=mu, W=W.numpy().copy())


class FixedCovNormal(ConvCovariance):
    def __init__(self, shape, loc, cov):
        super().__init__(shape, loc, cov)

    def _base(self, zeros):
        return td.Normal(zeros, zeros + 1)

    def _base_spec(self, P):
        return _hip.FILTER_BASE_NORMAL, 2.0, 1.0, -0.5 * P * _LOG_2PI


class FixedCovLaplace(ConvCovariance):
    "Laplace base of scale ``base_scale`` (the default sqrt(1/2) gives it unit variance)"

    def __init__(self, shape, loc, cov, base_scale=math.sqrt(1 / 2)):
        super().__init__(shape, loc, cov, base_scale=base_scale)

    def _base(self, zeros, base_scale):
        return td.Laplace(loc=zeros, scale=base_scale.expand(zeros.shape))

    def _base_spec(self, P):
        s = _fixed(self.base_scale)
        if s is None or s.numel() != 1:
            return None
        s = float(s)
        # td.Laplace: log p(z) = -log(2 s) - |z| / s
        return _hip.FILTER_BASE_LAPLACE, 1.0, s, -P * np.log(2.0 * s)


class FixedCovDoubleGamma(ConvCovariance):
    """double-Gamma base ``DoubleGamma(concentration, base_rate)``: |z| ~ Gamma(c, rate), a random sign.  Without
    ``base_scale`` the rate is sqrt(c (1 + c)), which gives the base unit variance; else it is 1 / base_scale.

    In the HIP hook the base's gradient is 0 at z == 0 (autograd gives NaN there) and its log term (c - 1) log|z| follows
    torch's xlogy: 0 when c == 1, +-inf otherwise."""

    def __init__(self, shape, loc, cov, concentration, base_scale=None):
        if base_scale is None:
            base_rate = (concentration * (1 + concentration)) ** .5
        else:
            base_rate = 1. / base_scale
        super().__init__(shape, loc, cov, concentration=concentration, base_rate=base_rate)

    def _base(self, zeros, concentration, base_rate):
        shape = zeros.shape
        return DoubleGamma(concentration.expand(shape), rate=base_rate.expand(shape))

    def _base_spec(self, P):
        c, r = _fixed(self.concentration), _fixed(self.base_rate)
        if c is None or r is None or c.numel() != 1 or r.numel() != 1:
            return None
        c, r = float(c), float(r)
        # DoubleGamma: log p(z) = c log r - lgamma(c) - log 2 + (c - 1) log|z| - r |z|  (prior/distributions.py); the
        # record's beta is c and its base_scale 1 / r
        return _hip.FILTER_BASE_DOUBLE_GAMMA, c, 1.0 / r, P * (c * np.log(r) - math.lgamma(c) - np.log(2.0))


class FixedCovGenNorm(ConvCovariance):
    "(the reference notes that sampling is slightly off -- the CDF's accuracy -- and irrelevant for inference)"

    def __init__(self, shape, loc, cov, beta, base_scale=None):
        if isinstance(beta, Number):
            beta = torch.tensor(beta, dtype=torch.float64)        # (stored in double, as the reference stores it)
        if base_scale is None:        # the scale that gives the base density unit variance
            base_scale = ((torch.lgamma(1 / beta) - torch.lgamma(3 / beta)) / 2).exp()
        super().__init__(shape, loc, cov, beta=beta, base_scale=torch.as_tensor(base_scale).to(torch.get_default_dtype()))

    def _base(self, zeros, beta, base_scale):
        shape = zeros.shape
        return GeneralizedNormal(loc=zeros, scale=base_scale.expand(shape), beta=beta.expand(shape))

    def _base_spec(self, P):
        beta, s = _fixed(self.beta), _fixed(self.base_scale)
        if beta is None or s is None or beta.numel() != 1 or s.numel() != 1:
            return None
        beta, s = float(beta), float(s)
        # GeneralizedNormal: log p(z) = log beta - log(2 s) - lgamma(1 / beta) - |z / s|^beta  (prior/distributions.py)
        return _hip.FILTER_BASE_GENNORM, beta, s, P * (np.log(beta) - np.log(2.0 * s) - math.lgamma(1.0 / beta))
