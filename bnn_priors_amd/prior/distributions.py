"""Distributions the prior modules need beyond ``torch.distributions``.

``GeneralizedNormal(loc, scale, beta)``: density  beta / (2 scale Gamma(1/beta)) * exp(-(|x - loc| / scale)^beta)
(reference: bnn_priors/prior/distributions.py:15-98).  ``DoubleGamma(concentration, rate)``: a Gamma density on |x|,
halved, with a random sign when sampled (distributions.py:97-112).  ``MultivariateT(event_shape, df, loc, ...)``: the
multivariate Student-t in Shah et al.'s (2014) parameterisation, whose covariance is ``scale_tril scale_tril^T``
(distributions.py:115-199).  Sampling goes through ``scipy.stats.gennorm`` seeded from
torch's global generator, so a run under ``torch.manual_seed`` draws what the reference draws.
"""
import math

import torch
from torch.distributions import constraints
from torch.distributions.distribution import Distribution
from torch.distributions.utils import broadcast_all

__all__ = ("GeneralizedNormal", "DoubleGamma", "MultivariateT")


class GeneralizedNormal(Distribution):
    arg_constraints = {"loc": constraints.real, "scale": constraints.positive, "beta": constraints.positive}
    support = constraints.real
    has_rsample = False

    def __init__(self, loc, scale, beta, validate_args=None):
        self.loc, self.scale = broadcast_all(loc, scale)
        (self.beta,) = broadcast_all(beta)
        super().__init__(self.loc.size(), validate_args=validate_args)

    @property
    def mean(self):
        return self.loc

    @property
    def variance(self):
        return self.scale.pow(2) * (torch.lgamma(3 / self.beta) - torch.lgamma(1 / self.beta)).exp()

    def log_prob(self, value):
        if self._validate_args:
            self._validate_sample(value)
        z = (value - self.loc).abs() / self.scale
        return torch.log(self.beta) - torch.log(2 * self.scale) - torch.lgamma(1 / self.beta) - z.pow(self.beta)

    def entropy(self):
        return 1 / self.beta - torch.log(self.beta) + torch.log(2 * self.scale) + torch.lgamma(1 / self.beta)

    def sample(self, sample_shape=torch.Size()):
        from scipy import stats
        frozen = stats.gennorm(loc=self.loc.detach().cpu().numpy(), scale=self.scale.detach().cpu().numpy(),
                               beta=self.beta.detach().cpu().numpy())
        seed = torch.randint(2 ** 32, ()).item()     # one draw from torch's generator per call
        shape = list(torch.Size(sample_shape) + self.loc.size())
        return torch.tensor(frozen.rvs(shape, random_state=seed), dtype=self.loc.dtype, device=self.loc.device)


class DoubleGamma(torch.distributions.Gamma):
    "density Gamma(|x|; concentration, rate) / 2 on the real line"
    mean = 0.

    @property
    def variance(self):
        return self.concentration * (1 + self.concentration) / self.rate.pow(2)

    def rsample(self, sample_shape=torch.Size()):
        x = super().rsample(sample_shape)
        sign = torch.randint(0, 2, x.size(), device=x.device, dtype=x.dtype).mul_(2).sub_(1)
        return x * sign

    def log_prob(self, value):
        return super().log_prob(value.abs()) - math.log(2)


class MultivariateT(torch.distributions.MultivariateNormal):
    """Multivariate Student-t as a Gamma scale mixture of Gaussians (Shah et al. 2014, arXiv:1402.4306) with
    ``lambda = df - 2``: ``x = loc + sqrt(lambda / r) L eps``, ``r ~ Gamma(df / 2, rate 1 / 2)``, so that the covariance
    is ``L L^T`` itself; hence ``df > 2``.

    ``event_shape`` may extend the Gaussian's event ``[D0]`` to the left (``[..., D0]``): one event is then several
    vectors that share ONE mixing variable, and its log-density (with ``p`` the event's element count and ``M`` the sum
    of the vectors' Mahalanobis norms) is
    ``lgamma((p + df)/2) - lgamma(df/2) - (p/2) log(pi lambda) - half_log_det - ((df + p)/2) log(1 + M / lambda)``."""
    # (no entry for df: MultivariateNormal.__init__ validates these before df exists; df > 2 is checked below)
    arg_constraints = {"loc": constraints.real_vector,
                       "covariance_matrix": constraints.positive_definite,
                       "precision_matrix": constraints.positive_definite,
                       "scale_tril": constraints.lower_cholesky}
    support = constraints.real
    has_rsample = True
    expand = NotImplemented

    def __init__(self, event_shape, df=3., loc=0., covariance_matrix=None, precision_matrix=None, scale_tril=None,
                 validate_args=None):
        super().__init__(loc=loc, covariance_matrix=covariance_matrix, precision_matrix=precision_matrix,
                         scale_tril=scale_tril, validate_args=validate_args)
        event_shape, inner = torch.Size(event_shape), self._event_shape
        if len(event_shape) < len(inner):
            raise NotImplementedError("an event smaller than the Gaussian's (a non-elliptical t) is not supported")
        if len(event_shape) < 1 or event_shape[len(event_shape) - len(inner):] != inner:
            raise ValueError(f"event_shape {tuple(event_shape)} does not end in the Gaussian's event {tuple(inner)}")
        whole = self._batch_shape + self._event_shape
        self._batch_shape = whole[:max(0, len(whole) - len(event_shape))]     # (an event may cover the batch too)
        self._event_shape = event_shape
        df = torch.as_tensor(df, dtype=self.loc.dtype, device=self.loc.device)
        if bool((df <= 2).any()):
            raise ValueError("MultivariateT needs df > 2 (its covariance is undefined otherwise)")
        self.df = df.expand(torch.broadcast_shapes(df.shape, self._batch_shape))
        self.gamma = torch.distributions.Gamma(concentration=self.df / 2., rate=0.5)

    def rsample(self, sample_shape=torch.Size()):
        from torch.distributions.multivariate_normal import _batch_mv
        from torch.distributions.utils import _standard_normal
        shape = self._extended_shape(sample_shape)
        eps = _standard_normal(shape, dtype=self.loc.dtype, device=self.loc.device)
        r = self.gamma.rsample(sample_shape)                       # one mixing variable per event
        mix = ((self.df - 2.) / r).sqrt()
        mix = mix.reshape(mix.shape + (1,) * len(self._event_shape))
        return self.loc + mix * _batch_mv(self._unbroadcasted_scale_tril, eps)

    def log_prob(self, value):
        from torch.distributions.multivariate_normal import _batch_mahalanobis
        if self._validate_args:
            self._validate_sample(value)
        diff = value - self.loc
        maha = _batch_mahalanobis(self._unbroadcasted_scale_tril, diff)
        n_dim = len(self._event_shape)
        p = diff.shape[len(diff.shape) - n_dim:].numel()
        if n_dim > 1:
            maha = maha.sum(tuple(range(-n_dim + 1, 0)))
        log_diag = self._unbroadcasted_scale_tril.diagonal(dim1=-2, dim2=-1).log()
        if n_dim > log_diag.dim():          # every vector of the event has the same factor
            half_log_det = log_diag.sum() * (p / log_diag.numel())
        else:
            half_log_det = log_diag.sum(tuple(range(-n_dim, 0))) * (p / log_diag.shape[log_diag.dim() - n_dim:].numel())
        lam = self.df - 2.
        return (torch.lgamma((p + self.df) / 2.) - torch.lgamma(self.df / 2.) - (p / 2.) * torch.log(math.pi * lam)
                - half_log_det - ((self.df + p) / 2.) * torch.log1p(maha / lam))
