"""The multivariate Student-t prior (reference: bnn_priors/prior/multivariate_t.py): a tensor's elements, optionally
permuted, are split into independent EVENTS of its trailing ``event_dim`` dimensions; one event is a set of vectors of the
size of ``scale_tril`` that share one Gamma mixing variable (``distributions.MultivariateT``).  The decreasing-tails
googleresnet (models/nets.py) uses it with ``permute = (1, 0, 2, 3)``, ``event_dim = 3``: one event per INPUT channel of
a convolution weight, spanning all its output channels' filters.

With fixed ``loc``, ``scale_tril`` and ``df`` the HIP prior hook evaluates it as SGMCMC_PRIOR_MULTIVARIATE_T
(include/sgmcmc_hip.h): ``fused_mvt_spec()`` hands over the whitening ``W = L^-T`` of the ``P`` positions, the event
geometry and the event's log-normaliser, computed in float64.  A learnable argument keeps the prior in autograd.

One divergence: a NUMBER ``loc`` with a ``P x P`` ``scale_tril`` becomes one location per position.  The reference hands
MultivariateNormal a one-element location there, which torch >= 2 no longer broadcasts against the factor (its event would
be one element and ``log_prob`` fails); the density is the one the reference intends, as for ``ConvCorrelatedNormal``.
"""
import math
from numbers import Number

import numpy as np
import torch

from .. import _hip
from .base import Prior
from .correlated import _fixed
from . import distributions

__all__ = ("MultivariateT",)


class MultivariateT(Prior):
    fused_kind = None

    def __init__(self, shape, loc, scale_tril, df=3, event_dim=None, permute=None):
        shape = torch.Size(shape)
        if event_dim is None:
            event_dim = len(shape)
        permute = tuple(range(len(shape))) if permute is None else tuple(int(i) for i in permute)
        if sorted(permute) != list(range(len(shape))):
            raise ValueError(f"permute {permute} is not a permutation of the {len(shape)} dimensions")
        if not 1 <= event_dim <= len(shape):
            raise ValueError(f"event_dim must be in [1, {len(shape)}], not {event_dim}")
        permuted = torch.Size([shape[i] for i in permute])
        out_event_shape = permuted[len(permuted) - event_dim:]
        batch_shape = permuted[:len(permuted) - event_dim]
        dt = torch.get_default_dtype()
        if isinstance(scale_tril, Number) or isinstance(loc, Number):
            scale_tril = torch.ones([1, 1], dtype=dt) * scale_tril
            loc = torch.zeros([1], dtype=dt) + loc
        loc = torch.as_tensor(loc, dtype=dt) if not isinstance(loc, torch.Tensor) else loc
        if loc.dim() == 0:
            loc = loc.reshape(1)
        P = scale_tril.shape[-1]
        if loc.shape[-1] == 1 and P > 1:        # one location per position (see the module's docstring)
            loc = loc.expand(loc.shape[:-1] + (P,)).clone()
        # the Gaussian's event size after broadcasting loc against scale_tril
        size = torch.distributions.MultivariateNormal(loc.detach(), scale_tril=scale_tril.detach()).event_shape[-1]
        if size == 1:
            event_shape = out_event_shape if out_event_shape[-1] == 1 else torch.Size([*out_event_shape, 1])
        else:
            # the trailing dimensions of the event whose product is the Gaussian's size form its vectors
            prod, split = 1, None
            for i in range(len(out_event_shape) - 1, -1, -1):
                prod *= out_event_shape[i]
                if prod == size:
                    split = i
                    break
            if split is None:
                raise ValueError(f"no trailing dimensions of the event {tuple(out_event_shape)} hold {size} elements")
            event_shape = torch.Size([*out_event_shape[:split], size])
        super().__init__(shape, loc=loc, scale_tril=scale_tril, df=df, event_shape=event_shape,
                         out_event_shape=out_event_shape, permute=permute, batch_shape=batch_shape)

    def _dist(self, loc, scale_tril, df, event_shape, **_kwargs):
        return distributions.MultivariateT(event_shape, df=df, loc=loc, scale_tril=scale_tril)

    def _draw(self, shape):
        x = self._dist_obj().sample(sample_shape=self.batch_shape)
        inverse = tuple(int(i) for i in np.argsort(self.permute))
        # (contiguous: the tensor goes into an nn.Parameter)
        return x.reshape(self.batch_shape + self.out_event_shape).permute(*inverse).contiguous()

    def log_prob(self):
        p = self.p.permute(*self.permute).reshape(self.batch_shape + self.event_shape)
        return self._dist_obj().log_prob(p).sum()

    def event_geometry(self):
        """(ev_div, ev_mod) such that element j of the contiguous tensor belongs to event (j / ev_div) % ev_mod, or None
        for a geometry the HIP hook does not take: unpermuted trailing events, or (1, 0, 2, 3) with event_dim = 3 (one
        event per input channel of a convolution weight)"""
        shape, D = self.p.shape, self.out_event_shape.numel()
        if self.permute == tuple(range(len(shape))):
            return D, shape.numel() // D
        if len(shape) == 4 and self.permute == (1, 0, 2, 3) and len(self.out_event_shape) == 3:
            return shape[2] * shape[3], shape[1]
        return None

    def fused_mvt_spec(self):
        """The table of SGMCMC_PRIOR_MULTIVARIATE_T in float64: ``P``, ``mu`` [P], ``W = L^-T`` [P, P], ``df``, ``ev_size``
        (D), ``ev_div``, ``ev_mod`` and ``lognorm`` (the event's log-normaliser) such that an event's log-density is
        ``lognorm - (df + D)/2 log(1 + M / (df - 2))`` with ``M = sum_f |(theta_f - mu) W|^2`` over its filters of P
        consecutive elements.  None when an argument is learnable or batched, or the geometry is not the hook's."""
        loc, L, df = _fixed(self.loc), _fixed(self.scale_tril), _fixed(self.df)
        if loc is None or L is None or df is None or df.numel() != 1 or L.dim() != 2 or not self.p.is_contiguous():
            return None
        P = L.shape[-1]
        if not 1 <= P <= _hip.FILTER_MAX_P or loc.numel() not in (1, P):
            return None
        geo = self.event_geometry()
        D = self.out_event_shape.numel()
        if geo is None or geo[0] % P or D % P or self.p.numel() % (geo[0] * geo[1]):
            return None
        df = float(df)
        lam = df - 2.0
        half_log_det = (D / P) * float(torch.log(torch.diagonal(L)).sum())
        lognorm = (math.lgamma((D + df) / 2.0) - math.lgamma(df / 2.0) - (D / 2.0) * math.log(math.pi * lam)
                   - half_log_det)
        W = torch.linalg.inv(L).T
        return dict(kind=_hip.PRIOR_MULTIVARIATE_T, P=P, mu=loc.reshape(-1).expand(P).numpy().copy(), W=W.numpy().copy(),
                    df=df, ev_size=D, ev_div=int(geo[0]), ev_mod=int(geo[1]), lognorm=lognorm)
