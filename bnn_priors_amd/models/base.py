"""Potential-energy interface of a BNN: what the samplers differentiate.

Mirrors ``bnn_priors/models/base.py:14-136,168-191`` of the reference
(``AbstractModel.log_prior / log_likelihood / potential_avg /
split_potential_and_acc``, ``ClassificationModel``, ``RegressionModel``).
The Rao-Blackwellised model (:194-311) is out of scope.

    potential_avg(x, y, N) = -(1/B) sum_i log p(y_i | x_i, theta) - log p(theta) / N
"""
from collections import OrderedDict

import torch
from torch import nn

from .. import prior
from .. import raob as _raob

__all__ = ("AbstractModel", "ClassificationModel", "RegressionModel", "RaoBRegressionModel")


class AbstractModel(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    # -- densities -------------------------------------------------------------
    def log_prior(self):
        total = sum(pr.log_prob() for _, pr in prior.named_priors(self))
        return torch.tensor(total) if isinstance(total, float) else total

    def likelihood_dist(self, f):
        raise NotImplementedError

    def forward(self, x):
        return self.likelihood_dist(self.net(x))

    def _log_likelihood_preds(self, x, y, eff_num_data):
        assert x.shape[0] == y.shape[0]
        preds = self(x)
        return preds.log_prob(y).sum() * (eff_num_data / x.shape[0]), preds

    def log_likelihood(self, x, y, eff_num_data):
        return self._log_likelihood_preds(x, y, eff_num_data)[0]

    def log_likelihood_avg(self, x, y):
        return self._log_likelihood_preds(x, y, 1)[0]

    # -- potentials ------------------------------------------------------------
    def potential(self, x, y, eff_num_data):
        return -(self.log_likelihood(x, y, eff_num_data) + self.log_prior())

    def potential_avg(self, x, y, eff_num_data):
        return -(self.log_likelihood_avg(x, y) + self.log_prior() / eff_num_data)

    def _split_potential_preds(self, x, y, eff_num_data):
        lla, preds = self._log_likelihood_preds(x, y, 1)
        log_prior = self.log_prior()
        return -lla, log_prior, -lla - log_prior / eff_num_data, preds

    def split_potential_and_acc(self, x, y, eff_num_data):
        raise NotImplementedError

    def params_dict(self):
        return OrderedDict((n, p.detach()) for n, p in self.named_parameters())

    def sample_all_priors(self):
        for _, pr in prior.named_priors(self):
            pr.sample()


class RegressionModel(AbstractModel):
    "independent Gaussian likelihood with std ``noise_std`` (reference :139-165)"

    def __init__(self, net, noise_std):
        super().__init__(net)
        self.noise_std = noise_std

    def likelihood_dist(self, f):
        return torch.distributions.Normal(f, prior.value_or_call(self.noise_std))

    def acc_mse(self, preds, y):
        d = preds.mean - y
        return (d * d).sum(-1)

    def split_potential_and_acc(self, x, y, eff_num_data):
        loss, log_prior, pot, preds = self._split_potential_preds(x, y, eff_num_data)
        return loss, log_prior, pot, self.acc_mse(preds, y), preds


class ClassificationModel(AbstractModel):
    "categorical likelihood on ``net(x) / softmax_temp`` (reference :168-191)"

    def __init__(self, net, softmax_temp=1.):
        super().__init__(net)
        self.softmax_temp = softmax_temp

    def likelihood_dist(self, f):
        return torch.distributions.Categorical(logits=f / prior.value_or_call(self.softmax_temp))

    def acc_mse(self, preds, y):
        return preds.logits.argmax(dim=1).eq(y).to(torch.float32)

    def split_potential_and_acc(self, x, y, eff_num_data):
        loss, log_prior, pot, preds = self._split_potential_preds(x, y, eff_num_data)
        return loss, log_prior, pot, self.acc_mse(preds, y), preds


def _same_tensor(a, b):
    "a and b are one tensor or two views of the same memory: decided on the host, without reading an element"
    return a is b or (a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and a.stride() == b.stride()
                      and a.data_ptr() == b.data_ptr())


class RaoBRegressionModel(RegressionModel):
    """Univariate Gaussian regression with the last layer integrated out (reference :194-311): ``net`` maps x to F
    features, the last layer's weights are iid Normal(0, ``last_layer_std``^2), and the model is conditioned on the
    training set it is built with.

    ``log_likelihood`` (hence ``potential``) is the marginal likelihood log N(y | 0, last_layer_std^2 f f^T + noise_std^2 I)
    of ``raob.marginal_log_likelihood``: two launches forward, one backward, no host synchronisation; ``eff_num_data`` is
    ignored, as in the reference.  ``posterior_w``, ``_posterior_w`` and ``forward`` / ``likelihood_dist`` read the state
    record of the same kernels when no gradient is required (under ``torch.no_grad()``, or with no input that requires
    one); when one is, they are a ``torch.linalg.cholesky_ex`` / ``solve_triangular`` restatement of :283-311 that
    autograd differentiates -- that path is NOT accelerated.

    A quirk of the reference that is kept: ``potential_avg`` and ``split_potential_and_acc`` go through ``self(x)``, the
    posterior PREDICTIVE at the rows of x, not through the marginal likelihood.  The accelerated sampling route is
    therefore a closure over ``potential``."""

    def __init__(self, x_train, y_train, noise_std, last_layer_std, net):
        assert x_train.dim() == 2
        assert x_train.size(0) == y_train.size(0)
        assert y_train.dim() == 2 and y_train.size(1) == 1
        super().__init__(net, noise_std)
        self.register_buffer("x_train", x_train)
        self.register_buffer("y_train", y_train)
        self.last_layer_std = last_layer_std

    def _noise_var(self):
        return prior.value_or_call(self.noise_std) ** 2

    def _check_training_set(self, x, y):
        # identity first: torch.equal reads the device, and this runs once per leapfrog step
        assert x is None or _same_tensor(x, self.x_train) or torch.equal(x, self.x_train)
        assert y is None or _same_tensor(y, self.y_train) or torch.equal(y, self.y_train)

    def log_likelihood(self, x, y, eff_num_data):
        self._check_training_set(x, y)
        return _raob.marginal_log_likelihood(self.net(self.x_train), self.y_train, self._noise_var(),
                                             self.last_layer_std ** 2)

    def _needs_grad(self, *tensors):
        return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)

    def _record(self, f, y, sig):
        return _raob.posterior(f, y, sig, self.last_layer_std ** 2)

    def _posterior_w(self, x, y):
        "mean and lower-triangular root of the precision of the whitened p(w | x, y), in fp64 (reference :283-293)"
        f, sig = self.net(x), self._noise_var()
        if not self._needs_grad(f, y, sig):
            rec = self._record(f, y, sig)
            root_v = rec.noise_var.sqrt()
            return (rec.L.t() @ rec.b.unsqueeze(1)) * (self.last_layer_std / root_v), rec.L / root_v
        f = f * self.last_layer_std
        A = (f.t() @ f) / sig + torch.eye(f.size(-1), dtype=f.dtype, device=f.device)
        L = torch.linalg.cholesky_ex(A.to(torch.float64)).L
        white_mean = torch.linalg.solve_triangular(L, (f.t() @ y).to(torch.float64), upper=False)
        return white_mean / sig, L

    def posterior_w(self):
        "mean [F, 1] and the root R [F, F] of the covariance, Cov = R^T R, of the whitened weights (reference :295-302)"
        f, sig = self.net(self.x_train), self._noise_var()
        if not self._needs_grad(f, sig):
            rec = self._record(f, self.y_train, sig)
            return rec.b.unsqueeze(1) * self.last_layer_std, rec.Linv * rec.noise_var.sqrt()
        white_w_mean, L_w = self._posterior_w(self.x_train, self.y_train)
        mean = torch.linalg.solve_triangular(L_w.t(), white_w_mean, upper=True)
        eye = torch.eye(L_w.size(-1), dtype=L_w.dtype, device=L_w.device)
        return mean, torch.linalg.solve_triangular(L_w, eye, upper=False)

    def likelihood_dist(self, f):
        "the posterior predictive Normal at the rows of f = net(x) (reference :304-311)"
        f_train, sig = self.net(self.x_train), self._noise_var()
        if not self._needs_grad(f, f_train, sig):
            mean, var = _raob.predictive(self._record(f_train, self.y_train, sig), f)
        else:
            white_w_mean, L_w = self._posterior_w(self.x_train, self.y_train)
            Lf = torch.linalg.solve_triangular(L_w, (f * self.last_layer_std).t().to(torch.float64), upper=False)
            mean = (Lf.t() @ white_w_mean).squeeze(-1)
            var = (Lf * Lf).sum(0) + sig
        return torch.distributions.Normal(mean.to(f).unsqueeze(-1), var.sqrt().to(f).unsqueeze(-1))
