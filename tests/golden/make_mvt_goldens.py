"""Golden vectors for the multivariate Student-t prior and the decreasing-tails googleresnet (reference:
prior/distributions.py:115-199, prior/multivariate_t.py, models/mvt_resnets.py:51-109, exp_utils.py:194-200) -- generated
by IMPORTING THE REFERENCE.  Build container only:

    python tests/golden/make_mvt_goldens.py     ->  tests/golden/mvt.npz

Shims that let the reference run on this image's torch, as in make_correlated_model_goldens.py: ``torch.cholesky`` points
at ``torch.linalg.cholesky``; ``ConvCorrelatedNormal`` and ``MultivariateT`` get a one-element location expanded to one
value PER POSITION when the factor is P x P (torch >= 2's MultivariateNormal does not broadcast it: its event would be one
element); and the reference's ``distributions.MultivariateT`` drops ``df`` from ``arg_constraints`` (torch >= 2 validates
them inside MultivariateNormal.__init__, before the subclass has set ``df``, and raises AttributeError).

Stored, float64:
  (a) ``dist|...``: the event-shape cases of the reference's testing/test_priors.py (TestMultivariateT.test_density): the
      inputs and ``distributions.MultivariateT.log_prob`` for event shapes [D], [M, D], [N, M, D] and the whole tensor;
  (b) ``prior|<case>|...``: ``prior.MultivariateT`` for five geometries (config JSON, loc, scale_tril), its log_prob and
      gradient at theta = numpy default_rng(seed).standard_normal(shape) * theta_scale;
  (c) ``model|<weight_prior>|...``: decreasing_mvt_googleresnet's parameter names, shapes, state_dict keys and, per
      parameter, the prior's class name and df (NaN when it has none), for weight_prior gaussian and convcorrnormal;
  (d) ``model|<weight_prior>|log_prior``: the model-level log-prior (models/base.py:57-62) at theta regenerated from
      MODEL_SEED (every parameter, in order, standard normal * 0.1), for both; for gaussian also its gradient w.r.t. the
      10 multivariate-t tensors (``model|gaussian|grad:<name>``).
"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

ref_stubs.install()
if not hasattr(torch, "cholesky"):
    torch.cholesky = torch.linalg.cholesky
if not hasattr(torch.Tensor, "cholesky"):
    torch.Tensor.cholesky = lambda self: torch.linalg.cholesky(self)
from bnn_priors import prior as RP  # noqa: E402
from bnn_priors import models as RM  # noqa: E402
from bnn_priors.exp_utils import DummyModule  # noqa: E402
from bnn_priors.prior import distributions as RD  # noqa: E402

RD.MultivariateT.arg_constraints = {k: v for k, v in RD.MultivariateT.arg_constraints.items() if k != "df"}

_ccn_init = RP.ConvCorrelatedNormal.__init__


def _ccn_per_position(self, shape, loc, scale, **kw):
    if isinstance(loc, float) or len(torch.as_tensor(loc).shape) == 0:
        loc = torch.zeros(shape[-2] * shape[-1]) + float(loc)
    _ccn_init(self, shape, loc, scale, **kw)


RP.ConvCorrelatedNormal.__init__ = _ccn_per_position
_mvt_init = RP.MultivariateT.__init__


def _mvt_per_position(self, shape, loc, scale_tril, *a, **kw):
    if isinstance(scale_tril, torch.Tensor) and scale_tril.dim() == 2 and scale_tril.shape[-1] > 1 \
            and isinstance(loc, torch.Tensor) and loc.numel() == 1:
        loc = loc.reshape(-1).expand(scale_tril.shape[-1]).clone()
    _mvt_init(self, shape, loc, scale_tril, *a, **kw)


RP.MultivariateT.__init__ = _mvt_per_position


def _factor(P, seed):
    "a well-conditioned lower-triangular P x P factor with a positive diagonal"
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((P, P)) * 0.3
    return np.linalg.cholesky(a @ a.T + 0.5 * np.eye(P))


def _se_factor(scale, lengthscale):
    pts = np.mgrid[:3, :3].reshape(2, -1).T
    d = np.sum((pts[:, None, :] - pts[None, :, :]) ** 2.0, 2) ** 0.5
    return np.linalg.cholesky(np.exp(-d / lengthscale)) * scale


# name -> shape, loc, scale_tril (None: the scalar `scale`), scale, df, event_dim, permute, theta seed, theta scale
PRIOR_CASES = {
    "perm3x3_full": dict(shape=[32, 16, 3, 3], loc=list(np.linspace(-0.05, 0.05, 9)), factor="se", scale=0.25, df=3.55,
                         event_dim=3, permute=[1, 0, 2, 3], seed=1, theta_scale=0.3),          # 4608 > 4096 elements
    "perm3x3_scalar": dict(shape=[16, 3, 3, 3], loc=0.1, factor=None, scale=0.4, df=3.0, event_dim=3,
                           permute=[1, 0, 2, 3], seed=2, theta_scale=0.5),
    "perm1x1": dict(shape=[32, 16, 1, 1], loc=0.0, factor=None, scale=0.3, df=32.0, event_dim=3, permute=[1, 0, 2, 3],
                    seed=3, theta_scale=0.2),
    "dense_ed2": dict(shape=[6, 4, 9], loc=list(np.linspace(0.1, -0.1, 9)), factor="random", scale=1.0, df=5.5,
                      event_dim=2, permute=None, seed=4, theta_scale=0.7),
    "dense_ed1": dict(shape=[80, 64], loc=-0.02, factor=None, scale=0.2, df=4.0, event_dim=1, permute=None, seed=5,
                      theta_scale=0.25),                                                        # 5120 > 4096 elements
}
MODEL_SEED = 17


def prior_args(case):
    "(loc, scale_tril) as the prior's constructor takes them (numbers, or float64 tensors)"
    if case["factor"] is None:
        return case["loc"], case["scale"]
    L = _se_factor(case["scale"], 0.7) if case["factor"] == "se" else _factor(9, 99) * case["scale"]
    return torch.tensor(case["loc"], dtype=torch.float64), torch.from_numpy(L)


def theta(case):
    return np.random.default_rng(case["seed"]).standard_normal(case["shape"]) * case["theta_scale"]


def _dist_cases(out):
    torch.manual_seed(100)
    N, D, M = 4, 6, 5
    cov = torch.randn(N, M, D, D)
    cov = cov @ cov.transpose(-1, -2)
    mean = torch.arange(D).to(cov)
    df = torch.arange(3, 3 + N)[:, None].to(cov)
    x = torch.randn(2, *cov.shape[:-1])
    out["dist|cov"], out["dist|mean"], out["dist|df"], out["dist|x"] = (t.numpy().copy() for t in (cov, mean, df, x))
    MVT = RD.MultivariateT
    out["dist|log_prob:D"] = MVT(torch.Size([D]), df, mean, cov).log_prob(x).numpy().copy()
    out["dist|log_prob:MD"] = MVT(torch.Size([M, D]), df.squeeze(-1), mean, cov).log_prob(x).numpy().copy()
    out["dist|log_prob:NMD"] = MVT(torch.Size([N, M, D]), df[0], mean, cov).log_prob(x).numpy().copy()
    out["dist|log_prob:all"] = MVT(x.size(), df[0], mean, cov).log_prob(x).numpy().copy()


def _prior_cases(out):
    for name, case in PRIOR_CASES.items():
        torch.manual_seed(0)
        loc, scale_tril = prior_args(case)
        pr = RP.MultivariateT(case["shape"], loc, scale_tril, df=case["df"], event_dim=case["event_dim"],
                              permute=case["permute"])
        with torch.no_grad():
            pr.p.copy_(torch.from_numpy(theta(case)))
        lp = pr.log_prob()
        lp.backward()
        key = "prior|" + name + "|"
        out[key + "config"] = np.array(json.dumps(case, sort_keys=True))
        out[key + "scale_tril"] = np.asarray(scale_tril, dtype=np.float64).reshape(
            (1, 1) if case["factor"] is None else (9, 9))
        out[key + "log_prob"] = np.float64(float(lp.detach()))
        out[key + "grad"] = pr.p.grad.numpy().copy()
        out[key + "state_keys"] = np.array(json.dumps(list(pr.state_dict().keys())))


def _model(weight_prior):
    prior_w = {"gaussian": RP.Normal, "convcorrnormal": RP.ConvCorrelatedNormal}[weight_prior]
    torch.manual_seed(0)
    net = RM.DecreasingMVTGoogleResNet(prior_w=prior_w, loc_w=0., std_w=2 ** .5, depth=20, prior_b=RP.Normal, loc_b=0.,
                                       std_b=1., scaling_fn=lambda std, dim: std / dim ** 0.5, bn=True, softmax_temp=1.,
                                       weight_prior_params={}, bias_prior_params={})
    inner = net.net                       # the CPU wrapper at the end of exp_utils.get_model
    del net.net
    net.net = DummyModule(inner)
    return net


def _model_cases(out):
    for wp in ("gaussian", "convcorrnormal"):
        net = _model(wp)
        key = "model|" + wp + "|"
        names = [n for n, _ in net.named_parameters()]
        out[key + "names"] = np.array(json.dumps(names))
        out[key + "shapes"] = np.array(json.dumps([list(p.shape) for _, p in net.named_parameters()]))
        out[key + "state_keys"] = np.array(json.dumps(list(net.state_dict().keys())))
        kinds, dfs = [], []
        mods = dict(net.named_modules())
        for n in names:
            m = mods.get(n[:-2]) if n.endswith(".p") else None
            kinds.append(type(m).__name__ if m is not None else "")
            dfs.append(float(m.df) if isinstance(m, RP.MultivariateT) else math.nan)
        out[key + "prior_types"] = np.array(json.dumps(kinds))
        out[key + "df"] = np.array(dfs, dtype=np.float64)
        rng = np.random.default_rng(MODEL_SEED)
        with torch.no_grad():
            for _, p in net.named_parameters():
                p.copy_(torch.from_numpy(rng.standard_normal(p.shape) * 0.1))
        lp = net.log_prior()
        lp.backward()
        out[key + "log_prior"] = np.float64(float(lp.detach()))
        if wp == "gaussian":
            for n, p in net.named_parameters():
                if isinstance(mods.get(n[:-2]), RP.MultivariateT):
                    out[key + "grad:" + n] = p.grad.numpy().copy()


def main(path=os.path.join(HERE, "mvt.npz")):
    out = {}
    torch.set_default_dtype(torch.float64)
    _dist_cases(out)
    _prior_cases(out)
    _model_cases(out)
    out["model|seed"] = np.int64(MODEL_SEED)
    torch.set_default_dtype(torch.float32)
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays")


if __name__ == "__main__":
    main(*sys.argv[1:])
