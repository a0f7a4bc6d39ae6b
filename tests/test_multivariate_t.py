"""The multivariate Student-t prior (prior/multivariate_t.py, prior/distributions.py) and its kind of the HIP prior hook
(SGMCMC_PRIOR_MULTIVARIATE_T, include/sgmcmc_hip.h).  CPU: the distribution and the prior against the reference's values
(tests/golden/make_mvt_goldens.py), the host table evaluated with the kernel's formula, the table's limits and the
sampling moments.  GPU: the two launches (per-event sums, then the gradient) against the fixtures across chunk boundaries
in both precisions, and run-to-run bit identity."""
import json
import math
import os

import numpy as np
import pytest
import torch

from bnn_priors_amd import _hip
from bnn_priors_amd import prior as P
from bnn_priors_amd.prior.distributions import MultivariateT as MVTDist
from prior_reference import whitened

CASES = ("perm3x3_full", "perm3x3_scalar", "perm1x1", "dense_ed2", "dense_ed1")


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "mvt.npz"))


def _case(z, name, dtype=torch.float64):
    "the fixture's prior at its theta (float64, then converted), and the case's config"
    cfg = json.loads(str(z["prior|" + name + "|config"]))
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        if cfg["factor"] is None:
            loc, scale_tril = cfg["loc"], cfg["scale"]
        else:
            loc, scale_tril = torch.tensor(cfg["loc"]), torch.from_numpy(z["prior|" + name + "|scale_tril"])
        pr = P.MultivariateT(cfg["shape"], loc, scale_tril, df=cfg["df"], event_dim=cfg["event_dim"],
                             permute=cfg["permute"])
        with torch.no_grad():
            pr.p.copy_(torch.from_numpy(np.random.default_rng(cfg["seed"]).standard_normal(cfg["shape"])
                                        * cfg["theta_scale"]))
    finally:
        torch.set_default_dtype(torch.float32)
    return pr.to(dtype), cfg


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_distribution_reproduces_the_reference_event_shapes(golden_dir):
    z = _fixture(golden_dir)
    cov, mean, df, x = (torch.from_numpy(z["dist|" + k]) for k in ("cov", "mean", "df", "x"))
    N, M, D = cov.shape[0], cov.shape[1], cov.shape[-1]
    got = {"D": MVTDist(torch.Size([D]), df, mean, cov).log_prob(x),
           "MD": MVTDist(torch.Size([M, D]), df.squeeze(-1), mean, cov).log_prob(x),
           "NMD": MVTDist(torch.Size([N, M, D]), df[0], mean, cov).log_prob(x),
           "all": MVTDist(x.size(), df[0], mean, cov).log_prob(x)}
    for k, v in got.items():
        np.testing.assert_allclose(v.numpy(), z["dist|log_prob:" + k], rtol=1e-12, err_msg=k)


def test_distribution_refuses_df_at_most_two():
    for df in (2.0, 1.5, torch.tensor([3.0, 2.0])):
        with pytest.raises(ValueError, match="df > 2"):
            MVTDist(torch.Size([3]), df, torch.zeros(3), scale_tril=torch.eye(3))
    with pytest.raises(ValueError, match="df > 2"):
        P.MultivariateT((4, 3), 0., 1., df=2.0)


@pytest.mark.parametrize("name", CASES)
def test_prior_reproduces_the_reference(golden_dir, name):
    z = _fixture(golden_dir)
    pr, _ = _case(z, name)
    assert list(pr.state_dict().keys()) == json.loads(str(z["prior|" + name + "|state_keys"]))
    lp = pr.log_prob()
    lp.backward()
    assert float(lp.detach()) == pytest.approx(float(z["prior|" + name + "|log_prob"]), rel=1e-12)
    np.testing.assert_allclose(pr.p.grad.numpy(), z["prior|" + name + "|grad"], rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("name", CASES)
def test_host_table_with_the_kernel_formula_reproduces_the_reference(golden_dir, name):
    z = _fixture(golden_dir)
    pr, cfg = _case(z, name)
    spec = pr.fused_mvt_spec()
    assert spec is not None
    assert spec["P"] == (1 if cfg["factor"] is None else 9)
    assert spec["ev_size"] * spec["ev_mod"] == pr.p.numel()
    lp, g, _ = whitened(spec, pr.p.detach().numpy())
    assert lp == pytest.approx(float(z["prior|" + name + "|log_prob"]), rel=1e-12)
    np.testing.assert_allclose(g, z["prior|" + name + "|grad"], rtol=1e-10, atol=1e-13)
    assert pr.fused_spec() is None and pr.fused_filter_spec() is None


def test_event_geometry():
    torch.manual_seed(0)
    conv = P.MultivariateT((8, 5, 3, 3), 0., 0.5, df=4., event_dim=3, permute=(1, 0, 2, 3))
    assert conv.fused_mvt_spec()["ev_div"] == 9 and conv.fused_mvt_spec()["ev_mod"] == 5
    assert conv.fused_mvt_spec()["ev_size"] == 72
    dense = P.MultivariateT((6, 4, 9), 0., torch.eye(9), df=4., event_dim=2)
    s = dense.fused_mvt_spec()
    assert (s["P"], s["ev_size"], s["ev_div"], s["ev_mod"]) == (9, 36, 36, 6)
    whole = P.MultivariateT((6, 4), 0., 0.3)                     # one event: the whole tensor
    s = whole.fused_mvt_spec()
    assert (s["ev_size"], s["ev_mod"]) == (24, 1)


def test_only_fixed_arguments_and_known_geometries_give_a_table():
    torch.manual_seed(0)
    shape = (8, 4, 3, 3)
    assert P.MultivariateT(shape, 0., 0.5, df=3., event_dim=3, permute=(1, 0, 2, 3)).fused_mvt_spec() is not None
    # other permutations / event dimensions of a permuted tensor stay in autograd
    assert P.MultivariateT(shape, 0., 0.5, df=3., event_dim=2, permute=(1, 0, 2, 3)).fused_mvt_spec() is None
    assert P.MultivariateT(shape, 0., 0.5, df=3., event_dim=3, permute=(0, 1, 3, 2)).fused_mvt_spec() is None
    # learnable arguments
    pr = P.MultivariateT(shape, 0., 0.5, df=3., event_dim=3, permute=(1, 0, 2, 3))
    pr.df = torch.nn.Parameter(torch.tensor(3.0))
    assert pr.fused_mvt_spec() is None
    pr = P.MultivariateT(shape, 0., 0.5, df=3., event_dim=3, permute=(1, 0, 2, 3))
    pr.scale_tril = torch.nn.Parameter(torch.ones(1, 1) * 0.5)
    assert pr.fused_mvt_spec() is None
    pr = P.MultivariateT(shape, torch.nn.Parameter(torch.zeros(1)), torch.ones(1, 1) * 0.5, df=3., event_dim=3,
                         permute=(1, 0, 2, 3))
    assert pr.fused_mvt_spec() is None
    # a factor of more than 25 positions, a batched factor, a non-contiguous tensor
    assert P.MultivariateT((4, 36), 0., torch.eye(36), df=3., event_dim=1).fused_mvt_spec() is None
    assert P.MultivariateT((4, 2, 3), 0., torch.eye(3).expand(2, 3, 3).clone(), df=3., event_dim=2).fused_mvt_spec() is None
    pr = P.MultivariateT(shape, 0., 0.5, df=3., event_dim=3, permute=(1, 0, 2, 3))
    pr.p.data = pr.p.data.transpose(0, 1).contiguous().transpose(0, 1)
    assert pr.fused_mvt_spec() is None


def test_number_loc_with_a_factor_is_one_location_per_position():
    L = torch.linalg.cholesky(torch.eye(9) * 0.5 + 0.1)
    pr = P.MultivariateT((4, 2, 3, 3), 0.3, L, df=3., event_dim=3, permute=(1, 0, 2, 3))
    assert pr.loc.shape == (9,) and torch.all(pr.loc == 0.3)
    assert np.allclose(pr.fused_mvt_spec()["mu"], 0.3)


def test_sampling_moments():
    "mean loc and covariance scale_tril scale_tril^T (Shah et al.'s parameterisation), reference test_priors.py"
    torch.manual_seed(102)
    N = 200000
    loc = torch.tensor([1., 2., 3., 4.])
    cov = torch.randn(4, 4)
    cov = cov @ cov.t()
    pr = P.MultivariateT((N, 2, 2), loc=loc, scale_tril=torch.linalg.cholesky(cov), df=8, event_dim=2)
    p = pr().detach().view(-1, 4).double()
    mean = p.mean(0)
    assert torch.allclose(mean, loc.double(), atol=0.03)
    b = p - mean
    emp = (b.t() @ b) / len(b)
    assert torch.allclose(emp, cov.double(), atol=0.05 * float(cov.abs().max()))
    # one mixing variable per EVENT: the permuted convolution draw is contiguous and has the prior's shape
    conv = P.MultivariateT((8, 5, 3, 3), 0., 0.5, df=4., event_dim=3, permute=(1, 0, 2, 3))
    assert conv.p.shape == (8, 5, 3, 3) and conv.p.is_contiguous()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _fused(priors, chunk, N):
    from bnn_priors_amd import mcmc
    model = torch.nn.ModuleList(priors)
    opt = mcmc.VerletSGLD([pr.p for pr in priors], lr=0.01, num_data=N, momentum=0.9, chunk_elems=chunk)
    assert opt.engine.chunk == chunk
    assert opt.fuse_priors(model) == []
    flags = opt.engine.layout.prior_flags
    assert flags & _hip.PRIOR_FULL and flags & _hip.PRIOR_EVENTS
    return opt


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("chunk", [_hip.CHUNK, _hip.CHUNK_SMALL])
def test_kernel_matches_the_reference_fixtures(golden_dir, dtype, chunk):
    """all five geometries in one table (segments of 4608 and 5120 elements: events straddle chunks of both sizes)"""
    z = _fixture(golden_dir)
    dev, N = "cuda:0", 61.0
    priors = [_case(z, name, dtype)[0].to(dev) for name in CASES]
    opt = _fused(priors, chunk, N)
    g0 = [torch.randn(pr.p.shape, generator=torch.Generator().manual_seed(i)).to(dtype).to(dev)
          for i, pr in enumerate(priors)]
    for pr, g in zip(priors, g0):
        pr.p.grad = g.clone()
    opt.add_prior_gradient(calc_log_prior=True)
    tol = dict(rtol=1e-4, atol=2e-6) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-12)
    want_lp = 0.0
    for name, pr, g in zip(CASES, priors, g0):
        want = g - torch.from_numpy(z["prior|" + name + "|grad"]).to(dtype).to(dev) / N
        torch.testing.assert_close(pr.p.grad, want, **tol, msg=lambda m: f"{name}: {m}")
        want_lp += float(z["prior|" + name + "|log_prob"])
    rel, ab = (1e-5, 1e-4) if dtype == torch.float32 else (1e-11, 1e-10)
    assert opt.fused_log_prior().item() == pytest.approx(want_lp, rel=rel, abs=ab)
    if dtype == torch.float32:
        # (the fixtures were taken at the float64 theta.)  Both launches work in fp64 from the stored values and round
        # once into g: against float64 autograd at the WIDENED float32 parameters the gradient is held to that one
        # rounding with a safety factor of 2, plus the float64 comparison's own allowance; the log-density to float64's
        import copy
        exact_lp = 0.0
        for name, pr, g in zip(CASES, priors, g0):
            wide = copy.deepcopy(pr).double()
            wide.p.grad = None
            lp = wide.log_prob()
            lp.backward()
            exact_lp += float(lp.detach())
            ref = g.double().cpu() - wide.p.grad.cpu() / N
            err = (pr.p.grad.double().cpu() - ref).abs()
            bound = 2 * 2.0 ** -24 * ref.abs() + (1e-10 * ref.abs() + 1e-12)
            worst = (err / bound).max().item()
            print(f"mvt-ratio {name} chunk {chunk}: worst error / bound {worst:.4f}")
            assert worst <= 1.0, (name, worst)
        assert opt.fused_log_prior().item() == pytest.approx(exact_lp, rel=1e-11, abs=1e-10)


@pytest.mark.gpu
def test_event_sums_are_bit_reproducible(golden_dir):
    z = _fixture(golden_dir)
    dev, N = "cuda:0", 50000.0
    priors = [_case(z, name, torch.float32)[0].to(dev) for name in CASES]
    opt = _fused(priors, _hip.CHUNK_SMALL, N)
    runs = []
    for _ in range(2):
        for pr in priors:
            pr.p.grad = torch.zeros_like(pr.p)
        opt.add_prior_gradient(calc_log_prior=True)
        runs.append(([pr.p.grad.clone() for pr in priors], opt.fused_log_prior().item(),
                     opt.engine._event_sums.clone()))
    (g0, lp0, s0), (g1, lp1, s1) = runs
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert lp0 == lp1 and torch.equal(s0, s1)
    assert math.isfinite(lp0)
