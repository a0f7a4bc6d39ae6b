"""The whitened-filter kind of the HIP prior hook (SGMCMC_PRIOR_FILTER_WHITENED, include/sgmcmc_hip.h): the correlated /
fixed-covariance convolution priors with fixed arguments (prior/correlated.py) are one segment-level branch of the full
prior kernel instead of autograd.  CPU: the host-built tables, evaluated with the kernel's formula in float64, against the
reference fixtures.  GPU: the kernel against the fixtures, against float64 autograd across chunk boundaries, and the in-place
refresh of ``assign_cov``."""
import numpy as np
import pytest
import torch

from bnn_priors_amd import _hip
from bnn_priors_amd import prior as P
from prior_reference import whitened
from test_priors import _build_remaining, _remaining_cases

FILTER_NAMES = ("convcorrnormal", "convcorrnormal_fitted_ls", "fixedcov_normal", "fixedcov_gennorm")
LEARNABLE_NAMES = ("convcorrnormal_gamma", "convcorrnormal_empirical")


def _filter_cases(golden_dir, names=FILTER_NAMES):
    z, keys = _remaining_cases(golden_dir)
    return z, [k for k in keys if k.split("|")[0] in names]


def test_host_tables_reproduce_the_reference_fixtures(golden_dir):
    z, keys = _filter_cases(golden_dir)
    assert len(keys) == 2 * 2 * (2 + 1 + 2 + 2)      # dtypes x shapes x cases of the four names
    for key in keys:
        name, pr, dtype, _ = _build_remaining(key, z)
        spec = pr.fused_filter_spec()
        assert spec is not None and spec["P"] == 9, key
        assert spec["base"] == (_hip.FILTER_BASE_GENNORM if name == "fixedcov_gennorm" else _hip.FILTER_BASE_NORMAL)
        lp, g, _ = whitened(spec, pr.p.detach().double().numpy())
        tol = dict(rtol=3e-5, atol=3e-5) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(lp, float(z[key + "|log_prior"]), **tol, err_msg=key)
        np.testing.assert_allclose(g, z[key + "|grad:p"].reshape(g.shape), rtol=tol["rtol"] * 10, atol=tol["atol"] * 10,
                                   err_msg=key)


def test_only_fixed_whitenings_are_filter_tables(golden_dir):
    """learnable scale / lengthscale stay in autograd; the multivariate priors never claim an element-wise fused_spec
    (tests/test_priors.py pins the element-wise routes of every name)"""
    z, keys = _remaining_cases(golden_dir)
    seen = set()
    for key in keys:
        name, pr, _, _ = _build_remaining(key, z)
        assert (pr.fused_filter_spec() is not None) == (name in FILTER_NAMES), key
        if name in FILTER_NAMES + LEARNABLE_NAMES:
            assert pr.fused_spec() is None, key
            seen.add(name)
    assert seen == set(FILTER_NAMES + LEARNABLE_NAMES)
    for name in ("gaussian", "laplace", "student-t", "cauchy", "gennorm", "improper", "lognormal"):
        assert P.get_prior(name)((4, 3, 3, 3), 0., 0.5).fused_filter_spec() is None, name


def test_filter_table_limits():
    torch.manual_seed(0)
    assert P.ConvCorrelatedNormal((4, 3, 5, 5), 0., 0.5).fused_filter_spec()["P"] == 25
    assert P.ConvCorrelatedNormal((4, 3, 3, 1), 0., 0.5).fused_filter_spec()["P"] == 3
    assert P.ConvCorrelatedNormal((4, 3, 1, 1), 0., 0.5).fused_filter_spec()["P"] == 1
    assert P.ConvCorrelatedNormal((2, 2, 6, 6), 0., 0.5).fused_filter_spec() is None        # P = 36 > 25
    pr = P.ConvCorrelatedNormal((4, 3, 3, 3), 0., 0.5)
    pr.p.data = pr.p.data.transpose(0, 1).contiguous().transpose(0, 1)                     # not contiguous
    assert pr.fused_filter_spec() is None


def test_assign_cov_changes_the_table():
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        pr = P.FixedCovNormal((3, 2, 3, 3), 0., 0.5)
        before = pr.fused_filter_spec()
        i = np.arange(9)
        cov = torch.from_numpy(0.2 * np.exp(-np.abs(i[:, None] - i[None, :])) + 0.05 * np.eye(9))
        pr.assign_cov(cov)
        after = pr.fused_filter_spec()
    finally:
        torch.set_default_dtype(torch.float32)
    assert not np.allclose(before["W"], after["W"])
    lp, g, _ = whitened(after, pr.p.detach().numpy())
    want_lp, want_g = _autograd(pr)
    np.testing.assert_allclose(lp, want_lp, rtol=1e-10)
    np.testing.assert_allclose(g, want_g.numpy(), rtol=1e-9, atol=1e-12)
    # the gradient is the new covariance's Gaussian one (the log-density differs from it by a constant, see
    # ConvCovariance.fused_filter_spec)
    th = pr.p.detach().clone().requires_grad_(True)
    torch.distributions.MultivariateNormal(torch.zeros(9, dtype=torch.float64), cov).log_prob(th.reshape(-1, 9)).sum().backward()
    np.testing.assert_allclose(g, th.grad.numpy(), rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_kernel_matches_the_reference_fixtures(golden_dir):
    from bnn_priors_amd import mcmc
    z, keys = _filter_cases(golden_dir)
    dev, N, done = "cuda:0", 61.0, 0
    for key in keys:
        _, pr, dtype, _ = _build_remaining(key, z)
        pr = pr.to(dev)
        opt = mcmc.VerletSGLD([pr.p], lr=0.01, num_data=N, momentum=0.9)
        assert opt.fuse_priors(pr) == [], key
        assert opt.engine.layout.prior_flags & _hip.PRIOR_FULL
        g0 = torch.randn(pr.p.shape, generator=torch.Generator().manual_seed(5)).to(dtype).to(dev)
        pr.p.grad = g0.clone()
        opt.add_prior_gradient(calc_log_prior=True)
        tol = dict(rtol=1e-4, atol=2e-6) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-12)
        want = g0 - torch.from_numpy(z[key + "|grad:p"]).to(dtype).to(dev).reshape(g0.shape) / N
        torch.testing.assert_close(pr.p.grad, want, **tol, msg=lambda m: f"{key}: {m}")
        assert opt.fused_log_prior().item() == pytest.approx(float(z[key + "|log_prior"]), rel=1e-5 if dtype == torch.float32 else 1e-11,
                                                             abs=1e-4 if dtype == torch.float32 else 1e-10), key
        done += 1
    assert done == 28


def _autograd(pr):
    "float64 log p and its gradient through the module's own (autograd) formulation"
    saved, grad = pr.p.data, pr.p.grad
    pr.p.grad = None
    lp = pr.log_prob()
    lp.backward()
    g = pr.p.grad.detach().cpu().double()
    pr.p.data, pr.p.grad = saved, grad
    return float(lp.detach()), g


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,dtype", [(_hip.CHUNK, torch.float64), (_hip.CHUNK_SMALL, torch.float64),
                                         (_hip.CHUNK, torch.float32), (_hip.CHUNK_SMALL, torch.float32)],
                         ids=["4096", "1024", "4096-float32", "1024-float32"])
def test_filters_straddling_chunks_match_float64_autograd(chunk, dtype):
    """several segments whose filters straddle the chunk boundaries (9, 25, 3 do not divide 4096 / 1024) and 1 x 1
    filters, Normal and generalised-normal bases: the kernel's gradient and log-density against float64 autograd.
    float32 arenas: the kernel works in fp64 from the stored values and rounds once into g, so the reference is float64
    autograd at the WIDENED float32 parameters (and widened arguments) and the gradient is held to one rounding of the
    result with a safety factor of 2, 2 * 2^-24 |ref|, plus the allowance the float64 comparison gives autograd itself"""
    import copy
    from bnn_priors_amd import mcmc
    dev, N = "cuda:0", 37.0
    torch.set_default_dtype(dtype)
    try:
        torch.manual_seed(3)
        priors = [P.ConvCorrelatedNormal((64, 64, 3, 3), 0., 0.3, lengthscale=0.7),
                  P.ConvCorrelatedNormal((16, 32, 1, 1), 0.1, 0.5),
                  P.FixedCovGenNorm((10, 7, 5, 5), 0., 0.4, beta=1.3),
                  P.FixedCovNormal((6, 4, 3, 1), 0.05, 0.6)]
    finally:
        torch.set_default_dtype(torch.float32)
    model = torch.nn.ModuleList(priors).to(dev)
    want_lp, want_g = 0.0, []
    for pr in priors:
        lp, g = _autograd(pr if dtype == torch.float64 else copy.deepcopy(pr).double())
        want_lp += lp
        want_g.append(g)
    opt = mcmc.VerletSGLD([pr.p for pr in priors], lr=0.01, num_data=N, momentum=0.9, chunk_elems=chunk)
    assert opt.engine.chunk == chunk and opt.engine.dtype == dtype
    assert opt.fuse_priors(model) == []
    g0 = [torch.randn(pr.p.shape, dtype=dtype, generator=torch.Generator().manual_seed(i)).double()
          for i, pr in enumerate(priors)]
    for pr, g in zip(priors, g0):
        pr.p.grad = g.to(dtype).to(dev)
    opt.add_prior_gradient(calc_log_prior=True)
    for pr, g, w in zip(priors, g0, want_g):
        ref = g - w / N
        if dtype == torch.float64:
            torch.testing.assert_close(pr.p.grad.cpu(), ref, rtol=1e-10, atol=1e-12)
        else:
            err = (pr.p.grad.cpu().double() - ref).abs()
            bound = 2 * 2.0 ** -24 * ref.abs() + (1e-10 * ref.abs() + 1e-12)
            worst = (err / bound).max().item()
            print(f"filter-ratio {tuple(pr.p.shape)} chunk {chunk}: worst error / bound {worst:.4f}")
            assert worst <= 1.0, (tuple(pr.p.shape), worst)
    assert opt.fused_log_prior().item() == pytest.approx(want_lp, rel=1e-11, abs=1e-9)


@pytest.mark.gpu
def test_assign_cov_after_fusing_refreshes_the_device_table():
    from bnn_priors_amd import mcmc
    dev, N = "cuda:0", 50.0
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        pr = P.FixedCovNormal((16, 8, 3, 3), 0., 0.5)
    finally:
        torch.set_default_dtype(torch.float32)
    pr = pr.to(dev)
    opt = mcmc.VerletSGLD([pr.p], lr=0.01, num_data=N, momentum=0.9)
    assert opt.fuse_priors(pr) == []
    table = opt.engine._filter_dev.data_ptr()

    def hook_grad():
        pr.p.grad = torch.zeros_like(pr.p)
        opt.add_prior_gradient(calc_log_prior=True)
        return pr.p.grad.clone(), opt.fused_log_prior().item()

    g_old, _ = hook_grad()
    i = np.arange(9)
    cov = torch.from_numpy(0.2 * np.exp(-np.abs(i[:, None] - i[None, :])) + 0.05 * np.eye(9))
    pr.assign_cov(cov.to(dev))
    g_new, lp_new = hook_grad()
    assert opt.engine._filter_dev.data_ptr() == table          # rewritten in place: a captured graph sees it
    want_lp, want_g = _autograd(pr)
    assert not torch.allclose(g_new, g_old)
    torch.testing.assert_close(g_new.cpu(), -want_g / N, rtol=1e-10, atol=1e-12)
    assert lp_new == pytest.approx(want_lp, rel=1e-11)
