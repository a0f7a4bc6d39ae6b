"""``FixedCovLaplace`` / ``FixedCovDoubleGamma`` (reference: prior/conv_loc_scale.py:82-114) and their base densities in
the whitened-filter kind of the HIP prior hook (SGMCMC_FILTER_BASE_LAPLACE / _DOUBLE_GAMMA, include/sgmcmc_hip.h).
CPU: construction, sampling, keys and autograd against the reference fixtures (tests/golden/make_datadriven_goldens.py),
and the host-built tables evaluated with the kernel's formula.  GPU: the kernel against the fixtures on segments that cross
chunk boundaries, against float64 autograd, at z == 0, and run to run."""
import json
import math
import os

import numpy as np
import pytest
import torch

from bnn_priors_amd import _hip
from bnn_priors_amd import prior as P
from bnn_priors_amd.prior import loc_scale
from golden.ref_stubs import REFERENCE_ROOT
from prior_reference import whitened

DTYPES = (torch.float32, torch.float64)


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "datadriven.npz"))


def _cases(z):
    return sorted({k.split("|")[1] for k in z.files if k.startswith("prior|")})


def _synthetic_cov(n):
    "the generator's synthetic covariance (make_datadriven_goldens.synthetic_cov)"
    rng = np.random.default_rng(n)
    i = np.arange(n)
    a = rng.standard_normal((n, n)) * 0.1
    return 0.3 * np.exp(-np.abs(i[:, None] - i[None, :]) / 2.0) + a @ a.T + 0.05 * np.eye(n)


def _build(z, case, dtype, seed=None):
    """the fixture's case in this package, constructed under ``dtype`` as the default (and ``torch.manual_seed(seed)``,
    the generator's SEED by default)"""
    cfg = json.loads(str(z[f"prior|{case}|config"]))
    n = cfg["shape"][-2] * cfg["shape"][-1]
    dt = json.loads(str(z["data|dtypes"]))
    if cfg["cov"] == "synthetic":
        loc, cov = cfg["loc"], torch.from_numpy(_synthetic_cov(n))
    else:
        key = cfg["cov"] + ".weight_prior.p"
        loc = torch.from_numpy(z[f"data|mean_covs|{key}|0"].astype(dt[key + "|0"]))
        cov = torch.from_numpy(z[f"data|mean_covs|{key}|1"].astype(dt[key + "|1"]))
    kw = dict(cfg["kw"])
    if isinstance(kw.get("concentration"), str):
        kw["concentration"] = np.float64(z["data|dgamma|" + kw["concentration"] + ".weight_prior.p"][0])
    torch.set_default_dtype(dtype)
    try:
        torch.manual_seed(int(z["seeds"][0]) if seed is None else seed)
        return getattr(P, cfg["cls"])(cfg["shape"], loc, cov, **kw)
    finally:
        torch.set_default_dtype(torch.float32)


def _key(case, dtype):
    return f"prior|{case}|{str(dtype)[6:]}|"


def _autograd(pr):
    "log p and its gradient through the module's own (autograd) formulation, in the prior's dtype"
    saved, grad = pr.p.data, pr.p.grad
    pr.p.grad = None
    lp = pr.log_prob()
    lp.backward()
    g = pr.p.grad.detach().cpu().double()
    pr.p.data, pr.p.grad = saved, grad
    return float(lp.detach()), g


def _tol(dtype):
    return dict(rtol=3e-5, atol=3e-5) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-10)


def test_fixture_covers_the_issue_matrix(golden_dir):
    z = _fixture(golden_dir)
    cfgs = [json.loads(str(z[f"prior|{c}|config"])) for c in _cases(z)]
    assert {c["cls"] for c in cfgs} == {"FixedCovLaplace", "FixedCovDoubleGamma"}
    assert {c["shape"][-1] ** 2 for c in cfgs} == {9, 25}
    assert {c["cov"] == "synthetic" for c in cfgs} == {True, False}
    conc = [float(_build(z, c, torch.float64).concentration) for c in _cases(z) if "dgamma" in c]
    assert min(conc) < 1 and 1.0 in conc and max(conc) > 1
    assert 0.28 == pytest.approx(min(conc), abs=1e-2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_construction_sampling_and_keys_match_the_reference(golden_dir, dtype):
    z = _fixture(golden_dir)
    seed = int(z["seeds"][0])
    for case in _cases(z):
        key = _key(case, dtype)
        pr = _build(z, case, dtype)
        assert list(pr.state_dict().keys()) == json.loads(str(z[key + "state_keys"])), case
        assert pr().dtype == dtype
        tol = dict(rtol=1e-6, atol=1e-7) if dtype == torch.float32 else dict(rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(pr().detach().double().numpy(), z[key + "sample"], **tol, err_msg=case)
        torch.manual_seed(seed + 1)
        pr.sample()
        np.testing.assert_allclose(pr.p.detach().double().numpy(), z[key + "resample"], **tol, err_msg=case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_log_prob_and_gradient_match_the_reference(golden_dir, dtype):
    z = _fixture(golden_dir)
    for case in _cases(z):
        key = _key(case, dtype)
        pr = _build(z, case, dtype)
        with torch.no_grad():
            pr.p.copy_(torch.from_numpy(z[key + "theta"]))
        lp, g = _autograd(pr)
        tight = dict(rtol=1e-5, atol=1e-4) if dtype == torch.float32 else dict(rtol=1e-12, atol=1e-10)
        assert lp == pytest.approx(float(z[key + "log_prob"]), rel=tight["rtol"]), case
        np.testing.assert_allclose(g.numpy(), z[key + "grad"], **tight, err_msg=case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_tables_reproduce_the_reference_fixtures(golden_dir, dtype):
    "the tables the hook receives, evaluated with the kernel's formula in float64 (as test_filter_prior.py does)"
    z = _fixture(golden_dir)
    for case in _cases(z):
        key = _key(case, dtype)
        pr = _build(z, case, dtype)
        spec = pr.fused_filter_spec()
        cfg = json.loads(str(z[f"prior|{case}|config"]))
        assert spec is not None and spec["P"] == cfg["shape"][-1] ** 2, case
        assert pr.fused_spec() is None and pr.fused_mvt_spec() is None
        want_base = _hip.FILTER_BASE_LAPLACE if cfg["cls"] == "FixedCovLaplace" else _hip.FILTER_BASE_DOUBLE_GAMMA
        assert spec["base"] == want_base, case
        lp, g, _ = whitened(spec, z[key + "theta"])
        tol = _tol(dtype)
        np.testing.assert_allclose(lp, float(z[key + "log_prob"]), **tol, err_msg=case)
        np.testing.assert_allclose(g, z[key + "grad"], rtol=tol["rtol"] * 10, atol=tol["atol"] * 10, err_msg=case)


def test_table_arguments():
    "the record's beta / base_scale and per-filter log-normaliser of both bases (include/sgmcmc_hip.h)"
    torch.manual_seed(0)
    lap = P.FixedCovLaplace((4, 3, 3, 3), 0.1, 0.5)
    spec = lap.fused_filter_spec()
    lsv = 9 * math.log(0.5)                # log sqrt det of 0.25 I_9
    assert spec["base_scale"] == pytest.approx(math.sqrt(0.5), rel=1e-7)
    assert spec["lognorm"] == pytest.approx(9 * -math.log(2 * math.sqrt(0.5)) - 9 * lsv, rel=1e-6)
    np.testing.assert_allclose(spec["mu"], np.full(9, 0.1), rtol=1e-7)
    c = 0.62
    dg = P.FixedCovDoubleGamma((4, 3, 3, 3), 0., 0.5, concentration=c)
    spec = dg.fused_filter_spec()
    r = math.sqrt(c * (1 + c))
    assert float(dg.base_rate) == pytest.approx(r, rel=1e-7)
    assert spec["beta"] == pytest.approx(c, rel=1e-7) and spec["base_scale"] == pytest.approx(1 / r, rel=1e-6)
    assert spec["lognorm"] == pytest.approx(9 * (c * math.log(r) - math.lgamma(c) - math.log(2)) - 9 * lsv, rel=1e-6)
    dg = P.FixedCovDoubleGamma((4, 3, 3, 3), 0., 0.5, concentration=2.0, base_scale=0.25)
    assert float(dg.base_rate) == 4.0 and dg.fused_filter_spec()["base_scale"] == 0.25


def test_learnable_arguments_stay_in_autograd():
    torch.manual_seed(0)
    lap = P.FixedCovLaplace((4, 3, 3, 3), 0., 0.5, base_scale=torch.nn.Parameter(torch.tensor(0.7)))
    assert lap.fused_filter_spec() is None
    dg = P.FixedCovDoubleGamma((4, 3, 3, 3), 0., 0.5, concentration=torch.nn.Parameter(torch.tensor(0.6)),
                               base_scale=0.5)
    assert dg.fused_filter_spec() is None
    assert P.FixedCovDoubleGamma((2, 2, 6, 6), 0., 0.5, concentration=0.6).fused_filter_spec() is None    # P = 36


def test_kernel_formula_at_the_location():
    "theta_f == mu: psi is 0 (autograd gives NaN for the double Gamma there), the log term is xlogy's 0 / +-inf"
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        priors = {c: P.FixedCovDoubleGamma((2, 3, 3, 3), 0.05, 0.5, concentration=c) for c in (0.5, 1.0, 2.5)}
        priors["laplace"] = P.FixedCovLaplace((2, 3, 3, 3), 0.05, 0.5)
    finally:
        torch.set_default_dtype(torch.float32)
    for c, pr in priors.items():
        spec = pr.fused_filter_spec()
        th = pr.p.detach().numpy().copy()
        th[1, 2] = 0.05                                     # one whole filter at its location
        lp, g, _ = whitened(spec, th)
        assert np.all(np.isfinite(g)) and np.all(g[1, 2] == 0.0), c
        want = {0.5: math.inf, 2.5: -math.inf}.get(c)
        assert lp == want if want is not None else math.isfinite(lp), c


def test_exports_and_the_name_table_is_unchanged():
    from bnn_priors_amd.prior import correlated
    assert {"FixedCovLaplace", "FixedCovDoubleGamma"} <= set(correlated.__all__)
    assert P.FixedCovLaplace is correlated.FixedCovLaplace and P.FixedCovDoubleGamma is correlated.FixedCovDoubleGamma
    table = loc_scale._table()
    assert len(table) == 31
    assert not {P.FixedCovLaplace, P.FixedCovDoubleGamma} & set(table.values())


def test_assign_cov_changes_the_table():
    torch.manual_seed(0)
    pr = P.FixedCovDoubleGamma((3, 2, 3, 3), 0., 0.5, concentration=1.5)
    before = pr.fused_filter_spec()
    pr.assign_cov(torch.from_numpy(_synthetic_cov(9)))
    after = pr.fused_filter_spec()
    assert not np.allclose(before["W"], after["W"]) and after["base"] == _hip.FILTER_BASE_DOUBLE_GAMMA


@pytest.mark.skipif(not os.path.isdir(REFERENCE_ROOT), reason="the reference is not on this machine")
def test_generator_check_mode_passes(golden_dir):
    import subprocess
    import sys
    subprocess.check_call([sys.executable, os.path.join(golden_dir, "make_datadriven_goldens.py"), "--check"],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _fuse(priors, N, chunk=None):
    from bnn_priors_amd import mcmc
    kw = {} if chunk is None else dict(chunk_elems=chunk)
    opt = mcmc.VerletSGLD([pr.p for pr in priors], lr=0.01, num_data=N, momentum=0.9, **kw)
    assert opt.fuse_priors(torch.nn.ModuleList(priors)) == []
    assert opt.engine.layout.prior_flags & _hip.PRIOR_FULL
    return opt


def _hook(opt, priors, g0):
    for pr, g in zip(priors, g0):
        pr.p.grad = g.clone()
    opt.add_prior_gradient(calc_log_prior=True)
    return [pr.p.grad.clone() for pr in priors], opt.fused_log_prior().item()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_reference_fixtures(golden_dir, dtype):
    """the six cases as segments of ONE optimizer with 1024-element chunks: every tensor (1152 / 1200 elements) spans two
    chunks and P = 9 / 25 does not divide 1024, so filters straddle the boundary"""
    z = _fixture(golden_dir)
    dev, N = "cuda:0", 61.0
    cases = _cases(z)
    priors = []
    for case in cases:
        pr = _build(z, case, dtype).to(dev)
        assert pr.p.numel() > _hip.CHUNK_SMALL
        with torch.no_grad():
            pr.p.copy_(torch.from_numpy(z[_key(case, dtype) + "theta"]))
        priors.append(pr)
    opt = _fuse(priors, N, chunk=_hip.CHUNK_SMALL)
    assert opt.engine.chunk == _hip.CHUNK_SMALL
    g0 = [torch.randn(pr.p.shape, generator=torch.Generator().manual_seed(5 + i)).to(dtype).to(dev)
          for i, pr in enumerate(priors)]
    grads, lp = _hook(opt, priors, g0)
    want_lp = 0.0
    for case, g, base, pr in zip(cases, grads, g0, priors):
        key = _key(case, dtype)
        if dtype == torch.float64:
            want = base - torch.from_numpy(z[key + "grad"]).to(dev) / N
            torch.testing.assert_close(g, want, rtol=1e-10, atol=1e-12, msg=lambda m: f"{case}: {m}")
        else:
            # float32: the kernel is the float64 formula rounded once into g; the reference's own float32 autograd is
            # further off (large whitening factors of the fitted covariances), so it is held to the host test's tolerance
            _, formula, _ = whitened(pr.fused_filter_spec(), z[key + "theta"])
            want = base.double() - torch.from_numpy(formula).to(dev) / N
            torch.testing.assert_close(g.double(), want, rtol=1e-6, atol=1e-6, msg=lambda m: f"{case}: {m}")
            grad = ((base.double() - g.double()) * N).cpu().numpy()
            np.testing.assert_allclose(grad, z[key + "grad"], rtol=3e-4, atol=3e-4, err_msg=case)
        want_lp += float(z[key + "log_prob"])
    assert lp == pytest.approx(want_lp, rel=3e-5 if dtype == torch.float32 else 1e-11)


def _away_from_kinks(pr, seed):
    "theta = z @ scale + loc with every |z| >= 0.1 (float64): random, and clear of the bases' kink at z == 0"
    rng = np.random.default_rng(seed)
    shape = tuple(pr.p.shape)
    z = rng.standard_normal(shape[:-2] + (shape[-2] * shape[-1],))
    z = np.sign(z) * (0.1 + np.abs(z))
    th = z @ pr.scale.detach().cpu().double().numpy() + pr.loc.detach().cpu().double().numpy()
    with torch.no_grad():
        pr.p.copy_(torch.from_numpy(th.reshape(shape)))
    return pr


def _random_priors():
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(3)
        i = np.arange(9)
        fitted_like = torch.from_numpy(0.01 * np.exp(-np.abs(i[:, None] - i[None, :]) / 3.0) + 0.002 * np.eye(9))
        priors = [P.FixedCovLaplace((64, 64, 3, 3), 0.01, fitted_like),
                  P.FixedCovDoubleGamma((50, 50, 3, 3), -0.003, fitted_like, concentration=0.6218),
                  P.FixedCovDoubleGamma((10, 7, 5, 5), 0.0, torch.from_numpy(_synthetic_cov(25)), concentration=1.0,
                                        base_scale=0.6),
                  P.FixedCovDoubleGamma((16, 32, 1, 1), 0.1, 0.5, concentration=2.5),
                  P.FixedCovLaplace((6, 4, 3, 1), 0.05, 0.6, base_scale=0.3)]
        return [_away_from_kinks(pr, i) for i, pr in enumerate(priors)]
    finally:
        torch.set_default_dtype(torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [_hip.CHUNK, _hip.CHUNK_SMALL])
def test_kernel_matches_float64_autograd(chunk):
    "random theta (P = 9, 25, 1, 3; both chunk sizes): gradient and log-density against autograd"
    dev, N = "cuda:0", 37.0
    priors = [pr.to(dev) for pr in _random_priors()]
    want = [_autograd(pr) for pr in priors]
    opt = _fuse(priors, N, chunk=chunk)
    g0 = [torch.randn(pr.p.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(i)).to(dev)
          for i, pr in enumerate(priors)]
    grads, lp = _hook(opt, priors, g0)
    for g, base, (_, w) in zip(grads, g0, want):
        torch.testing.assert_close(g.cpu(), base.cpu() - w / N, rtol=1e-10, atol=1e-12)
    assert lp == pytest.approx(sum(w[0] for w in want), rel=1e-11)


# filters of a [40, 30, 3, 3] tensor: filter 5, filter 113 (elements 1017..1025: across the first 1024-element chunk), the
# last filter
AT_LOCATION = ((0, 5), (3, 23), (39, 29))


@pytest.mark.gpu
def test_filters_at_their_location():
    """theta_f == mu for some filters: psi = 0 there (the element keeps its incoming gradient), autograd's value
    elsewhere, and the log-density is xlogy's: finite for c == 1 and Laplace, +inf for c < 1, -inf for c > 1"""
    dev, N = "cuda:0", 20.0
    for c, want_inf in ((1.0, None), (0.62, math.inf), (2.5, -math.inf), ("laplace", None)):
        torch.set_default_dtype(torch.float64)
        try:
            torch.manual_seed(7)
            pr = (P.FixedCovLaplace((40, 30, 3, 3), 0.02, 0.3) if c == "laplace"
                  else P.FixedCovDoubleGamma((40, 30, 3, 3), 0.02, 0.3, concentration=c))
        finally:
            torch.set_default_dtype(torch.float32)
        _away_from_kinks(pr, 2)
        with torch.no_grad():
            for f in AT_LOCATION:
                pr.p[f] = 0.02
        spec = pr.fused_filter_spec()
        want_lp, want_g, _ = whitened(spec, pr.p.detach().numpy())
        pr = pr.to(dev)
        opt = _fuse([pr], N, chunk=_hip.CHUNK_SMALL)
        g0 = torch.randn(pr.p.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
        (g,), lp = _hook(opt, [pr], [g0])
        assert torch.isfinite(g).all()
        for f in AT_LOCATION:
            assert torch.equal(g[f], g0[f]), (c, f)
        torch.testing.assert_close(g.cpu(), g0.cpu() - torch.from_numpy(want_g) / N, rtol=1e-10, atol=1e-12)
        if want_inf is None:
            assert math.isfinite(lp) and lp == pytest.approx(want_lp, rel=1e-11), c
        else:
            assert lp == want_inf == want_lp, c
        # elsewhere the kernel agrees with autograd
        mask = torch.ones(40, 30, dtype=torch.bool)
        for f in AT_LOCATION:
            mask[f] = False
        _, ag = _autograd(pr)
        torch.testing.assert_close(g.cpu()[mask], (g0.cpu() - ag / N)[mask], rtol=1e-10, atol=1e-12)


@pytest.mark.gpu
def test_two_runs_give_identical_bits():
    dev, N = "cuda:0", 37.0
    out = []
    for _ in range(2):
        priors = [pr.to(dev) for pr in _random_priors()]
        opt = _fuse(priors, N)
        g0 = [torch.zeros_like(pr.p) for pr in priors]
        out.append(_hook(opt, priors, g0))
    (g_a, lp_a), (g_b, lp_b) = out
    assert lp_a == lp_b
    for a, b in zip(g_a, g_b):
        assert torch.equal(a, b)
