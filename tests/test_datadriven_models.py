"""``datadrivengaussconv`` / ``datadrivendoublegammaconv`` (reference: models/data_driven_conv_nets.py:15-109,
exp_utils.py:130-152): construction by name against the reference's names, shapes, prior classes, keys and model-level
log-prior (tests/golden/make_datadriven_goldens.py), the ``prior_data`` routes, and on the GPU the fast path -- the
convolution priors in the HIP hook, the same gradient as the autograd formulation, a captured step that agrees with the
eager one, and finite samples."""
import copy
import gzip
import json
import os
import pickle
import sys
import warnings

import numpy as np
import pytest
import torch

from bnn_priors_amd import models
from bnn_priors_amd import prior as P
from bnn_priors_amd.models import data_driven

NAMES = ("datadrivengaussconv", "datadrivendoublegammaconv")


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "datadriven.npz"))


def fixture_prior_data(z):
    """the fixture's subset of the reference's two tables as ``prior_data`` ({file name: contents}), each value in its
    dtype in the files"""
    dtypes = json.loads(str(z["data|dtypes"]))
    mean_covs = {}
    for k in z.files:
        if k.startswith("data|mean_covs|"):
            name, j = k.split("|")[2:]
            v = z[k].astype(dtypes[f"{name}|{j}"])
            mean_covs.setdefault(name, [None, None])[int(j)] = v if v.ndim else v[()]
    fits = {k.split("|")[2]: {"dgamma": tuple(float(x) for x in z[k])} for k in z.files if k.startswith("data|dgamma|")}
    return {data_driven.MEAN_COVS_FILE: {k: tuple(v) for k, v in mean_covs.items()},
            data_driven.FITS_FILE: (None, fits)}


def _net(golden_dir, name, device="cpu", width=8, n=16, prior_data=None, **kw):
    torch.manual_seed(0)
    x, y = torch.rand(n, 784), torch.arange(n) % 10
    if prior_data is None:
        prior_data = fixture_prior_data(_fixture(golden_dir))
    torch.manual_seed(0)
    net = models.get_model(x, y, name, width=width, depth=3, prior_data=prior_data, **kw)
    return net.to(device), x.to(device), y.to(device)


def _in_hook(pr):
    return pr.fused_spec() is not None or pr.fused_filter_spec() is not None


@pytest.mark.parametrize("name", NAMES)
def test_builds_with_the_reference_parameters_priors_and_keys(golden_dir, name):
    z = _fixture(golden_dir)
    key = "model|" + name + "|"
    net, _, _ = _net(golden_dir, name, width=int(z["seeds"][2]))
    names = [n for n, _ in net.named_parameters()]
    mods = dict(net.named_modules())
    assert names == json.loads(str(z[key + "names"]))
    assert [list(p.shape) for _, p in net.named_parameters()] == json.loads(str(z[key + "shapes"]))
    assert list(net.state_dict().keys()) == json.loads(str(z[key + "state_keys"]))
    assert [type(mods[n[:-2]]).__name__ for n in names] == json.loads(str(z[key + "prior_types"]))


@pytest.mark.parametrize("name", NAMES)
def test_model_log_prior_matches_the_reference(golden_dir, name):
    "the autograd formulation (models/base.py:57-62) at the fixture's theta, float64 (built in float32, then .double())"
    z = _fixture(golden_dir)
    net, _, _ = _net(golden_dir, name, width=int(z["seeds"][2]))
    net = net.double()
    rng = np.random.default_rng(int(z["seeds"][1]))
    with torch.no_grad():
        for _, p in net.named_parameters():
            p.copy_(torch.from_numpy(rng.standard_normal(p.shape) * 0.1))
    lp = net.log_prior()
    lp.backward()
    key = "model|" + name + "|"
    assert float(lp.detach()) == pytest.approx(float(z[key + "log_prior"]), rel=1e-12)
    for n, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), z[key + "grad:" + n], rtol=1e-10, atol=1e-12, err_msg=n)


def test_routes_of_the_priors(golden_dir):
    """gauss: every prior in the hook (nothing left for autograd); doublegamma: the convolutions in the hook (Laplace and
    double-Gamma bases), exactly the head's element-wise DoubleGamma left over"""
    from bnn_priors_amd import _hip
    net, _, _ = _net(golden_dir, "datadrivengaussconv", width=50)
    assert all(_in_hook(pr) for _, pr in P.named_priors(net))
    net, _, _ = _net(golden_dir, "datadrivendoublegammaconv", width=50)
    left = [n for n, pr in P.named_priors(net) if not _in_hook(pr)]
    assert left == ["net.module.8.weight_prior"]
    bases = {n: pr.fused_filter_spec()["base"] for n, pr in P.named_priors(net) if pr.fused_filter_spec() is not None}
    assert bases == {"net.module.1.weight_prior": _hip.FILTER_BASE_LAPLACE,
                     "net.module.4.weight_prior": _hip.FILTER_BASE_DOUBLE_GAMMA}


def test_fitted_arguments_reach_their_priors(golden_dir):
    z = _fixture(golden_dir)
    net, _, _ = _net(golden_dir, "datadrivendoublegammaconv", width=50)
    mods = dict(net.named_modules())
    dg4, dg8 = z["data|dgamma|net.module.4.weight_prior.p"], z["data|dgamma|net.module.8.weight_prior.p"]
    c4 = float(mods["net.module.4.weight_prior"].concentration)
    assert c4 == pytest.approx(dg4[0], rel=1e-7)
    assert float(mods["net.module.4.weight_prior"].base_rate) == pytest.approx((c4 * (1 + c4)) ** .5, rel=1e-7)
    head = mods["net.module.8.weight_prior"]
    assert type(head) is P.DoubleGamma
    np.testing.assert_allclose([float(head.concentration), float(head.loc), float(head.scale)], dg8, rtol=1e-6)
    bias = mods["net.module.4.bias_prior"]
    assert float(bias.loc) == 0.0                  # the fitted bias mean is ignored, as Conv2dPrior ignores loc_b
    assert float(bias.scale) == pytest.approx(z["data|mean_covs|net.module.4.bias_prior.p|1"] ** .5, rel=1e-6)
    np.testing.assert_allclose(mods["net.module.1.weight_prior"].loc.numpy(),
                               z["data|mean_covs|net.module.1.weight_prior.p|0"], rtol=1e-7)


def test_weight_arguments_are_ignored(golden_dir):
    a, _, _ = _net(golden_dir, "datadrivengaussconv")
    b, _, _ = _net(golden_dir, "datadrivengaussconv", weight_prior="laplace", weight_loc=3., weight_scale=7.)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


def test_depth_must_be_three(golden_dir):
    with pytest.raises(AssertionError):
        models.get_model(torch.rand(4, 784), torch.arange(4), "datadrivengaussconv", depth=4,
                         prior_data=fixture_prior_data(_fixture(golden_dir)))


def _write_tables(directory, data):
    os.makedirs(directory, exist_ok=True)
    for fname, value in data.items():
        with gzip.open(os.path.join(directory, fname), "wb") as f:
            pickle.dump(value, f)


def test_prior_data_directory_mapping_and_missing(golden_dir, tmp_path, monkeypatch):
    data = fixture_prior_data(_fixture(golden_dir))
    _write_tables(tmp_path / "tables", data)
    for name in NAMES:
        a, _, _ = _net(golden_dir, name, prior_data=data)
        b, _, _ = _net(golden_dir, name, prior_data=str(tmp_path / "tables"))
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and va.dtype == vb.dtype and torch.equal(va, vb), (name, ka)
        with pytest.raises(FileNotFoundError, match=data_driven.FITS_FILE):
            _net(golden_dir, name, prior_data=str(tmp_path / "nowhere"))
    # None: next to an installed reference package (found without importing it) ...
    pkg = tmp_path / "site"
    (pkg / "bnn_priors").mkdir(parents=True)
    (pkg / "bnn_priors" / "__init__.py").write_text("raise ImportError('must not be imported')\n")
    _write_tables(pkg / "bnn_priors" / "models", data)
    monkeypatch.delitem(sys.modules, "bnn_priors", raising=False)
    monkeypatch.syspath_prepend(str(pkg))
    a, _, _ = _net(golden_dir, "datadrivendoublegammaconv", prior_data=data)
    x, y = torch.rand(16, 784), torch.arange(16) % 10
    torch.manual_seed(0)
    b = models.get_model(x, y, "datadrivendoublegammaconv", width=8)
    assert all(torch.equal(va, vb) for va, vb in zip(a.state_dict().values(), b.state_dict().values()))
    # ... or FileNotFoundError naming both files
    for f in data:
        os.remove(pkg / "bnn_priors" / "models" / f)
    with pytest.raises(FileNotFoundError, match=data_driven.MEAN_COVS_FILE) as err:
        models.get_model(torch.rand(4, 784), torch.arange(4), "datadrivengaussconv")
    assert data_driven.FITS_FILE in str(err.value)
    monkeypatch.setattr(data_driven, "_reference_models_dir", lambda: None)
    with pytest.raises(FileNotFoundError, match=data_driven.FITS_FILE):
        models.get_model(torch.rand(4, 784), torch.arange(4), "datadrivendoublegammaconv")


# ---------------------------------------------------------------------------------------------------------------- GPU
def _check_potential(net, x, y, N, leftover):
    """the hook's potential and gradient against a deep-copied autograd reference: its likelihood in float32, its priors
    in float64 (the kernel evaluates them in fp64; float32 autograd of a double-Gamma base is off by up to 2% where a
    whitened coordinate is near 0)"""
    from bnn_priors_amd import _hip, mcmc, potential
    ref, ref64 = copy.deepcopy(net), copy.deepcopy(net).double()
    opt = mcmc.VerletSGLD(net.parameters(), lr=1e-4, num_data=N, momentum=0.9, temperature=1.0, seed=3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        pot = potential.Potential(net, opt, N)
    assert pot.fast
    assert [type(pr).__name__ + ":" + str(tuple(pr.p.shape)) for pr in pot.leftover] == list(leftover)
    assert bool([w for w in caught if "differentiated by autograd" in str(w.message)]) == bool(leftover)
    assert int((opt.engine.seg_host["prior_kind"] == _hip.PRIOR_FILTER_WHITENED).sum()) == 2
    results = []
    for _ in range(2):                   # twice: the same bits
        for p in net.parameters():
            p.grad = None
        loss, log_prior, pot_value, acc = pot.minibatch(x, y, True)
        results.append((float(log_prior), float(pot_value), [p.grad.clone() for p in net.parameters()]))
    assert results[0][:2] == results[1][:2]
    assert all(torch.equal(a, b) for a, b in zip(results[0][2], results[1][2]))
    loss_ref = -ref.log_likelihood_avg(x, y)
    loss_ref.backward()
    lp_ref = ref64.log_prior()
    lp_ref.backward()
    assert results[0][0] == pytest.approx(float(lp_ref.detach()), rel=2e-5, abs=1e-3)
    assert results[0][1] == pytest.approx(float(loss_ref.detach()) - float(lp_ref.detach()) / N, rel=2e-5, abs=1e-5)
    for (n_, p), (_, q), (_, q64) in zip(net.named_parameters(), ref.named_parameters(), ref64.named_parameters()):
        want = (q.grad if q.grad is not None else torch.zeros_like(q)) - (q64.grad / N).float()
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        torch.testing.assert_close(got, want, rtol=2e-4, atol=2e-6, msg=lambda m: f"{n_}: {m}")
    opt.sample_momentum()
    opt.initial_step(save_state=False)
    assert all(torch.isfinite(p).all() for p in net.parameters())


@pytest.mark.gpu
def test_gauss_takes_the_hook(golden_dir):
    net, x, y = _net(golden_dir, "datadrivengaussconv", "cuda:0", width=50, n=128)
    models.he_initialize(net)
    _check_potential(net, x, y, 60000.0, ())


@pytest.mark.gpu
def test_doublegamma_leaves_only_the_head(golden_dir):
    net, x, y = _net(golden_dir, "datadrivendoublegammaconv", "cuda:0", width=50, n=128)
    models.he_initialize(net)
    _check_potential(net, x, y, 60000.0, ("DoubleGamma:(10, 2450)",))


def _run(golden_dir, name, use_graph):
    import runner_cases as RC
    from bnn_priors_amd import inference_reject
    from bnn_priors_amd.storage import MemoryMetrics
    cfg = dict(RC.CASES["VerletSGLDReject"], n=512)
    dev = "cuda:0"
    train, test, (x, y) = RC.make_data(dev, cfg)
    torch.manual_seed(0)
    model = models.get_model(x, y, name, width=50, depth=3, prior_data=fixture_prior_data(_fixture(golden_dir)))
    torch.manual_seed(1)
    models.he_initialize(model)
    model = model.to(dev)
    metrics = MemoryMetrics()
    torch.manual_seed(RC.SEED)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        runner = inference_reject.VerletSGLDRunnerReject(
            model=model, dataloader=train, dataloader_test=test, learning_rate=cfg["lr"],
            temperature=cfg["temperature"], momentum=cfg["momentum"], reject_samples=True,
            metrics_saver=metrics, model_saver=None, seed=RC.SEED, chain_id=0,
            cycle_seed=RC.CYCLE_SEED, use_graph=use_graph, **RC.RUN_KW)
        runner.run()
    assert runner.optimizer.engine.filter_host is not None
    return runner, RC.streams_of(metrics), {k: v.clone() for k, v in runner.get_samples().items()}


@pytest.mark.gpu
def test_gauss_graph_replay_agrees_with_eager(golden_dir):
    """the captured step (GraphedLeapfrog, whose prior launch is the full kernel with the filter table) really captures:
    accept / reject decisions, step indices, lr and temperature bit for bit, the float streams and samples within the
    tolerances of test_correlated_models.py (the same convnet trunk)"""
    import runner_cases as RC
    outs = []
    for use_graph in (False, True):
        runner, streams, samples = _run(golden_dir, "datadrivengaussconv", use_graph)
        assert (runner._graphed not in (None, False)) == use_graph
        outs.append((streams, samples))
    (s0, p0), (s1, p1) = outs
    assert sorted(s0) == sorted(s1)
    for k in s0:
        if k in ("timestamps",):
            continue
        assert np.array_equal(s0[k][0], s1[k][0]), k
        if k in RC.STREAMS_EXACT:
            assert np.array_equal(s0[k][1], s1[k][1]), (k, s0[k][1], s1[k][1])
        else:
            np.testing.assert_allclose(s1[k][1], s0[k][1], rtol=1e-5, atol=1e-7, err_msg=k)
    for k in p0:
        assert torch.isfinite(p0[k]).all(), k
        torch.testing.assert_close(p1[k], p0[k], rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")


@pytest.mark.gpu
def test_doublegamma_runs_eagerly_and_stays_finite(golden_dir):
    runner, streams, samples = _run(golden_dir, "datadrivendoublegammaconv", use_graph=True)
    assert runner._graphed in (None, False)           # the head's prior is in autograd: no capture
    assert samples and all(torch.isfinite(v).all() for v in samples.values())
    for k in ("delta_energy", "total_energy"):
        if k in streams:
            assert np.isfinite(streams[k][1]).all(), k
