"""``correlatedgoogleresnet`` / ``correlatedclassificationconvnet`` (reference: models/google_resnet.py:81-93,
models/conv_nets.py:73-115, exp_utils.py:130-152,201-207): construction by name against the reference's names, shapes and
keys (tests/golden/make_correlated_model_goldens.py), and on the GPU the whole fast path -- convolution priors in the HIP
hook (nothing left over), the same gradient as the reference formulation, a captured step bit-identical to the eager one."""
import copy
import json
import os
import warnings

import numpy as np
import pytest
import torch

from bnn_priors_amd import models
from bnn_priors_amd import prior as P
from golden.ref_stubs import REFERENCE_ROOT

NAMES = ("correlatedgoogleresnet", "correlatedclassificationconvnet")


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "correlated_models.npz"))


def _net(name, device="cpu", width=8, lengthscales=(0.5, 2.0), n=16):
    torch.manual_seed(0)
    if name == "correlatedgoogleresnet":
        x, y = torch.rand(n, 3, 32, 32), torch.randint(0, 10, (n,))
        kw = dict(weight_prior_params={"lengthscale": lengthscales[0]})
    else:
        x, y = torch.rand(n, 784), torch.randint(0, 10, (n,))
        kw = dict(width=width, depth=3,
                  weight_prior_params={"lengthscale_1": lengthscales[0], "lengthscale_2": lengthscales[1]})
    net = models.get_model(x, y, name, weight_prior="convcorrnormal", weight_loc=0., weight_scale=2 ** .5,
                           bias_prior="gaussian", bias_scale=1., **kw)
    return net.to(device), x.to(device), y.to(device)


@pytest.mark.parametrize("name", NAMES)
def test_names_build_with_the_reference_parameters_and_keys(golden_dir, name):
    z = _fixture(golden_dir)
    net, _, _ = _net(name)
    assert [n for n, _ in net.named_parameters()] == json.loads(str(z[name + "|names"]))
    assert [list(p.shape) for _, p in net.named_parameters()] == json.loads(str(z[name + "|shapes"]))
    assert list(net.state_dict().keys()) == json.loads(str(z[name + "|state_keys"]))
    convs = [m for m in net.modules() if isinstance(m, models.nets.Conv2d)]
    heads = [m for m in net.modules() if isinstance(m, models.nets.Linear)]
    assert convs and all(isinstance(m.weight_prior, P.ConvCorrelatedNormal) for m in convs)
    assert all(m.weight_prior.fused_filter_spec() is not None for m in convs)
    assert heads and all(type(m.weight_prior) is P.Normal for m in heads)       # the dense head stays Normal


def test_lengthscales_reach_their_layers():
    net, _, _ = _net("correlatedclassificationconvnet", lengthscales=(0.5, 2.0))
    conv = [m.weight_prior for m in net.modules() if isinstance(m, models.nets.Conv2d)]
    assert [float(c.lengthscale) for c in conv] == [0.5, 2.0]
    net, _, _ = _net("correlatedgoogleresnet", lengthscales=(0.7, None))
    conv = [m.weight_prior for m in net.modules() if isinstance(m, models.nets.Conv2d)]
    assert len(conv) == 21 and all(float(c.lengthscale) == pytest.approx(0.7) for c in conv)


def test_convnet_log_prior_matches_the_reference(golden_dir):
    "the autograd formulation (models/base.py:57-62) at the fixture's theta, float64"
    z = _fixture(golden_dir)
    torch.set_default_dtype(torch.float64)
    try:
        net, _, _ = _net("correlatedclassificationconvnet")
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(z["correlatedclassificationconvnet|theta:" + n]))
    lp = net.log_prior()
    lp.backward()
    assert float(lp.detach()) == pytest.approx(float(z["correlatedclassificationconvnet|log_prior"]), rel=1e-12)
    for n, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), z["correlatedclassificationconvnet|grad:" + n], rtol=1e-10, atol=1e-12)


@pytest.mark.skipif(not os.path.isdir(REFERENCE_ROOT), reason="the reference is not on this machine")
def test_generator_reproduces_its_fixture(golden_dir, tmp_path):
    import subprocess
    import sys
    out = tmp_path / "correlated_models.npz"
    subprocess.check_call([sys.executable, os.path.join(golden_dir, "make_correlated_model_goldens.py"), str(out)],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    a, b = _fixture(golden_dir), np.load(out)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- GPU
def _check_potential(net, x, y, N):
    from bnn_priors_amd import mcmc, potential
    ref = copy.deepcopy(net)
    opt = mcmc.VerletSGLD(net.parameters(), lr=1e-4, num_data=N, momentum=0.9, temperature=1.0, seed=3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        pot = potential.Potential(net, opt, N)
    assert pot.fast and pot.leftover == []
    assert not [w for w in caught if "differentiated by autograd" in str(w.message)]
    assert opt.engine.filter_host is not None
    loss, log_prior, pot_value, acc = pot.minibatch(x, y, True)
    _, lp_ref, potential_ref, _, _ = ref.split_potential_and_acc(x, y, N)
    potential_ref.backward()
    assert float(log_prior) == pytest.approx(float(lp_ref.detach()), rel=2e-5, abs=1e-3)
    assert float(pot_value) == pytest.approx(float(potential_ref), rel=2e-5, abs=1e-5)
    for (n_, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        want = q.grad if q.grad is not None else torch.zeros_like(q)
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        torch.testing.assert_close(got, want, rtol=2e-4, atol=2e-6, msg=lambda m: f"{n_}: {m}")
    opt.sample_momentum()
    opt.initial_step(save_state=False)
    assert all(torch.isfinite(p).all() for p in net.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [128, 80])
def test_correlated_googleresnet_takes_the_hook(batch):
    net, x, y = _net("correlatedgoogleresnet", "cuda:0", lengthscales=(0.5, None), n=batch)
    _check_potential(net, x, y, 50000.0)


@pytest.mark.gpu
def test_correlated_convnet_takes_the_hook():
    net, x, y = _net("correlatedclassificationconvnet", "cuda:0", width=50, lengthscales=(0.5, 2.0), n=128)
    _check_potential(net, x, y, 60000.0)


@pytest.mark.gpu
def test_correlated_convnet_graph_replay_agrees_with_eager():
    """the captured step (GraphedLeapfrog, whose prior launch is the full kernel with the filter table) really captures
    and changes nothing: same accept / reject decisions, step indices and schedules bit for bit, the float metric streams
    and samples to 1e-5 relative (pattern of test_runners.py::test_graph_replay_is_bit_identical_to_eager; the
    per-segment temperature estimates of the two paths were measured to differ by ~1e-8 absolute, so bit identity is not
    asserted)"""
    import runner_cases as RC
    from bnn_priors_amd import inference_reject
    from bnn_priors_amd.storage import MemoryMetrics
    cfg = dict(RC.CASES["VerletSGLDReject"], n=512)
    outs = []
    for use_graph in (False, True):
        dev = "cuda:0"
        train, test, (x, y) = RC.make_data(dev, cfg)
        torch.manual_seed(0)
        model = models.get_model(x, y, "correlatedclassificationconvnet", width=50, depth=3, weight_prior="convcorrnormal",
                                 weight_loc=0., weight_scale=2 ** .5, bias_prior="gaussian", bias_scale=1.,
                                 weight_prior_params={"lengthscale_1": 0.5, "lengthscale_2": 1.0})
        torch.manual_seed(1)
        models.he_initialize(model)
        model = model.to(dev)
        metrics = MemoryMetrics()
        torch.manual_seed(RC.SEED)
        runner = inference_reject.VerletSGLDRunnerReject(
            model=model, dataloader=train, dataloader_test=test, learning_rate=cfg["lr"],
            temperature=cfg["temperature"], momentum=cfg["momentum"], reject_samples=True,
            metrics_saver=metrics, model_saver=None, seed=RC.SEED, chain_id=0,
            cycle_seed=RC.CYCLE_SEED, use_graph=use_graph, **RC.RUN_KW)
        runner.run()
        assert (runner._graphed not in (None, False)) == use_graph
        assert runner.optimizer.engine.filter_host is not None
        outs.append((RC.streams_of(metrics), {k: v.clone() for k, v in runner.get_samples().items()}))
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
        torch.testing.assert_close(p1[k], p0[k], rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
