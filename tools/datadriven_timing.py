"""Leapfrog steps per second of the data-driven MNIST convnets next to classificationconvnet, in ONE process, width 50,
batch 128, float32, N = 60000 (the fitted tables are the fixture subset in tests/golden/datadriven.npz):

* ``classificationconvnet``       -- Normal priors, the captured step (GraphedLeapfrog);
* ``gauss_hook``                  -- datadrivengaussconv: FixedCovNormal convolutions in the full prior launch
                                     (SGMCMC_PRIOR_FILTER_WHITENED), Normal head and biases: every prior in the hook, captured;
* ``doublegamma_hook``            -- datadrivendoublegammaconv: the Laplace / double-Gamma filter bases in the hook, the
                                     head's element-wise DoubleGamma in autograd (Potential.leftover): eager steps;
* ``doublegamma_autograd``        -- the same model with every prior forced to autograd (``fused_spec`` and
                                     ``fused_filter_spec`` patched to None): eager steps.

    python tools/datadriven_timing.py [--steps 200] [--warmup 30] [--out profiles/datadriven_timing.json]
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bnn_priors_amd import _hip, graphed, mcmc, models, potential  # noqa: E402
from bnn_priors_amd import prior as P  # noqa: E402
from correlated_prior_timing import _time  # noqa: E402
from test_datadriven_models import fixture_prior_data  # noqa: E402

MODEL = dict(classificationconvnet="classificationconvnet", gauss_hook="datadrivengaussconv",
             doublegamma_hook="datadrivendoublegammaconv", doublegamma_autograd="datadrivendoublegammaconv")


def run(case, steps, warmup, data, dev="cuda:0", N=60000.0, batch=128):
    torch.manual_seed(0)
    x0, y0 = torch.rand(16, 784), torch.arange(16) % 10
    net = models.get_model(x0, y0, MODEL[case], width=50, depth=3, weight_prior="gaussian", weight_loc=0.,
                           weight_scale=2 ** .5, bias_prior="gaussian", bias_scale=1., prior_data=data).to(dev)
    torch.manual_seed(1)
    models.he_initialize(net)
    opt = mcmc.VerletSGLD(net.parameters(), lr=1e-4, num_data=N, momentum=0.98, temperature=1.0, seed=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pot = potential.Potential(net, opt, N)
    x = torch.rand(batch, 784, device=dev)
    y = torch.arange(batch, device=dev) % 10
    opt.sample_momentum()
    pot.minibatch(x, y, False)
    opt.initial_step(save_state=False, calc_metrics=False)
    if pot.leftover:
        def step():
            pot.minibatch(x, y, False)
            opt.step(calc_metrics=False)
        route = "eager"
    else:
        g = graphed.GraphedLeapfrog(pot, opt, x, y)

        def step():
            g.replay(x, y)
        route = "graph"
    s = _time(step, steps, warmup)
    return dict(case=case, model=MODEL[case], route=route, leftover=len(pot.leftover or []),
                filter_segments=int((opt.engine.seg_host["prior_kind"] == _hip.PRIOR_FILTER_WHITENED).sum()),
                prior_flags=int(opt.engine.layout.prior_flags), us_per_step=s * 1e6, steps_per_s=1.0 / s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    data = fixture_prior_data(np.load(os.path.join(ROOT, "tests", "golden", "datadriven.npz")))
    rows = [run(c, a.steps, a.warmup, data) for c in ("classificationconvnet", "gauss_hook", "doublegamma_hook")]
    saved = P.Prior.fused_spec, P.ConvCovariance.fused_filter_spec
    P.Prior.fused_spec = P.ConvCovariance.fused_filter_spec = lambda self: None      # the autograd route, same process
    try:
        rows.append(run("doublegamma_autograd", a.steps, a.warmup, data))
    finally:
        P.Prior.fused_spec, P.ConvCovariance.fused_filter_spec = saved
    base = rows[0]["steps_per_s"]
    for r in rows:
        r["vs_classificationconvnet"] = r["steps_per_s"] / base
        print(json.dumps(r), flush=True)
    out = dict(source_sha=_hip.source_sha(), library_sha=_hip.library_sha(), device=torch.cuda.get_device_name(0),
               width=50, batch=128, dtype="float32", steps=a.steps, warmup=a.warmup, rows=rows,
               gauss_vs_classificationconvnet=rows[1]["steps_per_s"] / rows[0]["steps_per_s"],
               doublegamma_hook_vs_autograd=rows[2]["steps_per_s"] / rows[3]["steps_per_s"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
