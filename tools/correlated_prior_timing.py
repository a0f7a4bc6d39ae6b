"""Leapfrog steps per second of googleresnet (Normal priors) and of correlatedgoogleresnet (ConvCorrelatedNormal on the
21 convolutions, lengthscale 0.5) in ONE process, batch 128, float32:

* ``googleresnet``             -- the captured step (GraphedLeapfrog), Normal priors in the update kernel's in-flight prior;
* ``correlated_hook``          -- the captured step, the filter priors in one full prior launch (SGMCMC_PRIOR_FILTER_WHITENED);
* ``correlated_autograd``      -- ``fused_filter_spec`` patched to None: the priors are Potential.leftover, differentiated
                                  by autograd through MultivariateNormal, no capture (eager steps).

    python tools/correlated_prior_timing.py [--steps 200] [--warmup 30] [--out profiles/correlated_prior_timing.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip, graphed, mcmc, models, potential  # noqa: E402
from bnn_priors_amd import prior as P  # noqa: E402


def _setup(name, weight_prior, kw, dev, N, batch):
    torch.manual_seed(0)
    x0, y0 = torch.rand(16, 3, 32, 32), torch.arange(16) % 10
    net = models.get_model(x0, y0, name, weight_prior=weight_prior, weight_loc=0., weight_scale=2 ** .5,
                           bias_prior="gaussian", bias_scale=1., weight_prior_params=kw).to(dev)
    torch.manual_seed(1)
    models.he_initialize(net)
    opt = mcmc.VerletSGLD(net.parameters(), lr=1e-4, num_data=N, momentum=0.98, temperature=1.0, seed=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pot = potential.Potential(net, opt, N)
    x = torch.rand(batch, 3, 32, 32, device=dev)
    y = torch.arange(batch, device=dev) % 10
    return net, opt, pot, x, y


def _time(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def run(case, steps, warmup, dev="cuda:0", N=50000.0, batch=128):
    name, prior, kw = (("googleresnet", "gaussian", {}) if case == "googleresnet"
                       else ("correlatedgoogleresnet", "convcorrnormal", {"lengthscale": 0.5}))
    net, opt, pot, x, y = _setup(name, prior, kw, dev, N, batch)
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
    return dict(case=case, route=route, leftover=len(pot.leftover or []), prior_flags=int(opt.engine.layout.prior_flags),
                us_per_step=s * 1e6, steps_per_s=1.0 / s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("googleresnet", a.steps, a.warmup), run("correlated_hook", a.steps, a.warmup)]
    saved = P.ConvCorrelatedNormal.fused_filter_spec
    P.ConvCorrelatedNormal.fused_filter_spec = lambda self: None        # the autograd route, same process
    try:
        rows.append(run("correlated_autograd", max(20, a.steps // 5), max(5, a.warmup // 3)))
    finally:
        P.ConvCorrelatedNormal.fused_filter_spec = saved
    base = rows[0]["steps_per_s"]
    for r in rows:
        r["vs_googleresnet"] = r["steps_per_s"] / base
        print(json.dumps(r), flush=True)
    out = dict(source_sha=_hip.source_sha(), library_sha=_hip.library_sha(), device=torch.cuda.get_device_name(0),
               batch=128, dtype="float32", steps=a.steps, warmup=a.warmup, rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
