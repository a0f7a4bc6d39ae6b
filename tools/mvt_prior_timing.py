"""Leapfrog steps per second of googleresnet (Normal priors) and of decreasing_mvt_googleresnet (weight_prior gaussian:
MultivariateT on the stem and blocks 3-6, events = input channels) in ONE process, batch 128, float32:

* ``googleresnet``       -- the captured step (GraphedLeapfrog), Normal priors in the update kernel's in-flight prior;
* ``mvt_hook``           -- the captured step, the multivariate-t priors in the event-sum launch + the full prior launch
                            (SGMCMC_PRIOR_MULTIVARIATE_T);
* ``mvt_autograd``       -- ``fused_mvt_spec`` patched to None: the ten priors are Potential.leftover, differentiated by
                            autograd, no capture (eager steps).

    python tools/mvt_prior_timing.py [--steps 200] [--warmup 30] [--out profiles/mvt_prior_timing.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bnn_priors_amd import _hip, graphed  # noqa: E402
from bnn_priors_amd import prior as P  # noqa: E402
from correlated_prior_timing import _setup, _time  # noqa: E402


def run(case, steps, warmup, dev="cuda:0", N=50000.0, batch=128):
    name = "googleresnet" if case == "googleresnet" else "decreasing_mvt_googleresnet"
    net, opt, pot, x, y = _setup(name, "gaussian", {}, dev, N, batch)
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
    rows = [run("googleresnet", a.steps, a.warmup), run("mvt_hook", a.steps, a.warmup)]
    saved = P.MultivariateT.fused_mvt_spec
    P.MultivariateT.fused_mvt_spec = lambda self: None        # the autograd route, same process
    try:
        rows.append(run("mvt_autograd", max(20, a.steps // 5), max(5, a.warmup // 3)))
    finally:
        P.MultivariateT.fused_mvt_spec = saved
    base = rows[0]["steps_per_s"]
    for r in rows:
        r["vs_googleresnet"] = r["steps_per_s"] / base
        print(json.dumps(r), flush=True)
    out = dict(source_sha=_hip.source_sha(), library_sha=_hip.library_sha(), device=torch.cuda.get_device_name(0),
               batch=128, dtype="float32", steps=a.steps, warmup=a.warmup, rows=rows,
               hook_vs_autograd=rows[1]["steps_per_s"] / rows[2]["steps_per_s"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
