"""Aggregate leapfrog steps per second of K = 8 lock-step chains of classificationdensenet (784-50-50-10, batch 128,
float32, metric read-back every 10th step: the shapes of bench.py's chains-per-launch sweep), two or three legs on the SAME
chains in ONE process:

* ``uniform``  -- every chain at T = 1: one 128-byte block of scalars for all (``sgmcmc_dense_step_multi``);
* ``ladder``   -- the chains at eight temperatures: one block per chain, 1 KiB of kernel arguments
                  (``sgmcmc_dense_step_multi_args``);
* ``parent_uniform`` (with ``--parent-fused-dense FILE``) -- every chain at T = 1 through the ``MultiChainDense`` of
                  ANOTHER commit's ``bnn_priors_amd/fused_dense.py`` (``git show COMMIT:bnn_priors_amd/fused_dense.py >
                  FILE``), loaded beside this tree's and run on this tree's library: the one-block call as it was
                  issued before there were per-chain blocks, i.e. without the comparisons that choose between the two.

The legs alternate (``--pairs`` times, uniform first) so that drift of the box hits both; per leg the median and the
spread (min .. max) of the blocks are reported, and the time the host spends inside ``MultiChainDense.step`` on the
steps without read-back (where the difference between the legs is made: K blocks built instead of one).

    python tools/dense_ladder_rate.py [--pairs 6] [--steps 600] [--warmup 60] [--parent-fused-dense FILE]
                                      [--out profiles/dense_ladder_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bnn_priors_amd import _hip, models  # noqa: E402
from bnn_priors_amd.fused_dense import MultiChainDense  # noqa: E402
from bnn_priors_amd.inference_reject import runner_class  # noqa: E402
from bnn_priors_amd.storage import MemoryMetrics  # noqa: E402

K, BATCH, ROWS = 8, 128, 8192
TEMPERATURES = (1.0, 0.5, 0.2, 0.1, 0.05, 0.02, 0.01, 0.0)


def chain(c, dev):
    g = torch.Generator().manual_seed(1234 + c)
    x = torch.rand(ROWS, 784, generator=g).to(dev)
    y = torch.randint(0, 10, (ROWS,), generator=g).to(dev)
    mk = torch.utils.data.TensorDataset
    train = torch.utils.data.DataLoader(mk(x, y), batch_size=BATCH, shuffle=True)
    empty = torch.utils.data.DataLoader(mk(x[:0], y[:0]), batch_size=BATCH)
    torch.manual_seed(c)
    model = models.get_model(x.cpu()[:2], torch.tensor([0, 9]), "classificationdensenet", width=50, depth=3,
                             weight_prior="gaussian", weight_scale=2 ** .5, bias_prior="gaussian", bias_scale=1.)
    models.he_initialize(model)
    r = runner_class("VerletSGLDReject")(
        model=model.to(dev), dataloader=train, dataloader_test=empty, epochs_per_cycle=50, warmup_epochs=45,
        sample_epochs=5, learning_rate=0.01, skip=1, metrics_skip=10, temperature=1.0, momentum=0.994,
        sampling_decay="cosine", cycles=60, precond_update=1, metrics_saver=MemoryMetrics(), model_saver=None,
        reject_samples=True, seed=1234, chain_id=c)
    r.begin()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--parent-fused-dense", default=None, metavar="FILE")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    runners = [chain(c, dev) for c in range(K)]
    multi = MultiChainDense([r._fused_dense() for r in runners])
    multis = {"uniform": multi, "ladder": multi}
    if a.parent_fused_dense:
        import importlib.util
        spec = importlib.util.spec_from_file_location("bnn_priors_amd._parent_fused_dense", a.parent_fused_dense)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        multis["parent_uniform"] = mod.MultiChainDense([r._fused_dense() for r in runners])
    legs_run = list(multis)
    nb = ROWS // BATCH
    idx = [[np.arange(BATCH * ((t + 7 * c) % nb), BATCH * ((t + 7 * c) % nb) + BATCH, dtype=np.int64) for c in range(K)]
           for t in range(64)]
    calls = {"sgmcmc_dense_step_multi": 0, "sgmcmc_dense_step_multi_args": 0}

    def set_leg(leg):
        for r, T in zip(runners, TEMPERATURES):
            r.optimizer.param_groups[0]["temperature"] = T if leg == "ladder" else 1.0

    def run(n, t0, host=None, leg="uniform"):
        step = multis[leg].step
        for t in range(t0, t0 + n):
            m = t % 10 == 0
            h0 = time.perf_counter()
            step(idx[t % 64], metrics=m)
            if host is not None and not m:
                host.append(time.perf_counter() - h0)
            for r in runners:
                r.scheduler.step()
        return t0 + n

    def block(leg, t):
        set_leg(leg)
        t = run(a.warmup, t, None, leg)
        for r in runners:                        # (the legs' step objects do not know each other's pending blocks)
            r.optimizer.engine.flush()
        torch.cuda.synchronize(dev)
        host = []
        ts = time.perf_counter()
        t = run(a.steps, t, host, leg)
        for r in runners:
            r.optimizer.engine.flush()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - ts
        return t, dict(leg=leg, us_per_lockstep=dt / a.steps * 1e6, aggregate_steps_per_s=K * a.steps / dt,
                       host_us_in_step=statistics.mean(host) * 1e6)

    # which entry point a leg takes is a property of the scalars: count it once, outside the timed blocks
    real = multi.lib
    for leg in ("uniform", "ladder"):
        class Count:
            def __getattr__(self, name, leg=leg):
                fn = getattr(real, name)
                if name not in calls:
                    return fn

                def call(*args):
                    calls[name] += 1
                    return fn(*args)
                return call
        multi.lib = Count()
        before = dict(calls)
        set_leg(leg)
        run(3, 1)
        took = [k for k in calls if calls[k] != before[k]]
        assert took == ["sgmcmc_dense_step_multi" if leg == "uniform" else "sgmcmc_dense_step_multi_args"], took
    multi.lib = real
    t, blocks = 4, []
    for _ in range(a.pairs):
        for leg in legs_run:
            t, b = block(leg, t)
            blocks.append(b)
            print(json.dumps(b), flush=True)
    legs = {}
    for leg in legs_run:
        v = sorted(b["aggregate_steps_per_s"] for b in blocks if b["leg"] == leg)
        h = [b["host_us_in_step"] for b in blocks if b["leg"] == leg]
        legs[leg] = dict(median_steps_per_s=statistics.median(v), min_steps_per_s=v[0], max_steps_per_s=v[-1],
                         median_us_per_lockstep=K * 1e6 / statistics.median(v), median_host_us_in_step=statistics.median(h))
    out = dict(source_sha=_hip.source_sha(), library_sha=_hip.library_sha(), device=torch.cuda.get_device_name(0),
               chains=K, batch=BATCH, steps=a.steps, warmup=a.warmup, pairs=a.pairs, temperatures=TEMPERATURES,
               legs=legs, ladder_vs_uniform=legs["ladder"]["median_steps_per_s"] / legs["uniform"]["median_steps_per_s"],
               blocks=blocks)
    print(json.dumps({k: out[k] for k in ("legs", "ladder_vs_uniform")}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
