"""Time of the evaluation's two phases for googleresnet, E = 20 seeded samples, a 10,000-row in-distribution set and a
26,032-row out-of-distribution set (the sizes of CIFAR-10 test / SVHN test), one process:

* ``forward``  -- ``evaluation.logit_tables``: per sample, the captured forwards over both sets into the fp64
                  [E, N, C] tables;
* ``metrics``  -- everything after the tables (calibration.py): the ensemble probabilities of both tables, ece / ace /
                  rmsce of the in-distribution set and AUROC / AUPRC of in- against out-of-distribution max-probs.

Each phase is warmed up once, then timed ``--repeats`` times (host clock around work that ends in a device
synchronise); the median is reported with the metric phase's share of the whole evaluation.

    python tools/eval_metrics_timing.py [--repeats 5] [--out profiles/eval_metrics_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip, calibration, evaluation, models  # noqa: E402


def _setup(dev, E, n_in, n_out):
    torch.manual_seed(0)
    x = torch.rand(n_in, 3, 32, 32)
    y = torch.arange(n_in) % 10
    net = models.get_model(x[:16], y[:16], "googleresnet", weight_prior="gaussian", weight_loc=0., weight_scale=2 ** .5,
                           bias_prior="gaussian", bias_loc=0., bias_scale=1., batchnorm=True, weight_prior_params={},
                           bias_prior_params={})
    models.he_initialize(net)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    samples = {}
    for k, v in net.state_dict().items():
        if v.is_floating_point():
            noise = 0.05 * torch.randn((E,) + tuple(v.shape), generator=g).to(dev)
            samples[k] = (v.unsqueeze(0) + noise * v.abs().mean()).clone()
            if k.endswith("running_var"):
                samples[k] = samples[k].abs() + 0.5
        else:
            samples[k] = v.unsqueeze(0).repeat((E,) + (1,) * v.dim())
    x_out = torch.rand((n_out, 3, 32, 32), generator=g) * 2 - 0.5
    loader_in = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x.to(dev), y.to(dev)), batch_size=128)
    loader_out = torch.utils.data.DataLoader(
        torch.utils.data.TensorDataset(x_out.to(dev), torch.zeros(n_out, dtype=torch.int64, device=dev)), batch_size=128)
    return net, loader_in, loader_out, samples, y.to(dev)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics_timing.json"))
    a = ap.parse_args()
    dev, n_in, n_out = "cuda:0", 10000, 26032
    net, loader_in, loader_out, samples, labels = _setup(dev, a.samples, n_in, n_out)

    def forward():
        return evaluation.logit_tables(net, (loader_in, loader_out), samples)

    def metrics(tables):
        acc_in, acc_out = tables
        ens_in = calibration.ensemble_probs(acc_in, labels)
        res = calibration.calibration_metrics(labels, ens_in.probs)
        res["auroc"], res["auprc"] = calibration.auroc_auprc(ens_in.conf, calibration.ensemble_probs(acc_out).conf)
        return res

    tables = forward()                        # warm-up: graph captures, first launches
    res = metrics(tables)
    t_fwd, t_met = [], []
    for _ in range(a.repeats):
        s, tables = _timed(forward)
        t_fwd.append(s)
        s, again = _timed(lambda: metrics(tables))
        t_met.append(s)
        assert again == res                   # deterministic: the same bits every time
    fwd, met = statistics.median(t_fwd), statistics.median(t_met)
    out = dict(source_sha=_hip.source_sha(), library_sha=_hip.library_sha(), device=torch.cuda.get_device_name(0),
               model="googleresnet", samples=a.samples, rows_in=n_in, rows_out=n_out, classes=10,
               table_bytes=8 * a.samples * (n_in + n_out) * 10, repeats=a.repeats,
               forward_ms=fwd * 1e3, metrics_ms=met * 1e3, metrics_fraction=met / (fwd + met),
               forward_ms_all=[t * 1e3 for t in t_fwd], metrics_ms_all=[t * 1e3 for t in t_met], results=res)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
