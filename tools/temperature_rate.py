"""Time of the temperature diagnostics (``temperature.chi2_interval`` / ``kinetic_coverage`` / ``weighted_temperature`` /
``ewma`` / ``chi2_tails``; csrc/temper_hip.inc) at the shape of a long googleresnet run: S = 100,000 metrics rows of K = 65
parameter tensors (1 to 36,864 elements, and one of 78,400), C = 5 confidence levels -- against the numpy / scipy
restatement of the reference's plot.py (``chi2.ppf``, the masked comparisons, ``weighted_var_se``, ``lfilter``) on the
same host.

Device times are device events around ``--reps`` calls after a warm-up call, profiler off, taken ``--windows`` times
(the spread is printed); the table is on the device already (what ``temperature_report`` uploads once).  The host
times are wall clock, the median of ``--windows`` calls -- of ``max(1, windows // 2)`` calls for the ``chi2.logcdf`` /
``logsf`` row, which takes seconds per call; that row says so.

    python tools/temperature_rate.py [--reps 10] [--windows 5] [--out profiles/temperature_rate.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bnn_priors_amd import _hip  # noqa: E402
from bnn_priors_amd import temperature as tp  # noqa: E402

S, K, ALPHA = 100_000, 65, 0.99


def _event_ms(fn, reps, windows):
    "ms per call: the median, the least and the largest of ``windows`` windows of ``reps`` calls"
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def _host_ms(fn, windows):
    out = []
    for _ in range(windows):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temperature_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "temperature_rate.py measures on the GPU"
    import scipy.signal
    import scipy.stats
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    sizes = [1, 78400] + [int(v) for v in rng.choice([16, 32, 64, 2304, 4608, 9216, 18432, 36864], size=K - 2)]
    conf = np.array(tp.CONFIDENCES)
    est_host = np.stack([rng.chisquare(d, size=S) / d for d in sizes], axis=1)
    temp_host = np.ones(S)
    est, temp = torch.from_numpy(est_host).to(dev), torch.from_numpy(temp_host).to(dev)
    bounds = tp.chi2_interval(sizes, tp.CONFIDENCES, device=dev)
    share = tp.kinetic_coverage(est, temp, sizes, bounds=bounds)[0]

    def host_intervals():
        return [(scipy.stats.chi2.ppf((1 - conf) / 2, df=d, scale=1 / d), scipy.stats.chi2.ppf((1 + conf) / 2, df=d, scale=1 / d))
                for d in sizes]
    host_bounds = host_intervals()

    def host_coverage():
        counts = np.zeros((len(conf), S))
        for k in range(K):
            r = est_host[:, k] / temp_host
            lo, hi = host_bounds[k]
            counts += np.logical_and(lo[:, None] <= r, r <= hi[:, None]).astype(float)
        return counts / K
    host_share = host_coverage()
    w = np.array(sizes, dtype=float)

    def host_weighted():
        x, n = est_host, K
        xw = (x @ w) / w.sum()
        wb = w.mean()
        e = w * x - wb * xw[..., None]
        return xw, n / ((n - 1) * w.sum() ** 2) * ((e ** 2).sum(-1) - 2 * xw * (e @ (w - wb)) + xw ** 2 * ((w - wb) @ (w - wb)))

    def host_ewma():
        b, c = [1 - ALPHA], [1, -ALPHA]
        return [scipy.signal.lfilter(b, c, row, zi=scipy.signal.lfiltic(b, c, row[0:1], [0]))[0] for row in host_share]

    lines = [f"temperature diagnostics, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (sources "
             f"{_hip.source_sha()}), S = {S} steps, K = {K} tensors (sizes 1 .. 78400), C = {len(conf)} levels, fp64; device "
             f"events, {a.windows} windows of {a.reps} calls; host: numpy {np.__version__} / scipy {scipy.__version__}, wall "
             f"clock, {a.windows} calls unless the row says otherwise: median (least .. largest)",
             f"{'call':58s} {'device ms':>30s} {'host restatement ms':>34s}"]

    def row(what, dev_ms, host_ms=None):
        fmt = lambda m: f"{m[0]:.4f} ({m[1]:.4f} .. {m[2]:.4f})"
        lines.append(f"{what:58s} {fmt(dev_ms):>30s} {fmt(host_ms) if host_ms else '':>34s}")
        print(lines[-1], flush=True)

    row("chi2_interval: K x C x 2 quantiles", _event_ms(lambda: tp.chi2_interval(sizes, tp.CONFIDENCES, device=dev), a.reps, a.windows),
        _host_ms(host_intervals, a.windows))
    row("kinetic_coverage: step table + per-tensor counts + EWMA", _event_ms(lambda: tp.kinetic_coverage(est, temp, sizes, ewma_alpha=ALPHA, bounds=bounds), a.reps, a.windows),
        _host_ms(lambda: (host_coverage(), host_ewma()), a.windows))
    row("weighted_temperature: mean and Cochran's se per step", _event_ms(lambda: tp.weighted_temperature(est, sizes), a.reps, a.windows),
        _host_ms(host_weighted, a.windows))
    row(f"ewma of the [C, S] shares, alpha = {ALPHA}", _event_ms(lambda: tp.ewma(share, ALPHA), a.reps, a.windows),
        _host_ms(host_ewma, a.windows))
    few = max(1, a.windows // 2)
    row(f"chi2_tails: PIT, both log-tails, S x K elements (host: {few} calls)", _event_ms(lambda: tp.chi2_tails(est, sizes), a.reps, a.windows),
        _host_ms(lambda: [(scipy.stats.chi2.logcdf(est_host[:, k], df=d, scale=1 / d), scipy.stats.chi2.logsf(est_host[:, k], df=d, scale=1 / d))
                          for k, d in enumerate(sizes)], few))
    same = bool((share.cpu().numpy() == host_share).all())
    lines.append(f"coverage shares, device == host restatement at all {len(conf) * S} entries: {same} (scipy's interval ends are up to "
                 "9.6 eps from the 50-digit ones, the device's one rounding: a count can differ where an estimate sits on an end)")
    mean, se = (v.cpu().numpy() for v in tp.weighted_temperature(est, sizes))
    hm, hs = host_weighted()
    lines.append(f"weighted mean / se, largest relative distance device vs host: {np.max(np.abs(mean - hm) / hm):.2e} / "
                 f"{np.max(np.abs(se - hs) / hs):.2e} (the host's three-term se cancels; the device sums w^2 (x - mean)^2)")
    print("\n".join(lines[-2:]))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
