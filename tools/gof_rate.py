"""Time of the goodness-of-fit statistics (``goodness_of_fit.goodness_of_fit``: csrc/gof_hip.inc) at the size they are used
at: one pooled layer of the headline net, S = 300 samples of 270,000 weights in fp32 (81 M values, 324 MB), scored under
all five families of ``prior_fit.fit_marginal`` at once.

Reported separately: the ``torch.sort`` that orders the values (plumbing: every statistic is a function of the sorted
array), the statistics launch (one pass that loads every value once and evaluates the five families on it, and the
workgroup that adds the partials), the Q-Q launch at K = 4096, and the same statistics with scipy on this host's CPU
(``<family>.cdf`` / ``logcdf`` / ``logsf`` and the sums in numpy) at a SUBSAMPLE whose size is stated, with the time that
extrapolates to per value.  Device events; one warm-up call, then the median (least .. largest) of ``--windows`` windows
of ``--reps`` repetitions.

    python tools/gof_rate.py [--reps 3] [--windows 5] [--subsample 200000] [--out profiles/gof_rate.txt]
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
from bnn_priors_amd import goodness_of_fit as gof  # noqa: E402
from bnn_priors_amd.calibration import _stream  # noqa: E402

S, WEIGHTS, DF, SCALE = 300, 270_000, 4.0, 0.05
# what fit_marginal returns for such a stack, to three digits (the time does not depend on the digits)
FITS = {"norm": (0.0, 0.0707), "laplace": (0.0, 0.05), "t": (4.0, 0.0, 0.05), "gennorm": (0.95, 0.0, 0.046),
        "dgamma": (0.98, 0.0, 0.051)}


def _event_ms(fn, reps, windows):
    "ms per repetition: the median, the least and the largest of ``windows`` windows, after one warm-up call"
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


def _scipy_statistics(x, fits):
    "the statistics of the ascending x under every family, with scipy's distribution functions"
    import scipy.stats
    n = len(x)
    i = np.arange(1, n + 1)
    out = {}
    for fam, params in fits.items():
        dist = getattr(scipy.stats, fam)(*params)
        with np.errstate(divide="ignore"):
            F, lF, lS = dist.cdf(x), dist.logcdf(x), dist.logsf(x)
        out[fam] = (max(np.max(i / n - F), np.max(F - (i - 1) / n)), 1 / (12 * n) + np.sum((F - (2 * i - 1) / (2 * n)) ** 2),
                    -n - np.sum((2 * i - 1) * lF + (2 * (n - i) + 1) * lS) / n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--subsample", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gof_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gof_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    lib = _hip.lib()
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    n = S * WEIGHTS
    mix = torch.distributions.Gamma(torch.tensor(DF / 2, device=dev), torch.tensor(DF / 2, device=dev)).sample((n,))
    w = (SCALE * torch.randn(n, generator=g, device=dev) / mix.sqrt()).reshape(S, WEIGHTS).contiguous()
    del mix
    count = len(FITS)
    records = (_hip.GofRecord * count)(*[gof._record(fam, params)[0] for fam, params in FITS.items()])
    ordered, _ = torch.sort(w.reshape(-1))
    work = torch.empty(lib.sgmcmc_gof_workspace_doubles(n), dtype=torch.float64, device=dev)
    out = torch.empty(count * _hip.GOF_OUT, dtype=torch.float64, device=dev)
    K = gof.MAX_QQ_POINTS
    qq = torch.empty((count + 1) * K, dtype=torch.float64, device=dev)

    def statistics():
        _hip.check(lib.sgmcmc_gof_statistics(ordered.data_ptr(), _hip.F32, n, records, count, work.data_ptr(),
                                             out.data_ptr(), _stream()), "sgmcmc_gof_statistics")

    def quantiles():
        _hip.check(lib.sgmcmc_gof_ppf(ordered.data_ptr(), _hip.F32, n, records, count, K, qq.data_ptr(),
                                      qq[count * K:].data_ptr(), _stream()), "sgmcmc_gof_ppf")

    lines = [f"goodness of fit, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (source_sha "
             f"{_hip.source_sha()}), {S} x {WEIGHTS} fp32 = {n} values ({n * 4 / 1e6:.0f} MB), {count} families "
             f"{tuple(FITS)}, device events, one warm-up call, {a.windows} windows of {a.reps}: median (least .. largest)"]

    def row(what, ms, extra=""):
        lines.append(f"{what:58s} {ms[0]:10.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f}){extra}")
        print(lines[-1], flush=True)

    row("torch.sort of the flattened values", _event_ms(lambda: torch.sort(w.reshape(-1)), a.reps, a.windows))
    stat = _event_ms(statistics, a.reps, a.windows)
    row("statistics launch (KS, CvM, AD of 5 families, one pass)", stat,
        f"  {stat[0] * 1e6 / (n * count):.3f} ns per value and family")
    row(f"Q-Q launch (K = {K} model and empirical quantiles)", _event_ms(quantiles, a.reps, a.windows))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = gof.goodness_of_fit(w, fits=FITS)
    whole = (time.perf_counter() - t0) * 1e3
    lines.append(f"{'goodness_of_fit(w, fits) as called (host clock, sorts, reads back)':58s} {whole:10.3f} ms")
    # the kernels at this size against torch ops in fp64 on the same sorted array, for the family with closed forms
    loc, scale = FITS["laplace"]
    z = (ordered.to(torch.float64) - loc) / scale
    lt = -z.abs() - torch.log(torch.tensor(2.0, dtype=torch.float64, device=dev))
    up = z > 0
    lF, lS = torch.where(up, torch.log1p(-lt.exp()), lt), torch.where(up, lt, torch.log1p(-lt.exp()))
    F = torch.where(up, -torch.expm1(lt), lt.exp())
    i = torch.arange(1, n + 1, dtype=torch.float64, device=dev)
    ks = max(float((i / n - F).max()), float((F - (i - 1) / n).max()))
    cvm = 1 / (12 * n) + float(((F - (2 * i - 1) / (2 * n)) ** 2).sum())
    ad = -n - float(((2 * i - 1) * lF + (2 * (n - i) + 1) * lS).sum()) / n
    lap = table["laplace"]
    lines.append(f"laplace at all {n} values, kernel | torch ops (fp64, pairwise sums): D {lap.ks:.12g} | {ks:.12g}, "
                 f"W^2 {lap.cvm:.12g} | {cvm:.12g}, A^2 {lap.ad:.12g} | {ad:.12g}")
    del z, lt, up, lF, lS, F, i
    m = min(a.subsample, n)
    sub = np.sort(w.reshape(-1)[torch.randperm(n, generator=g, device=dev)[:m]].cpu().numpy().astype(np.float64))
    _scipy_statistics(sub[:1000], FITS)                       # warm-up: imports and scipy's first-call work
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        host = _scipy_statistics(sub, FITS)
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    lines.append(f"{f'scipy on the host CPU, SUBSAMPLE of {m} sorted values':58s} {times[1]:10.3f} ms ({times[0]:.3f} .. "
                 f"{times[2]:.3f})  {times[1] * 1e6 / (m * count):.1f} ns per value and family; at {n} values: "
                 f"{times[1] * n / m / 1e3:.1f} s = {times[1] * n / m / stat[0]:.0f} x the statistics launch")
    lines.append("A^2 per family, device (all values) | scipy (subsample): "
                 + ", ".join(f"{fam} {table[fam].ad:.4g} | {host[fam][2]:.4g}" for fam in FITS))
    print("\n".join(lines[-4:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
