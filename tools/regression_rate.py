"""Time of the regression scores (``regression.predictive``: ``sgmcmc_gmix_rows``, the pair sum of the mixture CRPS and
the per-entry pass; ``regression.quantiles``; ``regression.pit_calibration``; csrc/regress_hip.inc) at the shapes of a
UCI run: 1,000 samples on 1,000 rows and on 50 rows (a UCI test split: the case the pair sum is split over workgroups
for), one output, one noise level per sample.

Device times are device events around ``--reps`` calls after a warm-up call, profiler off, taken ``--windows`` times
(the spread is printed).  ``predictive`` with targets evaluates N D E (E - 1) / 2 pair terms (one erf, one exp, one
square root and one division each, fp64), which is what the rate counts; without targets it does not form the pair sum,
so the difference of the two is the pair sum's own time.  The tables are 8 MB at most: nothing here is bound by memory.

    python tools/regression_rate.py [--reps 10] [--windows 5] [--out profiles/regression_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip  # noqa: E402
from bnn_priors_amd import regression as reg  # noqa: E402

SHAPES = ((1000, 1000, 1), (1000, 50, 1))
PROBS = (0.025, 0.05, 0.25, 0.75, 0.95, 0.975)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regression_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "regression_rate.py measures on the GPU"
    dev = "cuda:0"
    lines = [f"regression scores, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (sources {_hip.source_sha()}), "
             f"device events, {a.windows} windows of {a.reps} calls: median (least .. largest)",
             f"{'call':44s} {'ms/call':>28s} {'workgroups':>11s} {'pair terms':>11s} {'G terms/s':>10s}"]

    def row(what, ms, groups="", terms=None):
        med, lo, hi = ms
        rate = "" if terms is None else f"{terms / (med * 1e-3) * 1e-9:10.2f}"
        lines.append(f"{what:44s} {f'{med:.4f} ({lo:.4f} .. {hi:.4f})':>28s} {groups!s:>11s} "
                     f"{'' if terms is None else f'{terms:.3g}':>11s} {rate:>10s}")
        print(lines[-1], flush=True)

    for E, N, D in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        mean = torch.randn((E, N, D), generator=g, dtype=torch.float64, device=dev)
        scale = 0.5 + torch.rand(E, generator=g, dtype=torch.float64, device=dev)
        y = torch.randn((N, D), generator=g, dtype=torch.float64, device=dev)
        name = f"{E} x {N} x {D}"
        terms = N * D * E * (E - 1) // 2
        with_y = _event_ms(lambda: reg.predictive(mean, scale, y), a.reps, a.windows)
        row(f"predictive {name}, with y", with_y, N * D * reg.pair_split(E, N, D), terms)
        without = _event_ms(lambda: reg.predictive(mean, scale), a.reps, a.windows)
        row(f"predictive {name}, without y", without)
        row(f"quantiles {name}, {len(PROBS)} levels", _event_ms(lambda: reg.quantiles(mean, scale, PROBS), a.reps, a.windows))
        pit = reg.predictive(mean, scale, y).pit[:, 0].contiguous()
        row(f"pit_calibration {N} rows (with its read-back)", _event_ms(lambda: reg.pit_calibration(pit), a.reps, a.windows))
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
