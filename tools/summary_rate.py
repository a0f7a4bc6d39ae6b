"""Time of ``diagnostics.posterior_summary`` (csrc/summary_hip.inc and the ESS / indicator entries it reuses) at the
shape of a stored run -- 4 chains x 300 draws x 270,000 fp32 quantities (googleresnet's weights), iid normal draws, the
default arguments: three quantiles, the 94 % HDI, split sequences, a 256 MiB workspace (20 chunks of quantities).

* the whole call: device-event time (warm-up, then ``--reps`` calls, the median);
* the split by kernel: device time per kernel name from one profiled call (torch.profiler), summed over the chunks;
* the yardstick of the sort alone: ``torch.sort`` down the draws of the same table viewed as [1200, 270000], in fp32 as it
  is stored and in fp64 as ``sgmcmc_summary_sort`` writes it (values and indices; the sort kernel writes values only and
  pads 1200 draws to 2048).

    python tools/summary_rate.py [--reps 5] [--out profiles/summary_rate.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from bnn_priors_amd import _hip, diagnostics  # noqa: E402

M, S, Q = 4, 300, 270000


def _event_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_rate.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((M, S, Q), generator=g, dtype=torch.float32, device=dev)
    lines = [f"library source hash {_hip.library_sha()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"posterior_summary, {M} x {S} x {Q} fp32 ({x.numel() * 4 / 1e9:.2f} GB), default arguments, "
             f"median of {args.reps} calls"]
    lines.append(f"  whole call                      {_event_ms(lambda: diagnostics.posterior_summary(x), args.reps):9.2f} ms")
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        diagnostics.posterior_summary(x)
        torch.cuda.synchronize()
    rows = []
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
        if t:
            rows.append((t / 1000.0, e.count, e.key.split("(")[0].replace("void ", "")))
    lines.append("  by kernel (one profiled call):      ms   launches")
    for t, count, name in sorted(rows, reverse=True):
        lines.append(f"    {name:<34}{t:9.2f} {count:6d}")
    flat = x.reshape(M * S, Q)
    lines.append(f"torch.sort(dim=0) of the table as [{M * S}, {Q}], median of {args.reps} calls")
    lines.append(f"  fp32                            {_event_ms(lambda: torch.sort(flat, dim=0), args.reps):9.2f} ms")
    wide = flat.double()
    lines.append(f"  fp64                            {_event_ms(lambda: torch.sort(wide, dim=0), args.reps):9.2f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
