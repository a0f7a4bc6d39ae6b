"""Time of the model-comparison path (``model_comparison.loo_waic``: ``sgmcmc_psis_loo`` + ``sgmcmc_psis_totals``;
csrc/psis_hip.inc) at the shapes of a stored run:

* train table  -- 2,400 draws x 60,000 observations, fp64 (``predictive_tables`` of a training set);
* test table   -- 2,400 draws x 10,000 observations, fp32.

The log-likelihoods are -2 log1p(t^2 / 3) of student-t(3) draws generated on the device from a seed.  Per shape:

* the device-event time per call of the whole path, profiler off (one warm-up call, then ``--reps`` calls between two
  events), beside the numpy restatement (tests/psis_reference.py) timed on the first 256 columns and scaled to the
  full width;
* each kernel's own time from a run of its own under ``rocprofv3 --kernel-trace --stats`` (a fresh child process that
  makes two calls; the average per call), with the work that the shape demands of it -- stats: two passes over the
  table; select: 2 S^2 N fp64 compares (less, equal); fit: (m + 2) n2 N evaluations of log1p and n2 N of exp; finish:
  four passes over the table and the uint16 positions, and 2 S N evaluations of exp -- and the resulting rate.

    python tools/loo_rate.py [--reps 3] [--out profiles/loo_rate.txt]
"""
import argparse
import csv
import glob
import math
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from bnn_priors_amd import _hip  # noqa: E402
from bnn_priors_amd import model_comparison as mc  # noqa: E402

HOST_SLICE = 256
SHAPES = (("train 2400x60000 fp64", 2400, 60000, "float64"), ("test 2400x10000 fp32", 2400, 10000, "float32"))
KERNELS = ("stats_kernel", "select_kernel", "fit_kernel", "finish_kernel", "totals_kernel")


def _table(S, N, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.randn((S, N), generator=g, dtype=torch.float64, device=dev)
    chi = torch.zeros_like(t)
    for _ in range(3):
        chi += torch.randn((S, N), generator=g, dtype=torch.float64, device=dev) ** 2
    t /= (chi / 3.0).sqrt_()
    del chi
    return (-2.0 * torch.log1p(t * t / 3.0)).to(getattr(torch, dtype))


def _event_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _child(S, N, dtype):
    "two calls of the whole path, for the kernel trace of the parent's profiler run"
    x = _table(S, N, dtype, "cuda:0")
    for _ in range(2):
        mc.loo_waic(x)
    torch.cuda.synchronize()


def _kernel_ms(S, N, dtype):
    "{kernel: ms per call} from a traced child process, or None where the profiler is missing or its run fails"
    if shutil.which("rocprofv3") is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "loo", "--",
               sys.executable, os.path.abspath(__file__), "--child", str(S), str(N), dtype]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            print("kernel trace failed:", r.returncode, r.stderr[-2000:], flush=True)
            return None
        out = dict.fromkeys(KERNELS, 0.0)
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if "psis::" + k in row["Name"]:
                        out[k] += float(row["TotalDurationNs"]) * 1e-6 / 2
        return out


def _work(S, N, item, M):
    "what the shape demands of each kernel: (amount, unit)"
    m = 30 + int(math.sqrt(M))
    return {"stats_kernel": (2 * S * N * item * 1e-9, "GB"),
            "select_kernel": (2.0 * S * S * N * 1e-9, "G compares"),
            "fit_kernel": ((m + 2) * M * N * 1e-9, "G log1p"),
            "finish_kernel": (4 * S * N * (item + 2) * 1e-9, "GB"),
            "totals_kernel": (9 * N * 8 * 1e-9, "GB")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_rate.txt"))
    ap.add_argument("--child", nargs=3, metavar=("S", "N", "DTYPE"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "loo_rate.py measures on the GPU"
    if a.child:
        return _child(int(a.child[0]), int(a.child[1]), a.child[2])
    from psis_reference import psis_reference, tail_length
    # the traced runs first, each in a process of its own: this process has not opened the GPU yet
    traces = {name: _kernel_ms(S, N, dtype) for name, S, N, dtype in SHAPES}
    dev = "cuda:0"
    lines = [f"PSIS-LOO + WAIC, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (sources "
             f"{_hip.source_sha()}), {a.reps} calls per figure, workspace 256 MiB",
             f"{'shape':24s} {'chunks':>6s} {'ms/call':>10s} {'host numpy s (scaled)':>22s} {'khat > 0.7':>10s}"]
    detail = []
    for name, S, N, dtype in SHAPES:
        x = _table(S, N, dtype, dev)
        per = mc.bytes_per_observation(S, False)
        chunks = 1 if per * N <= 256 << 20 else -(-N // ((256 << 20) // per // 64 * 64))
        ms = _event_ms(lambda: mc.loo_waic(x), a.reps)
        res = mc.loo(x)
        host = x[:, :HOST_SLICE].double().cpu().numpy()
        t0 = time.perf_counter()
        psis_reference(host)
        host_s = (time.perf_counter() - t0) * N / HOST_SLICE
        lines.append(f"{name:24s} {chunks:6d} {ms:10.2f} {host_s:22.1f} {res.n_bad:10d}")
        print(lines[-1], flush=True)
        work = _work(S, N, x.element_size(), tail_length(S))
        tr = traces[name]
        for k in KERNELS:
            amount, unit = work[k]
            if tr is None:
                detail.append(f"{name:24s} {k:14s} {'not measured':>10s} {amount:10.3f} {unit}")
            else:
                rate = amount / (tr[k] * 1e-3) if tr[k] > 0 else float("nan")
                detail.append(f"{name:24s} {k:14s} {tr[k]:10.3f} {amount:10.3f} {unit:11s} {rate:10.1f} {unit}/s")
        del x
    lines.append("")
    lines.append("per kernel, from a separate run under rocprofv3 --kernel-trace --stats (ms per call, all chunks):")
    lines.append(f"{'shape':24s} {'kernel':14s} {'ms/call':>10s} {'work':>10s}")
    lines += detail
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
