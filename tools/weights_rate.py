"""Time of the model-averaging path (``model_comparison.stacking_weights`` / ``bb_pseudo_bma_weights`` /
``pseudo_bma_weights``; csrc/weights_hip.inc) at the shapes of a prior comparison: K in {4, 8, 31} models' pointwise elpd
rows over N = 60,000 training observations, fp64.

The rows are -2 log1p(t^2 / 3) of student-t(3) draws generated on the device from a seed, half of each row shared by all
models (so the models are correlated) plus an offset per model.  Per shape:

* the device-event time per stacking iteration (one launch pair; ``--iters`` pairs between two events at tol = 0) with q
  recomputed per iteration and with q formed once into the workspace: five windows of each, taken in alternation, the
  median with the smallest and the largest window beside it;
* the iterations to tol = 1e-8 and the wall time of the whole ``stacking_weights`` call (its host reads included);
* the wall time of B = 1,000 bootstrap replicates and of pseudo-BMA;
* on the host, on the same input: the numpy restatement (tests/weights_reference.py, numpy's sums) -- stacking timed over
  ``HOST_ITERS`` iterations and scaled to the device's iteration count, the bootstrap over ``HOST_B`` replicates and scaled
  to 1,000 -- and ``scipy.optimize`` SLSQP run to its own convergence, with its objective's distance to the device's;
* each stacking kernel's own time per iteration from a run of its own under ``rocprofv3 --kernel-trace --stats`` (a fresh
  child process): which of the pair bounds an iteration.

    python tools/weights_rate.py [--iters 512] [--out profiles/weights_rate.txt]
"""
import argparse
import csv
import glob
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

N = 60000
MODELS = (4, 8, 31)
B = 1000
HOST_ITERS, HOST_B = 20, 10
TRACE_ITERS = 256
REPEATS = 5
KERNELS = ("slice_kernel", "stack_finish_kernel")


def _table(K, dev):
    g = torch.Generator(device=dev).manual_seed(K)

    def student(*shape):
        t = torch.randn(shape, generator=g, dtype=torch.float64, device=dev)
        chi = sum(torch.randn(shape, generator=g, dtype=torch.float64, device=dev) ** 2 for _ in range(3))
        return -2.0 * torch.log1p((t / (chi / 3.0).sqrt()) ** 2 / 3.0)

    return 0.5 * student(N) + 0.5 * student(K, N) + 0.01 * torch.randn((K, 1), generator=g, dtype=torch.float64, device=dev)


def _iterate_ms(P, iters, cache_q):
    "device-event time of one launch pair: ``iters`` pairs at tol = 0 after a warm-up batch"
    K = P.shape[0]
    work = torch.empty(mc.weights_workspace_bytes(K, N, 0, cache_q) // 8, dtype=torch.float64, device=P.device)
    state = torch.empty(mc.STATE, dtype=torch.float64, device=P.device)
    L, stream = _hip.lib(), torch.cuda.current_stream().cuda_stream
    args = (work.data_ptr(), work.numel() * 8, state.data_ptr(), stream)
    _hip.check(L.sgmcmc_stacking_init(P.data_ptr(), P.stride(0), K, N, 0.0, 1 << 40, int(cache_q), *args), "init")
    _hip.check(L.sgmcmc_stacking_iterate(P.data_ptr(), P.stride(0), K, N, int(cache_q), 16, *args), "iterate")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _hip.check(L.sgmcmc_stacking_iterate(P.data_ptr(), P.stride(0), K, N, int(cache_q), iters, *args), "iterate")
    e1.record()
    torch.cuda.synchronize()
    assert state[mc.S_FROZEN].item() == 0.0
    return e0.elapsed_time(e1) / iters


def _wall(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _child(K):
    "TRACE_ITERS launch pairs, for the kernel trace of the parent's profiler run"
    _iterate_ms(_table(K, "cuda:0"), TRACE_ITERS, False)


def _kernel_us(K):
    "{kernel: us per launch} from a traced child process, or None where the profiler is missing or its run fails"
    if shutil.which("rocprofv3") is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "weights", "--",
               sys.executable, os.path.abspath(__file__), "--child", str(K)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            print("kernel trace failed:", r.returncode, r.stderr[-2000:], flush=True)
            return None
        out = dict.fromkeys(KERNELS, 0.0)
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if "weights::" + k in row["Name"]:
                        out[k] += float(row["TotalDurationNs"]) * 1e-3 / float(row["Calls"])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weights_rate.txt"))
    ap.add_argument("--child", type=int, metavar="K")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "weights_rate.py measures on the GPU"
    if a.child:
        return _child(a.child)
    import weights_reference as ref
    # the traced runs first, each in a process of its own: this process has not opened the GPU yet
    traces = {K: _kernel_us(K) for K in MODELS}
    dev = "cuda:0"
    lines = [f"stacking / pseudo-BMA+ weights, N = {N}, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} "
             f"(sources {_hip.source_sha()}); tol = 1e-8, check_every = 64, B = {B}; stacking_weights forms q "
             f"{'once' if mc.CACHE_Q else 'per iteration'}",
             f"{'K':>3s} {'us/iter (range)':>25s} {'us/iter q once (range)':>25s} {'iterations':>10s} {'stacking s':>11s} "
             f"{'bootstrap ms':>13s} {'pseudo-BMA ms':>14s} | host: {'numpy EM s (scaled)':>20s} "
             f"{'numpy bootstrap s (scaled)':>27s} {'SLSQP s':>8s} {'f_dev - f_slsqp':>16s}"]
    for K in MODELS:
        P = _table(K, dev)
        # the two variants in alternation, REPEATS windows each: the median, with the windows' range beside it
        windows = {False: [], True: []}
        for _ in range(REPEATS):
            for cache_q in (False, True):
                windows[cache_q].append(_iterate_ms(P, a.iters, cache_q) * 1e3)
        us, us_once = (f"{sorted(v)[REPEATS // 2]:.2f} ({min(v):.2f}-{max(v):.2f})" for v in (windows[False], windows[True]))
        res, stack_s = _wall(lambda: mc.stacking_weights(P))
        _, boot_s = _wall(lambda: mc.bb_pseudo_bma_weights(P, B))
        _, bma_s = _wall(lambda: mc.pseudo_bma_weights(P))
        host = P.cpu().numpy()
        t0 = time.perf_counter()
        ref.stacking(host, tol=0.0, max_iter=HOST_ITERS, sums=ref.NUMPY)
        em_s = (time.perf_counter() - t0) / (HOST_ITERS + 1) * (res.iterations + 1)
        t0 = time.perf_counter()
        ref.bb_pseudo_bma(host, HOST_B, sums=ref.NUMPY)
        bb_s = (time.perf_counter() - t0) / HOST_B * B
        t0 = time.perf_counter()
        _, f_opt = ref.slsqp(host)
        slsqp_s = time.perf_counter() - t0
        lines.append(f"{K:3d} {us:>25s} {us_once:>25s} {res.iterations:10d} {stack_s:11.3f} {boot_s * 1e3:13.2f} "
                     f"{bma_s * 1e3:14.3f} | {'':6s}{em_s:20.1f} {bb_s:27.1f} {slsqp_s:8.2f} {res.lpd / N - f_opt:16.2e}"
                     f"   (converged {res.converged}, gap {res.gap:.2e})")
        print(lines[-1], flush=True)
        del P
    lines.append("")
    lines.append(f"per kernel of the stacking pair, from a separate run under rocprofv3 --kernel-trace --stats "
                 f"({TRACE_ITERS + 16} pairs, q recomputed; us per launch):")
    lines.append(f"{'K':>3s} {'slice_kernel':>13s} {'stack_finish_kernel':>20s}")
    for K in MODELS:
        tr = traces[K]
        lines.append(f"{K:3d} {'not measured':>13s}" if tr is None else
                     f"{K:3d} {tr['slice_kernel']:13.2f} {tr['stack_finish_kernel']:20.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
