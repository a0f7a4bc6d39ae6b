"""Time of the two kernels of csrc/powerscale_hip.inc at the shape of a stored run -- 4 chains x 300 draws (N = 1200) x
272,474 fp32 quantities (googleresnet's weight count), iid normal draws, A = 4 weight vectors near uniform (the powers
0.98, 0.99, 1.01, 1.02 of a component that depends on the first quantity), one chunk (a 3.3 GB workspace):

* ``sgmcmc_powerscale_sort``: device-event time of one launch, per tile of TQ columns (the grid is Q / TQ workgroups,
  so this is the launch's time over the tile count, the tiles of all CUs running side by side);
* ``sgmcmc_powerscale_distance``: device-event time of one launch, the bytes it has to read -- A N Q (8 + 2) -- and
  write over that time, and that rate over the HBM peak (8.0 TB/s) and over the measured copy rate (6.29 TB/s).  The
  sorted table is re-read per weight vector, the cache's help included: this is the algorithm's traffic over time, not a
  counter.

Warm-up, then ``--windows`` windows of ``--reps`` launches each between two events; the median window.

    python tools/powerscale_rate.py [--reps 5] [--windows 5] [--out profiles/powerscale_rate.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip, prior_sensitivity  # noqa: E402

M, S, Q, A = 4, 300, 272474, 4
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def _window_ms(fn, reps, windows):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "powerscale_rate.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    N = M * S
    x = torch.randn((M, S, Q), generator=g, dtype=torch.float32, device=dev)
    lc = -0.5 * x[:, :, 0].double().square()
    lw = prior_sensitivity.power_scale_weights(lc, (0.98, 0.99, 1.01, 1.02)).log_weights
    w = torch.exp(lw).contiguous()
    values = torch.empty((N, Q), dtype=torch.float64, device=dev)
    order = torch.empty((N, Q), dtype=torch.int16, device=dev)
    out = torch.empty((3, A, Q), dtype=torch.float64, device=dev)
    L = _hip.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def sort():
        _hip.check(L.sgmcmc_powerscale_sort(x.data_ptr(), 0, x.stride(0), x.stride(1), M, S, Q, values.data_ptr(),
                                            order.data_ptr(), stream), "sgmcmc_powerscale_sort")

    def distance():
        _hip.check(L.sgmcmc_powerscale_distance(values.data_ptr(), order.data_ptr(), N, Q, w.data_ptr(), A, Q,
                                                out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream),
                   "sgmcmc_powerscale_distance")

    tq = prior_sensitivity.sort_tile(N)
    tiles = (Q + tq - 1) // tq
    lines = [f"library source hash {_hip.library_sha()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"N = {N} draws ({M} x {S}), Q = {Q} fp32 quantities, A = {A} weight vectors; median (min, max) of "
             f"{args.windows} windows of {args.reps} launches, device events"]
    ms, lo, hi = _window_ms(sort, args.reps, args.windows)
    lines.append(f"  sgmcmc_powerscale_sort      {ms:9.3f} ms ({lo:.3f}, {hi:.3f}); TQ = {tq}, {tiles} tiles: "
                 f"{ms * 1e3 / tiles:.4f} us per tile")
    ms, lo, hi = _window_ms(distance, args.reps, args.windows)
    nbytes = A * N * Q * 10 + N * A * 8 + 3 * A * Q * 8
    rate = nbytes / (ms * 1e-3)
    lines.append(f"  sgmcmc_powerscale_distance  {ms:9.3f} ms ({lo:.3f}, {hi:.3f}); {nbytes / 1e9:.2f} GB: {rate / 1e12:.3f} "
                 f"TB/s = {100 * rate / HBM_PEAK:.1f} % of the 8.0 TB/s peak, {100 * rate / HBM_COPY:.1f} % of the measured "
                 f"copy rate")
    whole = _window_ms(lambda: prior_sensitivity.weighted_distance(x, lw, workspace_bytes=4 << 30), 1, args.windows)[0]
    lines.append(f"  weighted_distance, the whole call (exp, workspace, both kernels)  {whole:9.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
