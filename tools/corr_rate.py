"""Time of the weight-correlation analysis (``weight_correlation``: csrc/corr_hip.inc) at the sizes it was written for:

  1. S = 100 samples of a 100 x 784 dense weight in fp32 (31.4 MB), on both axes: V = 100 rows with n = 78,400
     observations, and V = 784 columns with n = 10,000;
  2. S = 100 samples of a googleresnet 64 x 64 x 3 x 3 convolution weight in fp32 (14.7 MB), output channels: V = 64,
     n = 57,600 -- one covariance, and one launch chunk of permuted replicates (gather + Gram + finish + statistics, the
     tables drawn beforehand).

Per case: the mean pass, the Gram pass (its fp64 multiply-add rate, 2 V^2 n flop -- the kernel forms the upper block
triangle, so the rate is that of the useful product), ``covariance`` as a whole, and the same quantity through
``torch.cov`` in fp64 (on a contiguous [V, n] copy made beforehand) on the same GPU; for the replicates ``torch.gather``
plus a batched fp64 matmul of the centred copies.  No speed bar is set; the numbers are recorded.

    python tools/corr_rate.py [--reps 20] [--windows 5] [--out profiles/corr_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip  # noqa: E402
from bnn_priors_amd import weight_correlation as wc  # noqa: E402

CASES = (("dense 100 x 784, rows", (100, 784), 0), ("dense 100 x 784, columns", (100, 784), 1),
         ("conv 64 x 64 x 3 x 3, output channels", (64, 64, 3, 3), 0))
S = 100


def _event_ms(fn, reps, windows):
    "ms per repetition: the median, the least and the largest of ``windows`` windows; fn(reps) enqueues reps of them"
    fn(1)
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(reps)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "corr_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"weight correlation, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (sources "
             f"{_hip.source_sha()}), fp32 stacks of S = {S}, device events, {a.windows} windows of {a.reps}: median "
             f"(least .. largest)",
             f"{'what':62s} {'ms':>28s} {'fp64 Tflop/s':>13s}"]

    def row(what, ms, flop=None):
        med, lo, hi = ms
        lines.append(f"{what:62s} {f'{med:.4f} ({lo:.4f} .. {hi:.4f})':>28s} "
                     + (f"{flop / (med * 1e-3) / 1e12:13.2f}" if flop else ""))
        print(lines[-1], flush=True)

    for name, shape, var_dim in CASES:
        w = 0.05 * torch.randn((S,) + shape, generator=gen, device=dev)
        g = wc._geometry(w, var_dim)
        V, n = g.V, g.n
        sp = wc.splits(V, n)
        flop = 2.0 * V * V * n
        lines.append(f"{name}: V = {V}, n = {n}, {sp} splits x {-(-V // wc.TILE) * (-(-V // wc.TILE) + 1) // 2} block "
                     f"pairs, {'variable' if g.v_major else 'observation'}-major loads")
        mean, bad = wc._mean(w, g)
        row("  mean pass", _event_ms(lambda k: [wc._mean(w, g) for _ in range(k)], a.reps, a.windows))
        row("  Gram pass + finish (MFMA f64 16x16x4)",
            _event_ms(lambda k: [wc._gram(w, g, 1, 0, mean, bad, sp, 1, True) for _ in range(k)], a.reps, a.windows), flop)
        row("  covariance (mean, Gram, finish)",
            _event_ms(lambda k: [wc.covariance(w, var_dim) for _ in range(k)], a.reps, a.windows), flop)
        row("  covariance + offdiag_stats",
            _event_ms(lambda k: [wc.offdiag_stats(wc.covariance(w, var_dim).corr) for _ in range(k)], a.reps, a.windows))
        x = w.movedim(1 + var_dim, 0).reshape(V, n).contiguous()
        row("  torch.cov + torch.corrcoef in fp64 of the contiguous [V, n]",
            _event_ms(lambda k: [(torch.cov(x.double()), torch.corrcoef(x.double())) for _ in range(k)],
                      max(1, a.reps // 4), a.windows), 2 * flop)
        row("  torch.cov in fp64 alone", _event_ms(lambda k: [torch.cov(x.double()) for _ in range(k)],
                                                   max(1, a.reps // 4), a.windows), flop)
        if var_dim == 0 and len(shape) == 4:
            R = wc._batch_replicates(V, n, sp, x.element_size(), 199, wc.WORKSPACE_BYTES)
            tables = torch.argsort(torch.rand((R, V, n), generator=gen, device=dev), dim=-1, stable=True)
            gc = wc._contiguous_geometry(V, n)

            def ours(k):
                for _ in range(k):
                    xp = torch.gather(x.unsqueeze(0).expand(R, V, n), 2, tables)
                    wc.offdiag_stats(wc._gram(xp, gc, R, V * n, mean, bad, sp, 1, False)[1])

            def plain(k):
                for _ in range(k):
                    d = torch.gather(x.unsqueeze(0).expand(R, V, n), 2, tables).double() - mean[None, :, None]
                    G = d @ d.transpose(1, 2)
                    s = torch.diagonal(G, dim1=1, dim2=2).sqrt()
                    r = G / (s[:, :, None] * s[:, None, :])
                    i, j = torch.triu_indices(V, V, 1, device=dev)
                    (r[:, i, j] ** 2).mean(1).sqrt(), r[:, i, j].abs().amax(1)

            lines.append(f"  one chunk of R = {R} permuted replicates (of 199; the workspace of {wc.WORKSPACE_BYTES >> 20} "
                         f"MiB sizes R)")
            row("    gather + Gram + finish + offdiag_stats, HIP", _event_ms(ours, max(1, a.reps // 4), a.windows), R * flop)
            row("    gather + centred bmm + statistics, torch ops (fp64)", _event_ms(plain, max(1, a.reps // 4), a.windows),
                R * flop)
            row("    drawing the R tables (torch.rand + stable argsort)",
                _event_ms(lambda k: [torch.argsort(torch.rand((R, V, n), generator=gen, device=dev), dim=-1, stable=True)
                                     for _ in range(k)], 2, a.windows))
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
