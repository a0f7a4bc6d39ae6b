"""Time of the kernel Stein discrepancy (``stein``: csrc/stein_hip.inc) at the sizes it was written for:

  1. S = 100 samples of the dense classifier (784-100-100-10: D = 89,610 parameters), fp32 samples and scores;
  2. S = 512 samples of googleresnet (ResNet-20: D = 272,474 parameters), fp32 samples and scores.

Per case: the Gram pass of the 2S rows [X - x_0; G] with its reduction (the rate is 6 S^2 D flop -- the three products A, B
and C written out in full, what the torch comparison executes -- over the time; the kernel itself forms the upper block
triangle of the 2S x 2S matrix, 2 S^2 D multiply-adds plus the diagonal blocks' lower halves), ``kernel_matrix`` as a
whole, ``ksd``, ``thin(m = S / 10)``, a wild bootstrap of 199 replicates; and the same quantities through ``torch.matmul`` in fp64 plus element-wise operations in the same process (the thinning as m rounds of
``argmin`` and a row addition).  No rate is promised; the numbers are recorded and the long pole named.

    python tools/stein_rate.py [--reps 10] [--windows 5] [--out profiles/stein_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip  # noqa: E402
from bnn_priors_amd import stein  # noqa: E402

CASES = (("dense classifier 784-100-100-10", 100, 89610), ("googleresnet", 512, 272474))


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


def _torch_kernel_matrix(x, g, c2=1.0, beta=-0.5):
    "the same quantities by fp64 matmuls of the anchored copies and element-wise operations"
    xt = x.double() - x[0].double()
    gd = g.double()
    A, B, C = xt @ xt.T, xt @ gd.T, gd @ gd.T
    a, b = torch.diagonal(A), torch.diagonal(B)
    r2 = (a[:, None] + a[None, :] - 2 * A).clamp_min(0)
    t = b[:, None] - B - B.T + b[None, :]
    u = c2 + r2
    return u ** beta * C - 2 * beta * u ** (beta - 1) * (t + x.shape[1]) - 4 * beta * (beta - 1) * u ** (beta - 2) * r2


def _torch_thin(K, m):
    half, run = torch.diagonal(K) / 2, torch.zeros(K.shape[0], dtype=K.dtype, device=K.device)
    picks = []
    for _ in range(m):
        p = torch.argmin(half + run)
        picks.append(p)
        run = run + K[p]
    return torch.stack(picks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stein_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stein_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"kernel Stein discrepancy, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (sources "
             f"{_hip.source_sha()}), fp32 samples and scores, device events, {a.windows} windows of {a.reps}: median "
             f"(least .. largest)",
             f"{'what':62s} {'ms':>28s} {'fp64 Tflop/s':>13s}"]

    def row(what, ms, flop=None):
        med, lo, hi = ms
        lines.append(f"{what:62s} {f'{med:.4f} ({lo:.4f} .. {hi:.4f})':>28s} "
                     + (f"{flop / (med * 1e-3) / 1e12:13.2f}" if flop else ""))
        print(lines[-1], flush=True)

    for name, S, D in CASES:
        x = 0.05 * torch.randn((S, D), generator=gen, device=dev)
        g = -x / 0.05 ** 2 + torch.randn((S, D), generator=gen, device=dev)
        sp, nb, m = stein.splits(S, D), -(-2 * S // stein.TILE), S // 10
        flop = 6.0 * S * S * D
        lines.append(f"{name}: S = {S}, D = {D}, {sp} splits x {nb * (nb + 1) // 2} block pairs, "
                     f"{2 * 4 * S * D / 1e6:.1f} MB of input")
        gram, bad = stein._gram(x, g)
        k = stein.kernel_matrix(x, g)
        signs = torch.where(torch.rand((199, S), generator=gen, device=dev) < 0.5, -1.0, 1.0).double()
        row("  Gram pass + reduce (MFMA f64 16x16x4)",
            _event_ms(lambda n: [stein._gram(x, g) for _ in range(n)], a.reps, a.windows), flop)
        row("  finish (K and r2 from the Gram matrix)",
            _event_ms(lambda n: [stein._finish(gram, bad, D, 1.0, -0.5) for _ in range(n)], a.reps, a.windows))
        row("  kernel_matrix", _event_ms(lambda n: [stein.kernel_matrix(x, g) for _ in range(n)], a.reps, a.windows), flop)
        row("  kernel_matrix, c = 'median'",
            _event_ms(lambda n: [stein.kernel_matrix(x, g, c="median") for _ in range(n)], a.reps, a.windows), flop)
        row("  ksd", _event_ms(lambda n: [stein.ksd(k) for _ in range(n)], a.reps, a.windows))
        row(f"  thin(m = {m})", _event_ms(lambda n: [stein.thin(k, m) for _ in range(n)], a.reps, a.windows))
        row("  wild_bootstrap_test, 199 given sign vectors",
            _event_ms(lambda n: [stein.wild_bootstrap_test(k, signs=signs) for _ in range(n)], a.reps, a.windows))
        K = _torch_kernel_matrix(x, g)
        row("  torch: fp64 copies, three matmuls, element-wise K",
            _event_ms(lambda n: [_torch_kernel_matrix(x, g) for _ in range(n)], max(1, a.reps // 5), a.windows), flop)
        row("  torch: v_stat, u_stat, row means",
            _event_ms(lambda n: [(K.sum() / S ** 2, (K.sum() - torch.diagonal(K).sum()) / (S * (S - 1)), K.sum(1) / S)
                                 for _ in range(n)], a.reps, a.windows))
        row(f"  torch: thinning, m = {m} rounds of argmin",
            _event_ms(lambda n: [_torch_thin(K, m) for _ in range(n)], max(1, a.reps // 5), a.windows))
        row("  torch: 199 quadratic forms (two matmuls)",
            _event_ms(lambda n: [((signs @ K) * signs).sum(1) / S ** 2 for _ in range(n)], a.reps, a.windows))
        lines.append(f"  largest |K - torch's K| / sqrt(K_ii K_jj): "
                     f"{float(((k.K - K).abs() / torch.sqrt(torch.outer(torch.diagonal(K), torch.diagonal(K)))).max()):.2e}")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
