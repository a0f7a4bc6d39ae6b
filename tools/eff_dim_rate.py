"""Time of the effective-dimensionality kernels (``eff_dim``: csrc/lanczos_hip.inc) at the sizes they were written for:

  1. one Lanczos step -- all eight launches, without the Hessian-vector product and without the host's read of the state --
     at D = 89,610 (the dense classifier 784-100-100-10) and D = 272,474 (googleresnet), against j + 1 = 21, 101 and 501 rows;
  2. the tridiagonal eigensolver at m = 40, 128, 512, one matrix and a batch of 100;
  3. the Ritz GEMM U = V^T Y[:, top 20] at both D with m = 40 rows;

each beside its torch-fp64 equivalent in the same process (``V @ w`` and ``w - c @ V`` twice with two norms;
``torch.linalg.eigh`` of the dense T; ``V.T @ Y``), and one Hessian-vector product of the dense classifier on 1,024 rows for
context.  No rate is promised; the numbers are recorded as they come out.

    python tools/eff_dim_rate.py [--reps 10] [--windows 5] [--out profiles/eff_dim_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip  # noqa: E402
from bnn_priors_amd import eff_dim  # noqa: E402

SIZES = (("dense classifier 784-100-100-10", 89610), ("googleresnet", 272474))
ROWS = (21, 101, 501)


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


def _torch_step(V, w):
    "two passes of classical Gram-Schmidt, the norm and the next row by fp64 library calls"
    for _ in range(2):
        c = V @ w
        w = w - c @ V
    return w / torch.linalg.vector_norm(w)


def _dense_T(a, b):
    return torch.diag_embed(a) + torch.diag_embed(b[..., :-1], 1) + torch.diag_embed(b[..., :-1], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eff_dim_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eff_dim_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"effective dimensionality, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (sources "
             f"{_hip.source_sha()}), fp64, device events, {a.windows} windows of {a.reps}: median (least .. largest)",
             f"{'what':66s} {'ms':>28s} {'GB/s':>8s}"]

    def row(what, ms, nbytes=None):
        med, lo, hi = ms
        lines.append(f"{what:66s} {f'{med:.4f} ({lo:.4f} .. {hi:.4f})':>28s} "
                     + (f"{nbytes / (med * 1e-3) / 1e9:8.0f}" if nbytes else ""))
        print(lines[-1], flush=True)

    for name, D in SIZES:
        lines.append(f"{name}: D = {D}, {eff_dim.splits(D)} splits of {-(-D // eff_dim.CHUNK)} chunks")
        for rows in ROWS:
            V = torch.linalg.qr(torch.randn((D, rows), generator=gen, device=dev, dtype=torch.float64))[0].T.contiguous()
            buf = torch.zeros((rows + 1, D), dtype=torch.float64, device=dev)
            buf[:rows] = V
            w = torch.randn(D, generator=gen, device=dev, dtype=torch.float64)
            step = eff_dim._Step(buf)
            work = w.clone()
            traffic = 4.0 * 8 * rows * D                 # V is read four times: two dots and two updates

            def ours(n):
                for _ in range(n):
                    work.copy_(w)
                    step.run(rows - 1, work)

            row(f"  one step against {rows} rows (8 launches + the copy of w)", _event_ms(ours, a.reps, a.windows), traffic)
            row(f"  torch: V @ w, w - c @ V twice, norm, scale ({rows} rows)",
                _event_ms(lambda n: [_torch_step(V, w) for _ in range(n)], a.reps, a.windows), traffic)
            lines.append(f"    largest |next row - torch's| : {float((buf[rows] - _torch_step(V, w)).abs().max()):.2e}")
        m, k = 40, 20
        V = torch.linalg.qr(torch.randn((D, m), generator=gen, device=dev, dtype=torch.float64))[0].T.contiguous()
        theta, Y = torch.linalg.eigh(_dense_T(torch.randn(m, generator=gen, device=dev, dtype=torch.float64),
                                              torch.randn(m, generator=gen, device=dev, dtype=torch.float64)))
        Y = Y.contiguous()
        row(f"  Ritz GEMM U = V^T Y[:, top {k}], m = {m} (MFMA f64 16x16x4)",
            _event_ms(lambda n: [eff_dim._ritz(V, theta, Y, k, False) for _ in range(n)], a.reps, a.windows), 8.0 * (m + k) * D)
        row(f"  torch: V.T @ Y[:, -{k}:]", _event_ms(lambda n: [V.T @ Y[:, -k:] for _ in range(n)], a.reps, a.windows),
            8.0 * (m + k) * D)
    lines.append("tridiagonal eigensolver (implicit QL, one workgroup per matrix) against torch.linalg.eigh of the dense T")
    for m in (40, 128, 512):
        for batch in (1, 100):
            al = torch.randn((batch, m), generator=gen, device=dev, dtype=torch.float64)
            be = torch.randn((batch, m), generator=gen, device=dev, dtype=torch.float64)
            T = _dense_T(al, be)
            reps, windows = (1, min(a.windows, 3)) if m == 512 else (a.reps, a.windows)
            sweeps = eff_dim.tridiag_eig(al, be)[2]
            row(f"  m = {m}, batch {batch} ({float(sweeps.float().mean()):.0f} sweeps)",
                _event_ms(lambda n: [eff_dim.tridiag_eig(al, be) for _ in range(n)], reps, windows))
            row(f"  torch.linalg.eigh, m = {m}, batch {batch}",
                _event_ms(lambda n: [torch.linalg.eigh(T) for _ in range(n)], reps, windows))
            lines.append(f"    largest |theta - eigh's| / max |theta|: "
                         f"{float((eff_dim.tridiag_eig(al, be)[0] - torch.linalg.eigh(T)[0]).abs().max() / T.abs().max()):.2e}")
    from bnn_priors_amd import models
    torch.manual_seed(0)
    model = models.ClassificationDenseNet(784, 10, 100, 3).to(dev)
    x, y = torch.randn(1024, 784, device=dev), torch.randint(0, 10, (1024,), device=dev)
    hvp = eff_dim.model_hvp(model, x, y)
    D = sum(p.numel() for p in model.parameters())
    v = torch.randn(D, generator=gen, device=dev, dtype=torch.float64)
    lines.append(f"for context: one Hessian-vector product (autograd, fp32) of the dense classifier, D = {D}, 1,024 rows")
    row("  model_hvp(v)", _event_ms(lambda n: [hvp(v) for _ in range(n)], a.reps, a.windows))
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
