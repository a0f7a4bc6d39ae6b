"""Time of the Rao-Blackwellised model's marginal likelihood (``raob.marginal_log_likelihood``: csrc/raob_hip.inc), forward
and backward, at the sizes a leapfrog step meets: (N, F) = (1,000, 50), (10,000, 50), (45,000, 50), fp32 and fp64 features,
against the same quantity written with torch operators -- the reference's ``log_likelihood`` (models/base.py:229-277)
with ``torch.linalg.cholesky_ex`` / ``solve_triangular`` in place of the removed ``torch.cholesky`` (fp32 Gram matrix, fp64
factorisation, as there), differentiated by autograd.  ``cholesky_ex`` returns its error flag on the device, so neither
route synchronises with the host.

What is timed is one ``value = f(...); value.backward()`` with f a leaf that requires a gradient and the noise variance
a float.  Device events; one warm-up call, then the median (least .. largest) of ``--windows`` windows of ``--reps``
repetitions.  The Gram pass, the factor pass and the gradient pass are also timed each by itself.

    python tools/raob_rate.py [--reps 20] [--windows 7] [--out profiles/raob_rate.txt]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip, raob  # noqa: E402
from bnn_priors_amd.calibration import _stream  # noqa: E402

SIZES = ((1_000, 50), (10_000, 50), (45_000, 50))
NOISE_VAR = 0.64


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


def composition(f, y, sig, last_layer_var):
    "reference models/base.py:229-277 on current torch operators"
    N, F = f.shape
    const = N * math.log(2 * math.pi) + (N - F) * math.log(sig) + (y.view(-1) @ y.view(-1)) / sig
    FF = (f.t() @ f) * last_layer_var
    A = FF.to(torch.float64) + sig * torch.eye(F, dtype=torch.float64, device=f.device)
    L = torch.linalg.cholesky_ex(A).L
    logdet = 2 * L.diag().log().sum()
    Lfy = torch.linalg.solve_triangular(L, (f.t() @ y).to(torch.float64), upper=False).view(-1)
    return (-0.5 * (const + logdet - (Lfy @ Lfy) * (last_layer_var / sig))).to(f.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raob_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "raob_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    lib = _hip.lib()
    lines = [f"RaoB marginal likelihood, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (source_sha "
             f"{_hip.source_sha()}), noise_var {NOISE_VAR}, last_layer_var 2 / F, device events, one warm-up call, "
             f"{a.windows} windows of {a.reps}: median (least .. largest) in ms"]

    def row(what, ms, extra=""):
        lines.append(f"{what:66s} {ms[0]:9.4f} ({ms[1]:.4f} .. {ms[2]:.4f}){extra}")
        print(lines[-1], flush=True)

    for dtype in (torch.float32, torch.float64):
        for N, F in SIZES:
            g = torch.Generator(device=dev).manual_seed(N)
            f = torch.randn(N, F, generator=g, device=dev, dtype=dtype).relu_().requires_grad_()
            y = 2 * torch.randn(N, 1, generator=g, device=dev, dtype=dtype)
            s2 = 2.0 / F
            tag = f"N = {N:6d}, F = {F}, {str(dtype).split('.')[1]}:"

            def kernels():
                f.grad = None
                raob.marginal_log_likelihood(f, y, NOISE_VAR, s2).backward()

            def torch_ops():
                f.grad = None
                composition(f, y, NOISE_VAR, s2).backward()

            ours, theirs = _event_ms(kernels, a.reps, a.windows), _event_ms(torch_ops, a.reps, a.windows)
            value, grad = raob.marginal_log_likelihood(f, y, NOISE_VAR, s2).detach(), f.grad.clone()
            kernels()
            agree = (float((value - composition(f, y, NOISE_VAR, s2).detach()).abs() / value.abs()),
                     float((f.grad - grad).abs().max() / grad.abs().max()))
            row(f"{tag} HIP kernels, forward + backward", ours)
            row(f"{tag} torch operators + autograd, forward + backward", theirs,
                f"  {theirs[0] / ours[0]:.2f} x the kernels; relative difference of the value {agree[0]:.1e}, "
                f"of the gradient {agree[1]:.1e}")
            fd = f.detach()
            work = torch.empty(lib.sgmcmc_raob_workspace_doubles(N, F), dtype=torch.float64, device=dev)
            state = torch.empty(_hip.raob_state_doubles(F), dtype=torch.float64, device=dev)
            out = torch.empty_like(fd)
            is64 = _hip.F64 if dtype == torch.float64 else _hip.F32
            row(f"{tag}   Gram pass alone", _event_ms(lambda: _hip.check(lib.sgmcmc_raob_gram(
                fd.data_ptr(), y.data_ptr(), is64, N, F, work.data_ptr(), _stream()), "gram"), a.reps, a.windows))
            row(f"{tag}   factor pass alone", _event_ms(lambda: _hip.check(lib.sgmcmc_raob_factor(
                work.data_ptr(), N, F, s2, NOISE_VAR, 0, state.data_ptr(), _stream()), "factor"), a.reps, a.windows))
            row(f"{tag}   gradient pass alone", _event_ms(lambda: _hip.check(lib.sgmcmc_raob_grad(
                fd.data_ptr(), y.data_ptr(), is64, N, F, state.data_ptr(), 0, out.data_ptr(), 0, _stream()), "grad"),
                a.reps, a.windows))
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
