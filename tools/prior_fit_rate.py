"""Time of fitting a multivariate t to a stack of weight samples (``prior_fit.fit_mvt``: csrc/fit_hip.inc) at the size the
data-driven priors are fitted at: S = 100 samples of a googleresnet 64 x 64 x 3 x 3 convolution weight in fp32, 409,600
filters of 9 numbers (14.7 MB), in the two geometries of the prior hook: one filter per event (F = 1), and one event per
input channel (``permute = (1, 0, 2, 3)``, ``event_dim = 3``: F = 64).

Per geometry: ``moments``; one EM iteration (the pass over the stack, kernel A, and the single-workgroup update, kernel B:
``--reps`` iterations between two device events on a state that cannot converge, tol = 0); the whole fit with its host
read-backs (host clock around a call that ends synchronised); and the same EM iteration written in plain torch ops in
fp64 on the same GPU -- the only route there was before these kernels.  A pass reads the stack once: bytes / time is set
beside the 6.3 TB/s a streaming read achieves on this device (8 TB/s peak).

    python tools/prior_fit_rate.py [--reps 20] [--windows 5] [--out profiles/prior_fit_rate.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bnn_priors_amd import _hip  # noqa: E402
from bnn_priors_amd import prior_fit as pf  # noqa: E402
from bnn_priors_amd.calibration import _stream  # noqa: E402

S, SHAPE, P, DF = 100, (64, 64, 3, 3), 9, 4.0
GEOMETRIES = (("F = 1 (one filter per event)", None, None), ("F = 64 (one event per input channel)", 3, (1, 0, 2, 3)))
HBM_ACHIEVABLE = 6.3e12                 # a streaming read on this device (8 TB/s peak)


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


def _stack(dev):
    "heavy-tailed correlated filters: Gaussian vectors over sqrt(Gamma), one mixing variable per filter"
    g = torch.Generator(device=dev).manual_seed(0)
    torch.manual_seed(0)                                        # (the Gamma sampler draws from the global generator)
    n = S * SHAPE[0] * SHAPE[1]
    A = torch.eye(P, device=dev) + 0.3 * torch.randn((P, P), generator=g, device=dev)
    z = torch.randn((n, P), generator=g, device=dev) @ A.T
    mix = torch.distributions.Gamma(torch.tensor(DF / 2, device=dev), torch.tensor(DF / 2, device=dev)).sample((n, 1))
    return (0.05 * z / mix.sqrt()).reshape((S,) + SHAPE).contiguous()


def _torch_iteration(w, event_dim, permute, mu, S_, nu):
    "one EM iteration of include/sgmcmc_hip.h, definition 2, in torch ops (fp64)"
    x = w if permute is None else w.permute(0, *(1 + p for p in permute))
    E = x.reshape(-1, 1 if event_dim is None else SHAPE[0], P).to(torch.float64)
    n_ev, F, _ = E.shape
    D = F * P
    L = torch.linalg.cholesky(S_)
    d = E - mu
    z = torch.linalg.solve_triangular(L, d.reshape(-1, P).T, upper=False)
    M = (z * z).sum(0).reshape(n_ev, F).sum(1)
    u = (nu + D) / (nu + M)
    W = F * u.sum()
    A = (u[:, None, None] * d).sum((0, 1))
    B = torch.einsum("e,efa,efb->ab", u, d, d)
    ll = -(nu + D) / 2 * torch.log1p(M / nu).sum()
    c1 = (u.log() - u).sum()
    return mu + A / W, (B - torch.outer(A, A / W)) / W, ll, c1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_fit_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prior_fit_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    lib = _hip.lib()
    w = _stack(dev)
    nbytes = w.numel() * w.element_size()
    lines = [f"prior fit, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (sources {_hip.source_sha()}), "
             f"stack {tuple(w.shape)} {str(w.dtype)[6:]} = {nbytes / 1e6:.1f} MB, device events, {a.windows} windows of "
             f"{a.reps}: median (least .. largest)",
             f"{'what':58s} {'ms':>28s} {'TB/s read':>10s} {'of 6.3':>7s}"]

    def row(what, ms, reads=True):
        med, lo, hi = ms
        rate = nbytes / (med * 1e-3)
        lines.append(f"{what:58s} {f'{med:.4f} ({lo:.4f} .. {hi:.4f})':>28s} "
                     + (f"{rate / 1e12:10.3f} {rate / HBM_ACHIEVABLE:7.1%}" if reads else ""))
        print(lines[-1], flush=True)

    for name, event_dim, permute in GEOMETRIES:
        lines.append(name)
        g, _, _ = pf._geometry(w, P, event_dim, permute)
        work = pf._Workspace(g, dev)
        lines.append(f"  {g.events} events, tile of {pf.tile_events(P, g.F)} events, {work.blocks} workgroups")
        row("  moments", _event_ms(lambda k: [pf.moments(w, P, event_dim, permute) for _ in range(k)], a.reps, a.windows))
        mom, _ = pf._moments_table(w, g, 0, work)
        state = torch.empty(_hip.FIT_STATE, dtype=torch.float64, device=dev)
        trace = torch.zeros(1 << 20, dtype=torch.float64, device=dev)
        _hip.check(lib.sgmcmc_fit_mvt_init(P, mom.data_ptr(), mom[P:].data_ptr(), 5.0, state.data_ptr(), _stream()),
                   "init")

        def iterate(k):
            _hip.check(lib.sgmcmc_fit_mvt_iterate(w.data_ptr(), _hip.F32, g, k, 1 << 20, 0.0, 2.01, 1e4,
                                                  work.part.data_ptr(), work.counts.data_ptr(), state.data_ptr(),
                                                  trace.data_ptr(), _stream()), "iterate")
        kernel = _event_ms(iterate, a.reps, a.windows)
        row("  one EM iteration (pass A + update B), HIP", kernel)
        assert state[0].item() == 0.0                           # still iterating: the launches were not no-ops
        mu0, S0 = mom[:P].clone(), (mom[P:P + P * P] * 0.6).reshape(P, P).clone()
        nu0 = torch.tensor(5.0, dtype=torch.float64, device=dev)
        plain = _event_ms(lambda k: [_torch_iteration(w, event_dim, permute, mu0, S0, nu0) for _ in range(k)],
                          max(1, a.reps // 4), a.windows)
        row("  one EM iteration, torch ops (fp64), without its nu solve", plain)
        lines.append(f"  torch / HIP per iteration: {plain[0] / kernel[0]:.1f} x")
        fits = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = pf.fit_mvt(w, P, event_dim, permute)
            torch.cuda.synchronize()
            fits.append((time.perf_counter() - t0) * 1e3)
        fits.sort()
        lines.append(f"  whole fit (host clock, with read-backs): {fits[1]:.1f} ms ({fits[0]:.1f} .. {fits[2]:.1f}), "
                     f"{f.iterations} iterations, converged {f.converged}, df {f.df:.4f}; "
                     f"{fits[1] / (f.iterations + 1):.4f} ms per iteration")
        print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
