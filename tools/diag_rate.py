"""Time of the two chain-diagnostic entries (``sgmcmc_chain_rhat``, ``sgmcmc_chain_ess``; bnn_priors_amd/diagnostics.py)
and of the rank-normalised path built on them (``diagnostics.rank_rhat_ess``: ``sgmcmc_chain_rank_scores`` twice,
``sgmcmc_chain_quantiles``, ``sgmcmc_chain_tail_indicators``, the R-hat entry once and the ESS entry three times per
chunk of quantities) at the shapes of a stored run:

* weights    -- 8 chains x 300 draws x 272,474 fp32 quantities (googleresnet's weights), iid normal draws;
* table      -- 4 chains x 100 draws x 100,000 fp64 quantities (a CIFAR-10 test table of probabilities), iid normal;
* table ar1  -- the table's shape with AR(1) draws (phi = 0.9): K lies beyond the first lag block, so the ESS entry
                goes over the sequences more than once.

Per entry: device-event time per call (warm-up, then ``--reps`` calls between two events), and the bytes of ONE pass
over the data divided by that time (the R-hat entry reads the data twice and the ESS entry once per lag block, so this
is a rate of diagnosed data, not a memory bandwidth).  For scale: the same definition in numpy on the host
(tests/chain_diag_reference.py; tests/rank_diag_reference.py for the ``rank`` rows) on a 4,096-quantity slice, scaled
to the full width.  The ``rank`` rows (the two iid shapes) are bound by the N^2 comparisons per quantity of the ranking,
not by memory, and take ``--rank-reps`` calls per figure.

    python tools/diag_rate.py [--reps 10] [--rank-reps 2] [--out profiles/diag_rate.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from bnn_priors_amd import _hip, diagnostics  # noqa: E402
from chain_diag_reference import chain_diag_reference  # noqa: E402
from rank_diag_reference import rank_diag_reference  # noqa: E402

HOST_SLICE = 4096


def _draws(M, S, Q, dtype, phi, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((M, S, Q), generator=g, dtype=dtype, device=dev)
    if phi:
        x[:, 0] /= (1 - phi * phi) ** 0.5
        for s in range(1, S):
            x[:, s] += phi * x[:, s - 1]
    return x


def _event_ms(fn, reps, warmup=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rank-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "diag_rate.py measures on the GPU"
    dev = "cuda:0"
    lines = [f"chain diagnostics, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} (sources "
             f"{_hip.source_sha()}), {a.reps} calls per figure ({a.rank_reps} for rank), split chains",
             f"{'shape':28s} {'entry':6s} {'ms/call':>9s} {'GB/s of one pass':>17s} {'lag blocks (max)':>17s} "
             f"{'host numpy s (scaled)':>22s}"]
    for name, M, S, Q, dtype, phi in (("weights 8x300x272474 fp32", 8, 300, 272474, torch.float32, 0.0),
                                      ("table 4x100x100000 fp64", 4, 100, 100000, torch.float64, 0.0),
                                      ("table ar1(0.9) 4x100x100000", 4, 100, 100000, torch.float64, 0.9)):
        x = _draws(M, S, Q, dtype, phi, dev)
        nbytes = x.numel() * x.element_size()
        pairs = diagnostics.rhat_ess(x, pairs=True)[2]
        blocks = int((2 * pairs.max().item() + 1) // diagnostics.LAG_BLOCK) + 1
        t0 = time.perf_counter()
        chain_diag_reference(x[..., :HOST_SLICE].cpu().numpy())
        host_s = (time.perf_counter() - t0) * Q / HOST_SLICE
        for entry, fn in (("rhat", lambda: diagnostics.split_rhat(x)), ("ess", lambda: diagnostics.rhat_ess(x))):
            ms = _event_ms(fn, a.reps)
            lines.append(f"{name:28s} {entry:6s} {ms:9.3f} {nbytes / ms * 1e-6:17.1f} "
                         f"{(blocks if entry == 'ess' else 0):17d} {host_s:22.1f}")
            print(lines[-1], flush=True)
        if not phi:
            t0 = time.perf_counter()
            rank_diag_reference(x[..., :HOST_SLICE].cpu().numpy())
            host_s = (time.perf_counter() - t0) * Q / HOST_SLICE
            ms = _event_ms(lambda: diagnostics.rank_rhat_ess(x), a.rank_reps, warmup=1)
            lines.append(f"{name:28s} {'rank':6s} {ms:9.3f} {nbytes / ms * 1e-6:17.1f} {0:17d} {host_s:22.1f}")
            print(lines[-1], flush=True)
        del x
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
