"""Time of the uncertainty path (``uncertainty.decompose``: ``sgmcmc_uncertainty_rows``; ``uncertainty.risk_coverage``:
two ``sgmcmc_stable_order`` + two ``sgmcmc_risk_coverage``; csrc/uncert_hip.inc) at the shapes of a stored run:

* decompose      -- 100 samples x 10,000 rows x 10 classes, fp64, with labels; beside ``calibration.ensemble_probs`` on
                    the same table (the pass it shares its log-sum-exp with) and the numpy restatement;
* risk_coverage  -- 10,000 rows, 0/1 losses scored by the max-prob, the call with its one host synchronisation (two
                    orderings, two curve launches, one read-back); the two orderings by themselves; beside the numpy
                    restatement.

Device times are device events around ``--reps`` calls after a warm-up call, profiler off, taken ``--windows`` times
(the spread is printed).  The table pass must read 8 E N C bytes and nothing else of that order, so its share of the
HBM rate is those bytes over the event time per call, against the 6.3 TB/s a streaming copy reaches on this chip and
the 8 TB/s of its data sheet; at 80 MB the table fits the 256 MiB Infinity Cache, so repeated calls may be served from
there: the second table, 1.28 GB (100 x 160,000 x 10), does not fit and is the figure to quote.

    python tools/uncertainty_rate.py [--reps 20] [--windows 5] [--out profiles/uncertainty_rate.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from bnn_priors_amd import _hip  # noqa: E402
from bnn_priors_amd import calibration as cal  # noqa: E402
from bnn_priors_amd import uncertainty as unc  # noqa: E402

TABLES = (("100 x 10000 x 10", 100, 10000, 10), ("100 x 160000 x 10", 100, 160000, 10))
RISK_ROWS = 10000
HBM_STREAM, HBM_SPEC = 6.3e12, 8.0e12


def _table(E, N, C, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    f = 2.0 * torch.randn((E, N, C), generator=g, dtype=torch.float64, device=dev)
    y = torch.randint(0, C, (N,), generator=g, device=dev)
    return f - f.logsumexp(-1, keepdim=True), y


def _event_ms(fn, reps, windows):
    "ms per call: the median, the least and the largest of ``windows`` windows of ``reps`` calls"
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncertainty_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "uncertainty_rate.py measures on the GPU"
    from uncertainty_reference import decompose_reference, risk_coverage_reference
    dev = "cuda:0"
    lines = [f"uncertainty decomposition and risk-coverage, {torch.cuda.get_device_name(0)}, library {_hip.library_sha()} "
             f"(sources {_hip.source_sha()}), device events, {a.windows} windows of {a.reps} calls: median (least .. largest)",
             f"{'call':34s} {'ms/call':>28s} {'table GB':>9s} {'TB/s':>6s} {'of 6.3':>7s} {'of 8.0':>7s} {'host numpy s':>13s}"]
    for name, E, N, C in TABLES:
        acc, y = _table(E, N, C, dev)
        gb = acc.numel() * 8
        host_s = None
        if N <= 10000:
            h_acc, h_y = acc.cpu().numpy(), y.cpu().numpy()
            t0 = time.perf_counter()
            decompose_reference(h_acc, h_y)
            host_s = time.perf_counter() - t0
        for what, fn in (("decompose", lambda: unc.decompose(acc, y)), ("ensemble_probs", lambda: cal.ensemble_probs(acc, y))):
            med, lo, hi = _event_ms(fn, a.reps, a.windows)
            rate = gb / (med * 1e-3)
            host = f"{host_s:13.3f}" if host_s is not None and what == "decompose" else f"{'':13s}"
            lines.append(f"{what + ' ' + name:34s} {f'{med:.4f} ({lo:.4f} .. {hi:.4f})':>28s} {gb * 1e-9:9.3f} "
                         f"{rate * 1e-12:6.2f} {rate / HBM_STREAM:7.1%} {rate / HBM_SPEC:7.1%} {host}")
            print(lines[-1], flush=True)
        if N == RISK_ROWS:
            u = unc.decompose(acc, y)
            wrong = 1 - u.hit
            med, lo, hi = _event_ms(lambda: unc.risk_coverage(u.max_prob, wrong), a.reps, a.windows)
            s, l = u.max_prob.cpu().numpy(), wrong.cpu().numpy().astype("float64")
            t0 = time.perf_counter()
            risk_coverage_reference(s, l)
            risk_coverage_reference(-l, l)
            host_s = time.perf_counter() - t0
            lines.append(f"{'risk_coverage ' + str(N) + ' rows':34s} {f'{med:.4f} ({lo:.4f} .. {hi:.4f})':>28s} {'':9s} "
                         f"{'':6s} {'':7s} {'':7s} {host_s:13.3f}")
            print(lines[-1], flush=True)
            # ... of which the two orderings (sgmcmc_stable_order of the scores and of -losses), by themselves
            sc, neg = u.max_prob.contiguous(), -wrong.to(torch.float64)
            med, lo, hi = _event_ms(lambda: (cal._order(sc, N, 1, 1, 0), cal._order(neg, N, 1, 1, 0)), a.reps, a.windows)
            lines.append(f"{'  of which 2 x stable_order':34s} {f'{med:.4f} ({lo:.4f} .. {hi:.4f})':>28s}")
            print(lines[-1], flush=True)
        del acc, y
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
