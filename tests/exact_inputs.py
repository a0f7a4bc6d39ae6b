"""Inputs on which fp32 arithmetic is exact, and the comparison that goes with them.

Small integers (or integers times one power of two) make every product and every partial sum of a contraction exactly
representable in fp32 whatever the order of summation, PROVIDED the sum of the absolute values of an output's products
stays within 2^24 (``assert_budget``).  A kernel then has to equal the float64 reference bit for bit: one lost, doubled
or misplaced term moves the result by at least one unit, and there is no tolerance to hide it in."""
import torch

BUDGET = float(2 ** 24)      # every integer of magnitude <= 2^24 is an fp32 number
NAN = float("nan")


def ints(shape, lo, hi, seed, nonzero=True):
    """float32 tensor of integers drawn uniformly from [lo, hi]; with ``nonzero`` (the default) zero is left out, so that
    every product of two such tensors is nonzero and every lost term shows.  Callers that want exact zeros at a ReLU or
    tied maxima in a pooling window pass ``nonzero=False``."""
    g = torch.Generator().manual_seed(seed)
    if not nonzero or lo > 0 or hi < 0:
        return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    v = torch.randint(lo, hi, tuple(shape), generator=g)       # hi - lo values: [lo, hi] without zero
    return (v + (v >= 0).long()).float()


GUARD = 256                  # elements behind every guarded output


def guarded(shape, dtype=torch.float32, device="cuda"):
    """a NaN-filled output of ``shape`` with GUARD more NaN elements directly behind it in the same allocation, so that a
    write past the output's end shows without a fault -> (the output, the whole buffer for ``assert_guard``)"""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + GUARD,), NAN, dtype=dtype, device=device)
    return whole[:n].view(tuple(shape)), whole


def assert_guard(whole, out, what):
    "the GUARD elements behind ``out`` still hold the NaN they were filled with"
    tail = whole[out.numel():]
    assert tail.numel() == GUARD and bool(torch.isnan(tail).all()), \
        f"{what}: {int((~torch.isnan(tail)).sum())} of the {GUARD} elements BEHIND the output were written"


def assert_budget(*abs_sums):
    """the condition that makes "exact" true: ``abs_sums`` are float64 tensors holding, per output element, the sum of
    the absolute values of its products -- the same operator applied to |x|, |w|, |dy| -- in units of the values' common
    power of two.  Every one must be <= 2^24; partial sums in any order are bounded by it."""
    assert abs_sums
    for i, s in enumerate(abs_sums):
        assert s.dtype == torch.float64, f"budget {i}: computed in {s.dtype}, not float64"
        worst = s.abs().max().item()
        assert worst <= BUDGET, f"budget {i}: sum of |products| reaches {worst:.0f} > 2^24: fp32 sums are not exact here"


def assert_exact(got, ref64, what):
    "``got`` (fp32 or fp64, any device) equals the float64 reference element for element; the message says where not"
    assert ref64.dtype == torch.float64, what
    g = got.detach().double().cpu()
    r = ref64.detach().cpu()
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)}, expected {tuple(r.shape)}"
    if torch.equal(g, r):
        return
    bad = ~(g == r)                                   # NaN differs from everything
    idx = bad.nonzero()
    lines = [f"  {tuple(i.tolist())}: got {g[tuple(i)].item()!r}, want {r[tuple(i)].item()!r}, "
             f"difference {(g[tuple(i)] - r[tuple(i)]).item()!r}" for i in idx[:8]]
    unwritten = int(torch.isnan(g).sum())
    raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ from the float64 reference; "
                         f"{unwritten} still hold the NaN the buffer was filled with\n" + "\n".join(lines))
