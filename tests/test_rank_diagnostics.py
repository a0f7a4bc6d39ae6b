"""Rank-normalised R-hat with bulk and tail ESS on the device (bnn_priors_amd/diagnostics.py rank_rhat_ess,
csrc/rank_hip.inc; the definition is in include/sgmcmc_hip.h and restated in tests/rank_diag_reference.py).

On the CPU: the restatement against scipy / numpy and against the cases that motivate it, the module's argument
checking, and a check that the inputs of the GPU cases leave the restatement's discrete decisions far from rounding
level.  On the GPU: the kernels against the restatement, part by part.

Tolerances (derived, not tuned):
* medians, quantiles and indicators are selections and singly rounded operations: bit-equal;
* z: any sound fp64 inverse normal distribution function is within a few ulp (Cephes documents <= 1e-15 relative), so
  1e-14 relative is more than tenfold slack;
* R-hat and ESS parts: rtol 1e-9 and K equal where the margin is >= 1e-9 -- the rule and derivation of
  tests/test_chain_diagnostics.py; a relative error eps in z moves rho_t by about 3 eps and tau by at most
  n 3 eps = 1.5e-11 at n = 512, below the 3e-11 that rule already budgets for summation order;
* rhat, ess_bulk, ess_tail follow from the parts by max / min and are compared the same way.
Quantities whose margin is below 1e-9 may be left out of the ESS / K comparison, at most 0.1 % of a case's quantities
(asserted).  Indicator sequences are 0/1 data whose Geyer pairs are often exactly zero at small n, so the seeds below
were searched so that NO quantity of any case is left out: ``test_gpu_case_inputs_leave_no_quantity_out`` asserts it."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from chain_diag_reference import chain_diag_reference
from rank_diag_reference import average_ranks, quantile, rank_diag_reference

from bnn_priors_amd import _hip
from bnn_priors_amd import diagnostics as D

RTOL = 1e-9
MARGIN = 1e-9
Z_RTOL = 1e-14
MAX_SEQ, MAX_CHAINS, OWN = D.MAX_SEQ, D.MAX_CHAINS, _hip.RANK_OWN
INVALID_VALUE = 1           # hipErrorInvalidValue
PARTS = ("rhat", "ess_bulk", "ess_tail", "rhat_bulk", "rhat_folded", "ess_lower", "ess_upper", "median", "q_lower",
         "q_upper")


def _ar1(rng, phi, M, S, Q):
    "stationary AR(1) with unit innovations; phi may be a [Q] vector"
    e = rng.standard_normal((M, S, Q))
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (Q,))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi ** 2)
    for s in range(1, S):
        x[:, s] = phi * x[:, s - 1] + e[:, s]
    return x


def _iid(seed, M, S, Q):
    return np.random.default_rng(seed).standard_normal((M, S, Q))


def _halves(seed, M, S, Q):
    "draws rounded to halves: average ranks, tied order statistics, and -0.0 next to 0.0"
    return np.round(_iid(seed, M, S, Q) * 2.0) / 2.0


# name -> (input [M, S, Q] fp64, split)
CASES = {
    "tile_q1": lambda: (_iid(201, 2, 24, 1), True),
    "tile_q63": lambda: (_iid(271, 2, 24, 63), True),
    "tile_q65": lambda: (_iid(268, 2, 24, 65), True),
    "tile_q130": lambda: (_iid(364, 2, 24, 130), True),
    "short_1x8": lambda: (_iid(SEEDS["short_1x8"], 1, 8, 5), True),
    "odd_2x9": lambda: (_iid(SEEDS["odd_2x9"], 2, 9, 5), True),
    "odd_3x41": lambda: (_iid(SEEDS["odd_3x41"], 3, 41, 5), True),
    "unsplit_1x4": lambda: (_iid(SEEDS["unsplit_1x4"], 1, 4, 5), False),
    "unsplit_2x5": lambda: (_iid(SEEDS["unsplit_2x5"], 2, 5, 5), False),
    "own_blocks": lambda: (_ar1(np.random.default_rng(28), [0.0, 0.5, 0.9], 4, 600, 3), True),
    "max_seq": lambda: (_ar1(np.random.default_rng(7), [0.0, 0.9, 0.99], 1, 2 * MAX_SEQ, 3), True),
    "max_chains": lambda: (_iid(40, MAX_CHAINS // 2, 8, 5), True),
    "ties": lambda: (_halves(26, 3, 40, 65), True),
    "cauchy": lambda: (np.random.default_rng(SEEDS["cauchy"]).standard_cauchy((4, 50, 65)), True),
    "layouts": lambda: (_ar1(np.random.default_rng(99), 0.5, 3, 40, 133), True),
}
# the cases whose seed the issue did not give: searched against the restatement from 0 upwards for the first seed that
# leaves no quantity out -- with so few quantities per case the first one tried already does
SEEDS = {"short_1x8": 0, "odd_2x9": 0, "odd_3x41": 0, "unsplit_1x4": 0, "unsplit_2x5": 0, "cauchy": 0, "nan_rule": 0}
F32_CASES = ("layouts",)


@functools.lru_cache(maxsize=None)
def _case(name, f32=False):
    "(x, split, reference), computed once and shared; f32: the values rounded to fp32 (the reference sees them widened)"
    x, split = CASES[name]()
    if f32:
        x = x.astype(np.float32)
    x.setflags(write=False)
    return x, split, rank_diag_reference(x.astype(np.float64), split)


def _nan_rule_inputs():
    "(x with an inf, a NaN and a constant column; the mask of those columns; the same draws with other columns there)"
    x = _iid(SEEDS["nan_rule"], 2, 20, 72)
    bad = np.zeros(72, dtype=bool)
    bad[[5, 7, 66]] = True
    clean = x.copy()
    x[1, 13, 5] = np.inf                     # in the second half of chain 1
    x[:, :, 7] = 2.0                         # constant
    x[0, 3, 66] = np.nan
    return x, bad, clean


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------

def test_reference_ranks_are_average_ranks_on_tied_data():
    v = _halves(3, 1, 60, 7)[0]
    v[:5, 2] = [-0.0, 0.0, 0.0, -0.0, 0.5]
    less = (v[None, :, :] < v[:, None, :]).sum(axis=1)
    equal = (v[None, :, :] == v[:, None, :]).sum(axis=1)
    assert (equal > 1).any()
    np.testing.assert_array_equal(average_ranks(v), less + (equal + 1) / 2)


QUANTILE_SHAPES = ((1200, 0), (47, 1), (48, 2), (9, 3), (40, 6))         # (N, seed): 50 columns of normal draws each
QUANTILE_PROBS = (0.05, 0.5, 0.95, 0.3)


def test_reference_quantiles_are_numpy_linear_quantiles():
    """within 1 ulp of ``np.quantile(method="linear")``, and the median of an even N bit-equal.  The restatement spells
    the interpolation out in numpy's order (from the upper neighbour once the fraction reaches 0.5): the form
    a + (b - a) t alone rounds apart from numpy's b - (b - a) (1 - t) in a few per cent of the columns, by far more
    than an ulp of the quantile where the neighbours a < 0 < b straddle zero."""
    differ = 0
    for N, seed in QUANTILE_SHAPES:
        v = _iid(seed, 1, N, 50)[0]
        for p in QUANTILE_PROBS:
            got, want = quantile(v, p), np.quantile(v, p, axis=0, method="linear")
            differ += int((got != want).sum())
            assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), (N, p)
            if p == 0.5 and N % 2 == 0:
                np.testing.assert_array_equal(got, want)
        if N % 2 == 1:                                                  # the median of an odd count is one draw
            np.testing.assert_array_equal(quantile(v, 0.5), np.sort(v, axis=0)[N // 2])
    print("quantiles that differ from numpy's in a bit:", differ)


def test_reference_flags_a_shifted_cauchy_chain_that_the_moments_miss():
    x = np.random.default_rng(0).standard_cauchy((4, 200, 500))
    x[3] += 3.0
    ranked, moments = rank_diag_reference(x).rhat, chain_diag_reference(x).rhat
    print("share above 1.01: rank-normalised", (ranked > 1.01).mean(), "moment-based", (moments > 1.01).mean(),
          "medians", np.median(ranked), np.median(moments))
    assert (ranked > 1.01).mean() >= 0.99
    assert (moments > 1.01).mean() < 0.25


def test_reference_folded_part_flags_a_chain_of_another_scale():
    x = _iid(0, 4, 200, 500)
    x[3] *= 3.0
    ref, moments = rank_diag_reference(x), chain_diag_reference(x).rhat
    print("share above 1.01: folded", (ref.rhat_folded > 1.01).mean(), "bulk", (ref.rhat_bulk > 1.01).mean(),
          "moment-based", (moments > 1.01).mean())
    assert (ref.rhat_folded > 1.01).mean() >= 0.99
    assert (ref.rhat_bulk > 1.01).mean() < 0.10
    assert (moments > 1.01).mean() < 0.10


def test_reference_iid_draws_are_worth_their_count():
    M, S, Q = 4, 300, 1000
    ref = rank_diag_reference(_iid(0, M, S, Q))
    bulk, tail = ref.ess_bulk.mean() / (M * S), ref.ess_tail.mean() / (M * S)
    print("iid: ess_bulk / N", bulk, "ess_tail / N", tail, "mean rhat", ref.rhat.mean())
    assert 0.85 <= bulk <= 1.1 and 0.85 <= tail <= 1.1
    assert 0.999 <= ref.rhat.mean() <= 1.01


def test_reference_bulk_parts_ignore_a_strictly_increasing_map():
    x = _iid(5, 3, 40, 20)
    a, b = rank_diag_reference(x), rank_diag_reference(np.exp(3.0 * x))
    for part in ("z", "rhat_bulk", "ess_bulk", "pairs_bulk"):
        np.testing.assert_array_equal(getattr(a, part), getattr(b, part))


def test_reference_nan_rule():
    x, bad, _ = _nan_rule_inputs()
    ref = rank_diag_reference(x)
    for part in ("rhat", "ess_bulk", "ess_tail"):
        assert np.isnan(getattr(ref, part)[bad]).all() and np.isfinite(getattr(ref, part)[~bad]).all(), part
    assert np.isnan(ref.median[[5, 66]]).all() and ref.median[7] == 2.0


def test_gpu_case_inputs_leave_no_quantity_out():
    "every GPU case's input keeps all margins >= 1e-9 in the restatement, in the bulk part and in the tail part"
    smallest = math.inf
    refs = [(name, f32, _case(name, f32)[2]) for name in CASES
            for f32 in ((False, True) if name in F32_CASES else (False,))]
    x, bad, clean = _nan_rule_inputs()
    refs += [("nan_rule", False, rank_diag_reference(x)), ("nan_rule clean", False, rank_diag_reference(clean))]
    for name, f32, ref in refs:
        for margin in (ref.margin_bulk, ref.margin_tail):
            assert (margin < MARGIN).sum() == 0, (name, f32, margin.min())
            smallest = min(smallest, margin.min())
    print("smallest margin over the GPU cases:", smallest)
    ties = _case("ties")
    assert np.isnan(ties[2].ess_tail).sum() == 1                        # a constant indicator: legitimately NaN
    zero, minus = ties[0] == 0.0, np.signbit(ties[0])
    assert ((zero & minus).any(axis=(0, 1)) & (zero & ~minus).any(axis=(0, 1))).any()      # a column with -0.0 and 0.0


# ---- CPU: argument checking and the summary ---------------------------------------------------------------------------

def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_hip, "lib", no_library)
    fn = D.rank_rhat_ess
    with pytest.raises(ValueError, match="CUDA"):
        fn(torch.zeros(2, 16, 3))                                       # a CPU tensor
    with pytest.raises(ValueError, match="float32 or float64"):
        fn(torch.zeros(2, 16, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="float32 or float64"):
        fn(torch.zeros(2, 16, 3, dtype=torch.float16))
    with pytest.raises(ValueError, match="chains, draws"):
        fn(torch.zeros(16))
    with pytest.raises(ValueError):
        fn(np.zeros((2, 16, 3)))
    with pytest.raises(ValueError, match="at least 4"):
        fn(torch.zeros(2, 7, 3))
    with pytest.raises(ValueError, match="at least 4"):
        fn(torch.zeros(2, 3, 3), split=False)
    with pytest.raises(ValueError, match=f"at most {MAX_SEQ}"):
        fn(torch.zeros(1, 2 * MAX_SEQ + 2, 1))
    with pytest.raises(ValueError, match=f"at most {MAX_SEQ}"):
        fn(torch.zeros(1, MAX_SEQ + 1, 1), split=False)
    with pytest.raises(ValueError, match=f"at most {MAX_CHAINS}"):
        fn(torch.zeros(MAX_CHAINS // 2 + 1, 8, 1))
    with pytest.raises(ValueError, match=f"at most {MAX_CHAINS}"):
        fn(torch.zeros(MAX_CHAINS + 1, 8, 1), split=False)
    good = torch.zeros(2, 16, 3)
    for probs in ((0.0, 0.95), (0.05, 1.0), (-0.1, 0.5), (0.05, math.nan), (0.05,), (0.05, 0.5, 0.95), 0.05, ("a", "b")):
        with pytest.raises(ValueError, match="tail_probs"):
            fn(good, tail_probs=probs)
    for probs in ((0.95, 0.05), (0.5, 0.5)):
        with pytest.raises(ValueError, match="increasing"):
            fn(good, tail_probs=probs)
    need = 64 * (16 * 32 + 72)                                          # 64 quantities of N = 32 draws
    with pytest.raises(ValueError, match=f"workspace_bytes.*{need} bytes"):
        fn(good, workspace_bytes=need - 1)
    with pytest.raises(ValueError, match="CUDA"):
        fn(good, workspace_bytes=need)                                  # enough: the next check is reached
    with pytest.raises(ValueError, match="CUDA"):
        D.weight_space({"w": torch.zeros(16, 3)}, chains=2, rank_normalised=True)
    with pytest.raises(ValueError, match="CUDA"):
        D.function_space([torch.zeros(8, 5, 3), torch.zeros(8, 5, 3)], rank_normalised=True)


def test_summary_takes_the_tail_ess():
    r = torch.tensor([1.0, 1.02, 1.2, math.nan], dtype=torch.float64)
    e = torch.tensor([100.0, 80.0, 60.0, 40.0], dtype=torch.float64)
    t = torch.tensor([math.nan, 70.0, 50.0, 30.0], dtype=torch.float64)
    plain, with_tail = D.summary(r, e), D.summary(r, e, ess_tail=t)
    assert "ess_tail_min" not in plain and with_tail.pop("ess_tail_min") == 30.0
    assert plain == with_tail and plain["nan"] == 1 and plain["ess_min"] == 60.0
    assert math.isnan(D.summary(r, e, ess_tail=torch.full_like(t, math.nan))["ess_tail_min"])
    with pytest.raises(ValueError, match="ess_tail"):
        D.summary(r, e, ess_tail=t[:3])


def test_limits_mirror_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "sgmcmc_hip.h")) as f:
        macros = dict(re.findall(r"^#define SGMCMC_RANK_(\w+) (\d+)", f.read(), re.M))
    assert {k: int(v) for k, v in macros.items()} == dict(OWN=_hip.RANK_OWN, MAX_PROBS=_hip.RANK_MAX_PROBS)
    assert D.RANK_CHUNK == 64 and D.RANK_DRAW_BYTES == 16 and D.RANK_QUANTITY_BYTES == 8 * 3 * _hip.RANK_MAX_PROBS
    assert MAX_SEQ * MAX_CHAINS < 2 ** 31                               # the counts fit int32


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _dev(x):
    return torch.from_numpy(np.array(x)).to("cuda:0")        # a copy: the shared case inputs are read-only


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32) if a.dtype == torch.float32 else a


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _all_same_bits(got, want):
    return len(got) == len(want) and all(_same_bits(a, b) for a, b in zip(got, want))


def _assert_bit_equal(got, want, what):
    "numpy fp64 arrays: NaN in the same places, the same bits elsewhere (both sides write zeros as +0.0)"
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), what
    assert (got[~nan].view(np.int64) == want[~nan].view(np.int64)).all(), what


def _check_against(x_dev, split, ref, what, **kw):
    "every part of rank_rhat_ess(x_dev) (any layout) against the restatement; returns the device results"
    got = D.rank_rhat_ess(x_dev, split, parts=True, **kw)
    three = D.rank_rhat_ess(x_dev, split, **kw)
    assert got._fields == PARTS and three._fields == PARTS[:3] and _all_same_bits(three, got[:3])
    shape = tuple(x_dev.shape[2:])
    assert all(t.shape == shape and t.dtype == torch.float64 for t in got)
    g = {k: _np(v).reshape(-1) for k, v in got._asdict().items()}
    keep_bulk, keep_tail = ref.margin_bulk >= MARGIN, ref.margin_tail >= MARGIN
    left_out = int((~keep_bulk).sum() + (~keep_tail).sum())
    everything = np.ones_like(keep_bulk)
    compared = (("rhat_bulk", everything), ("rhat_folded", everything), ("rhat", everything), ("ess_bulk", keep_bulk),
                ("ess_lower", keep_tail), ("ess_upper", keep_tail), ("ess_tail", keep_tail))
    with np.errstate(all="ignore"):
        errs = {k: np.nanmax(np.abs(g[k][keep] / getattr(ref, k)[keep] - 1.0), initial=0.0) for k, keep in compared}
    print(f"{what}: Q {everything.size} left out {left_out} max rel err " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert left_out <= 1e-3 * everything.size
    for k in ("median", "q_lower", "q_upper"):
        _assert_bit_equal(g[k], getattr(ref, k), (what, k))
    for k, keep in compared:
        np.testing.assert_allclose(g[k][keep], getattr(ref, k)[keep], rtol=RTOL, atol=0, equal_nan=True, err_msg=f"{what} {k}")
    return got


def _abi_arrays(x_dev, split, probs=(0.05, 0.95)):
    "the [J, n, Q] arrays and the pairs behind rank_rhat_ess, through the C ABI (x_dev [M, S, Q] contiguous)"
    lib = _hip.lib()
    M, S, Q = x_dev.shape
    n, J = (S // 2, 2 * M) if split else (S, M)
    dev, stream = x_dev.device, torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    z, zf = torch.empty((J, n, Q), **f64), torch.empty((J, n, Q), **f64)
    ostat, quant = torch.empty((6, Q), **f64), torch.empty((3, Q), **f64)
    lower, upper = (torch.empty((J, n, Q), dtype=torch.float32, device=dev) for _ in range(2))
    ess = torch.empty(Q, **f64)
    pairs = [torch.empty(Q, dtype=torch.int32, device=dev) for _ in range(3)]
    p = (ctypes.c_double * 3)(0.5, *probs)
    seqs = (x_dev.data_ptr(), int(x_dev.dtype == torch.float64), x_dev.stride(0), x_dev.stride(1), M, S, Q, int(split))
    assert lib.sgmcmc_chain_rank_scores(*seqs, None, p, 3, z.data_ptr(), ostat.data_ptr(), stream) == 0
    assert lib.sgmcmc_chain_quantiles(ostat.data_ptr(), M, S, int(split), p, 3, Q, quant.data_ptr(), stream) == 0
    assert lib.sgmcmc_chain_rank_scores(*seqs, quant[0].data_ptr(), None, 0, zf.data_ptr(), None, stream) == 0
    assert lib.sgmcmc_chain_tail_indicators(*seqs, quant[1].data_ptr(), quant[2].data_ptr(), lower.data_ptr(),
                                            upper.data_ptr(), stream) == 0
    for src, is_f64, k in ((z, 1, pairs[0]), (lower, 0, pairs[1]), (upper, 0, pairs[2])):
        assert lib.sgmcmc_chain_ess(src.data_ptr(), is_f64, n * Q, Q, J, n, Q, 0, ess.data_ptr(), None, k.data_ptr(),
                                    stream) == 0
    torch.cuda.synchronize()
    return dict(z=z, z_folded=zf, ind_lower=lower, ind_upper=upper, quant=quant, pairs_bulk=pairs[0],
                pairs_lower=pairs[1], pairs_upper=pairs[2])


def _check_arrays(x_dev, split, ref, what):
    "z within 1e-14 relative, indicators bit-equal, K equal where the margin allows; returns the largest z error"
    a = _abi_arrays(x_dev, split)
    worst = 0.0
    for k in ("z", "z_folded"):
        got, want = _np(a[k]), getattr(ref, k)
        assert (np.isnan(got) == np.isnan(want)).all(), (what, k)
        with np.errstate(all="ignore"):
            err = np.where(want == 0.0, np.where(got == 0.0, 0.0, np.inf), np.abs(got / want - 1.0))
        worst = max(worst, float(np.nanmax(err, initial=0.0)))
    print(f"{what}: max rel err of z {worst:.3e}")
    assert worst <= Z_RTOL, (what, worst)
    for k in ("ind_lower", "ind_upper"):
        got, want = _np(a[k]).astype(np.float64), getattr(ref, k)
        defined = ~np.isnan(want)                                       # all but the quantities with a non-finite draw
        np.testing.assert_array_equal(got[defined], want[defined], err_msg=f"{what} {k}")
    for k, margin in (("pairs_bulk", ref.margin_bulk), ("pairs_lower", ref.margin_tail), ("pairs_upper", ref.margin_tail)):
        keep = margin >= MARGIN
        np.testing.assert_array_equal(_np(a[k])[keep], getattr(ref, k)[keep], err_msg=f"{what} {k}")
    for i, k in enumerate(("median", "q_lower", "q_upper")):
        _assert_bit_equal(_np(a["quant"][i]), getattr(ref, k), (what, k))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != "layouts"])
def test_every_part_against_the_restatement(name):
    """quantity tiles (Q = 1, 63, 65, 130), minimal and odd sequences (a dropped middle draw; odd N: the median is one
    draw; N = 8 and 40: an own-block that is not full), N = 2400 (more than one workgroup's own draws and no multiple of
    them), the longest sequence, the most sequences, ties with -0.0, and Cauchy draws"""
    x, split, ref = _case(name)
    if name == "own_blocks":
        N = 2 * x.shape[0] * (x.shape[1] // 2)
        assert N > 4 * OWN and N % (4 * OWN) != 0                       # the last workgroup has own-blocks past the end
    if name in ("unsplit_1x4", "unsplit_2x5", "odd_2x9", "odd_3x41"):
        assert (x.shape[1] % 2 == 1) or not split
    xd = _dev(x)
    _check_against(xd, split, ref, name)
    _check_arrays(xd, split, ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_dtypes_and_strided_inputs(f32):
    x, split, ref = _case("layouts", f32)
    M, S, Q = x.shape
    xd = _dev(x)
    base = _check_against(xd, split, ref, "contiguous")
    _check_arrays(xd, split, ref, "contiguous")
    gathered = xd.reshape(M * S, Q)                                     # gather_samples' layout, viewed as weight_space does
    wide = torch.zeros(M, S + 3, Q + 5, dtype=xd.dtype, device=xd.device)
    wide[:, :S, :Q] = xd                                                # chain stride > S Q, draw stride > Q
    transposed = xd.permute(2, 0, 1).contiguous().permute(1, 2, 0)      # the quantity stride is not 1: made contiguous
    layouts = {"gathered view": gathered.unflatten(0, (M, S)), "padded": wide[:, :S, :Q], "transposed": transposed}
    assert layouts["padded"].stride(0) > S * Q and not layouts["transposed"][0, 0].is_contiguous()
    for what, v in layouts.items():
        assert _all_same_bits(D.rank_rhat_ess(v, split, parts=True), base), what     # the layout changes no bit
    broadcast = xd[:1].expand(2, S, Q)                                  # chain stride 0: every draw is tied with its copy
    same = D.rank_rhat_ess(broadcast, split, parts=True)
    want = D.rank_rhat_ess(broadcast.contiguous(), split, parts=True)
    assert _all_same_bits(same, want) and not torch.isnan(same.rhat).any() and not torch.isnan(same.ess_bulk).any()
    x3 = xd.reshape(M, S, Q // 7, 7)                                    # trailing dims: results take their shape
    got3 = D.rank_rhat_ess(x3, split, parts=True)
    assert all(t.shape == (Q // 7, 7) for t in got3)
    assert _all_same_bits([t.reshape(-1) for t in got3], base)
    if f32:                                                             # widening on load = widening on the host
        assert _all_same_bits(D.rank_rhat_ess(xd.double(), split, parts=True), base)


@pytest.mark.gpu
def test_results_are_deterministic_and_independent_of_grid_chunk_and_neighbours():
    x, split, _ = _case("layouts")
    xd = _dev(x)
    M, S, Q = x.shape
    a = D.rank_rhat_ess(xd, split, parts=True)
    assert _all_same_bits(D.rank_rhat_ess(xd, split, parts=True), a)
    part = D.rank_rhat_ess(xd[..., :65], split, parts=True)
    assert _all_same_bits(part, [v[:65] for v in a])
    shifted = D.rank_rhat_ess(xd[..., 3:], split, parts=True)           # another lane phase, other neighbours
    assert _all_same_bits(shifted, [v[3:] for v in a])
    N = 2 * M * (S // 2)
    small = 64 * (16 * N + 72)                                          # chunks of 64 quantities: 64 + 64 + 5
    assert Q > 2 * 64
    assert _all_same_bits(D.rank_rhat_ess(xd, split, parts=True, workspace_bytes=small), a)
    assert _all_same_bits(D.rank_rhat_ess(xd, split, parts=True, workspace_bytes=2 * small + 63), a)
    other = D.rank_rhat_ess(xd, split, tail_probs=(0.1, 0.8), parts=True)
    assert _same_bits(other.rhat, a.rhat) and _same_bits(other.ess_bulk, a.ess_bulk)
    ref = rank_diag_reference(x, split, tail_probs=(0.1, 0.8))
    _assert_bit_equal(_np(other.q_lower), ref.q_lower, "q_0.1")
    _assert_bit_equal(_np(other.q_upper), ref.q_upper, "q_0.8")


@pytest.mark.gpu
def test_nan_rule_and_its_neighbours():
    x, bad, clean = _nan_rule_inputs()
    ref = rank_diag_reference(x)
    got = _check_against(_dev(x), True, ref, "nan rule")
    _check_arrays(_dev(x), True, ref, "nan rule")
    for k in ("rhat", "ess_bulk", "ess_tail"):
        v = _np(getattr(got, k))
        assert np.isnan(v[bad]).all() and np.isfinite(v[~bad]).all(), k
    assert np.isnan(_np(got.median)[[5, 66]]).all() and _np(got.median)[7] == 2.0
    other = D.rank_rhat_ess(_dev(clean), True, parts=True)
    good = torch.from_numpy(~bad).to("cuda:0")
    assert _all_same_bits([v[good] for v in other], [v[good] for v in got])      # neighbours unaffected


@pytest.mark.gpu
def test_c_abi_refuses_out_of_range_arguments_and_writes_nothing():
    lib = _hip.lib()
    Q = 5
    x = torch.randn(2, 2 * MAX_SEQ + 2, Q, dtype=torch.float64, device="cuda:0")
    sentinel = -7.25
    N = 2 * 2 * 8                                                       # of the accepted call: 2 chains x 16 draws, split
    f64 = dict(dtype=torch.float64, device="cuda:0")
    z, ostat, quant = torch.full((N, Q), sentinel, **f64), torch.full((6, Q), sentinel, **f64), torch.full((3, Q), sentinel, **f64)
    centre = torch.zeros(Q, **f64)
    lower, upper = (torch.full((N, Q), sentinel, dtype=torch.float32, device="cuda:0") for _ in range(2))
    cs, ds = x.stride(0), x.stride(1)
    stream = torch.cuda.current_stream().cuda_stream
    p3, one = (ctypes.c_double * 3)(0.5, 0.05, 0.95), ctypes.c_double * 1

    def scores(xp=x.data_ptr(), cs=cs, chains=2, draws=16, Q=Q, split=1, probs=p3, nprobs=3, zp=z.data_ptr(),
               op=ostat.data_ptr()):
        return lib.sgmcmc_chain_rank_scores(xp, 1, cs, ds, chains, draws, Q, split, None, probs, nprobs, zp, op, stream)

    def quantiles(op=ostat.data_ptr(), chains=2, draws=16, split=1, probs=p3, nprobs=3, Q=Q, out=quant.data_ptr()):
        return lib.sgmcmc_chain_quantiles(op, chains, draws, split, probs, nprobs, Q, out, stream)

    def indicators(xp=x.data_ptr(), cs=cs, chains=2, draws=16, Q=Q, split=1, ql=centre.data_ptr(), qu=centre.data_ptr(),
                   lo=lower.data_ptr(), up=upper.data_ptr()):
        return lib.sgmcmc_chain_tail_indicators(xp, 1, cs, ds, chains, draws, Q, split, ql, qu, lo, up, stream)

    # (chains, draws, split): chains = 0; n = 3 split and unsplit; n = MAX_SEQ + 1 split and unsplit; J > MAX_CHAINS
    refused = [(0, 16, 1), (2, 7, 1), (2, 3, 0), (2, 2 * MAX_SEQ + 2, 1), (2, MAX_SEQ + 1, 0), (MAX_CHAINS // 2 + 1, 8, 1)]
    for chains, draws, split in refused:
        for fn in (scores, quantiles, indicators):
            assert fn(chains=chains, draws=draws, split=split) == INVALID_VALUE, (fn.__name__, chains, draws, split)
    for fn in (scores, quantiles, indicators):
        assert fn(Q=0) == INVALID_VALUE                                 # no quantities
    assert scores(cs=-1) == INVALID_VALUE and indicators(cs=-1) == INVALID_VALUE     # a negative stride
    assert scores(xp=None) == INVALID_VALUE and scores(zp=None) == INVALID_VALUE     # null required pointers
    assert scores(op=None) == INVALID_VALUE and scores(probs=None) == INVALID_VALUE  # ... required when nprobs > 0
    assert quantiles(op=None) == INVALID_VALUE and quantiles(out=None) == INVALID_VALUE
    assert quantiles(probs=None) == INVALID_VALUE and quantiles(nprobs=0) == INVALID_VALUE
    for name in ("xp", "ql", "qu", "lo", "up"):
        assert indicators(**{name: None}) == INVALID_VALUE, name
    for bad_p in (0.0, 1.0, -0.5, 1.5, math.nan):                       # p outside (0, 1)
        assert scores(probs=one(bad_p), nprobs=1) == INVALID_VALUE, bad_p
        assert quantiles(probs=one(bad_p), nprobs=1) == INVALID_VALUE, bad_p
    assert scores(probs=(ctypes.c_double * 4)(0.1, 0.2, 0.3, 0.4), nprobs=4) == INVALID_VALUE      # too many
    assert scores(nprobs=-1) == INVALID_VALUE
    torch.cuda.synchronize()
    assert all((t == sentinel).all() for t in (z, ostat, quant, lower, upper))
    # ... and the optional arguments may be null: no order statistics, no centre
    assert scores(probs=None, nprobs=0, op=None) == 0
    torch.cuda.synchronize()
    assert (ostat == sentinel).all() and not (z == sentinel).any()
    want = _abi_arrays(x[:, :16].contiguous(), True)
    assert _same_bits(z.reshape(4, 8, Q), want["z"])
    assert scores() == 0 and quantiles() == 0 and indicators(ql=quant[1].data_ptr(), qu=quant[2].data_ptr()) == 0
    torch.cuda.synchronize()
    assert _same_bits(quant, want["quant"]) and _same_bits(lower.reshape(4, 8, Q), want["ind_lower"])
    assert _same_bits(upper.reshape(4, 8, Q), want["ind_upper"])


@pytest.mark.gpu
def test_weight_space_and_function_space_rank_normalised_and_by_default():
    M, S = 3, 12
    g = torch.Generator().manual_seed(0)
    shapes = {"net.0.weight": (7, 5), "net.0.bias": (7,), "scale": ()}
    chains = []
    for m in range(M):
        d = {k: torch.randn((S,) + s, generator=g).to("cuda:0") for k, s in shapes.items()}
        d["net.1.running_mean"] = torch.randn((S, 7), generator=g, dtype=torch.float64).to("cuda:0")
        d["steps"] = torch.arange(S, device="cuda:0") * 10
        chains.append(d)
    names = set(shapes) | {"net.1.running_mean"}
    gathered = {k: torch.cat([c[k] for c in chains]) for k in chains[0]}
    ranked = (D.weight_space(chains, rank_normalised=True), D.weight_space(gathered, chains=M, rank_normalised=True))
    default = (D.weight_space(chains), D.weight_space(gathered, chains=M), D.weight_space(chains, rank_normalised=False))
    for k in names:
        stacked = torch.stack([c[k] for c in chains])
        want = D.rank_rhat_ess(stacked)
        assert want.rhat.shape == tuple(chains[0][k].shape[1:])
        for got in ranked:
            assert set(got) == names and type(got[k]) is D.RankDiagnostics and _all_same_bits(got[k], want), k
        today = D.rhat_ess(stacked)
        for got in default:                                             # the default is what it was: a plain pair
            assert set(got) == names and type(got[k]) is tuple and _all_same_bits(got[k], today), k
    unsplit = D.weight_space(chains, split=False, rank_normalised=True)
    assert _all_same_bits(unsplit["scale"], D.rank_rhat_ess(torch.stack([c["scale"] for c in chains]), split=False))

    g = torch.Generator().manual_seed(1)
    tables = [torch.log_softmax(torch.randn((10, 9, 4), generator=g, dtype=torch.float64), -1).to("cuda:0")
              for _ in range(3)]
    probs = torch.stack(tables).exp()
    got = D.function_space(tables, rank_normalised=True)
    assert type(got) is D.RankDiagnostics and got.rhat.shape == (9, 4) and _all_same_bits(got, D.rank_rhat_ess(probs))
    for plain in (D.function_space(tables), D.function_space(tables, rank_normalised=False)):
        assert type(plain) is tuple and _all_same_bits(plain, D.rhat_ess(probs))
    s = D.summary(got.rhat, got.ess_bulk, ess_tail=got.ess_tail)
    assert s["ess_tail_min"] == got.ess_tail.min().item() and s["ess_min"] == got.ess_bulk.min().item()
