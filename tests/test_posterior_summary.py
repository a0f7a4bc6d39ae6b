"""Posterior summaries with Monte Carlo standard errors on the device (bnn_priors_amd/diagnostics.py posterior_summary,
csrc/summary_hip.inc; the definition is in include/sgmcmc_hip.h and restated in tests/summary_reference.py).

On the CPU: the restatement against independent sources (np.sort, np.quantile, scipy.stats.beta.ppf, a transcription of
ArviZ's HDI, math.fsum, the iid case), the module's argument checking, and a check that the inputs of the GPU cases leave
every discrete decision of the restatement far from rounding level.  On the GPU: the kernels against the restatement,
part by part.

Tolerances (derived or measured as the issue prescribes, not tuned):
* the sorted column, quantiles, HDI bounds, lo, hi and mcse_quantile are selections and singly rounded subtractions:
  bit-equal;
* mean: |error| <= N 2^-53 mean|v| against math.fsum, the first-order bound of a length-N sum;
* m2, m4, sd: relative error <= 16 N 2^-53 against math.fsum: the terms are non-negative, so the sum costs (N - 1) 2^-53
  and the rest is slack for the centring's error through the second and fourth power; the inputs have |mean| <= 10 sd
  (asserted) so that the centring is well conditioned;
* ess_*, mcse_mean, mcse_sd: rtol 1e-9 and K equal where the margin is >= 1e-9 -- the rule and derivation of
  tests/test_chain_diagnostics.py;
* a, b: no bound was fixed in advance.  Measured on the CPU (``measure_betaincinv(gpu_case_triples(8))`` below: the
  root in mpmath arithmetic at 50 digits, over (alpha, beta, P) of the GPU cases -- up to eight quantities of every case
  and probability, alpha and beta from 1.1 to 15 900): scipy.special.betaincinv lies within 1.77e-15 relative of the
  root (the largest of 978 roots, at alpha = beta = 509.6; the median is 9e-17).  The device gets ten times that:
  AB_RTOL = 1.77e-14, relative.  (The same measurement of the device's arithmetic compiled for the host gave 3.8e-15 at
  worst.)  a and b depend on ess_q, which is itself compared at
  1e-9 only, so the device's a and b are compared with scipy's at the DEVICE's ess_q (alpha and beta formed by the same
  singly rounded operations);
* lo, hi: discrete.  A quantity whose a N or b N lies within (1e-9 + AB_RTOL) N of an integer (the ESS tolerance and the
  beta tolerance, both taken as absolute errors of a, b < 1) may be left out of the lo, hi and mcse_quantile comparison.
Quantities left out by a margin are at most 0.1 % of a case's quantities (asserted); the seeds below were searched
against the restatement so that NO quantity of any case is left out: ``test_gpu_case_inputs_leave_no_quantity_out``."""
import functools
import math
import os
import re

import numpy as np
import pytest
import scipy.special
import scipy.stats
import torch

from chain_diag_reference import chain_diag_reference
from rank_diag_reference import quantile
from summary_reference import LOWER_TAIL, UPPER_TAIL, beta_ranks, exact_moments, hdi, summary_reference

from bnn_priors_amd import _hip
from bnn_priors_amd import diagnostics as D

RTOL = 1e-9
MARGIN = 1e-9
SCIPY_BETAINCINV_DISTANCE = 1.77e-15        # measured: see the module docstring
AB_RTOL = 10 * SCIPY_BETAINCINV_DISTANCE
EPS = 2.0 ** -53
MAX_SEQ, MAX_CHAINS, MAX_DRAWS = D.MAX_SEQ, D.MAX_CHAINS, D.SUMMARY_MAX_DRAWS
INVALID_VALUE = 1           # hipErrorInvalidValue
PROBS, HDI_PROB = (0.05, 0.5, 0.95), 0.94
FIELDS = ("mean", "sd", "mcse_mean", "mcse_sd", "ess_mean", "ess_sd", "quantiles", "mcse_quantile", "ess_quantile",
          "hdi_lower", "hdi_upper")
PART_FIELDS = FIELDS + ("m2", "m4", "a", "b", "lo", "hi")


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
    "draws rounded to halves: tied order statistics, and -0.0 next to 0.0"
    return np.round(_iid(seed, M, S, Q) * 2.0) / 2.0


def _total(M, S, split):
    return 2 * M * (S // 2) if split else M * S


# (M, S, split) of the draw counts around a padding boundary: N = 4, 8, 8 (nine draws split), 1023, 1024, 1025, 1200
GEOMETRY = {"n4": (1, 4, False), "n8": (2, 4, False), "n8_odd": (1, 9, True), "n1023": (3, 341, False),
            "n1024": (1, 1024, True), "n1025": (5, 205, False), "n1200": (4, 300, True)}
# ... and the quantity counts around the tile width TQ at three of them: TQ = 64, 16, 8
TILE_GEOMETRY = {"n8": 64, "n1024": 16, "n1200": 8}


def _tile_counts(tq):
    return (1, tq - 1, tq, tq + 1, 2 * tq + 3)


# the first seed from 0 upwards at which the restatement leaves no quantity of the case out (searched; asserted below)
SEEDS = {}
CASES = {}
for _name, (_M, _S, _split) in GEOMETRY.items():
    CASES[_name] = (lambda M=_M, S=_S, split=_split, name=_name: (_iid(SEEDS.get(name, 0), M, S, 5), split))
for _name, _tq in TILE_GEOMETRY.items():
    _M, _S, _split = GEOMETRY[_name]
    for _Q in _tile_counts(_tq):
        _key = f"{_name}_q{_Q}"
        CASES[_key] = (lambda M=_M, S=_S, split=_split, Q=_Q, key=_key: (_iid(SEEDS.get(key, 0), M, S, Q), split))
CASES.update({
    "max_draws": lambda: (_ar1(np.random.default_rng(SEEDS.get("max_draws", 0)), [0.0, 0.5, 0.9], 16, 1024, 3), True),
    "ties": lambda: (_halves(SEEDS.get("ties", 0), 3, 40, 65), True),
    "cauchy": lambda: (np.random.default_rng(SEEDS.get("cauchy", 0)).standard_cauchy((4, 50, 65)), True),
    "ar1": lambda: (_ar1(np.random.default_rng(SEEDS.get("ar1", 0)), [0.0, 0.5, 0.9], 4, 600, 3), True),
    "layouts": lambda: (_ar1(np.random.default_rng(SEEDS.get("layouts", 0)), 0.5, 3, 40, 133), True),
})
SEEDS.update({"ties": 1, "layouts": 7})
F32_CASES = ("layouts",)


@functools.lru_cache(maxsize=None)
def _case(name, f32=False):
    "(x, split, reference), computed once and shared; f32: the values rounded to fp32 (the reference sees them widened)"
    x, split = CASES[name]()
    if f32:
        x = x.astype(np.float32)
    x.setflags(write=False)
    return x, split, summary_reference(x.astype(np.float64), PROBS, HDI_PROB, split)


def _nan_rule_inputs():
    "(x with an inf, a NaN and two constant columns; the mask of those columns; the same draws with other columns there)"
    x = _iid(SEEDS.get("nan_rule", 0), 2, 20, 72)
    bad = np.zeros(72, dtype=bool)
    bad[[5, 7, 9, 66]] = True
    clean = x.copy()
    x[1, 13, 5] = np.inf                     # in the second half of chain 1
    x[:, :, 7] = 2.0                         # constant
    x[:, :, 9] = 0.1                         # constant, and the sum of its copies is not a multiple of it
    x[0, 3, 66] = np.nan
    return x, bad, clean


def _left_out(ref, N):
    "how many quantities of a case the margins leave out of a comparison, per kind"
    return {"mean": int((ref.margin_mean < MARGIN).sum()), "sd": int((ref.margin_sd < MARGIN).sum()),
            "quantile": int((ref.margin_quantile < MARGIN).sum()),
            "rank": int((ref.margin_rank < (RTOL + AB_RTOL) * N).sum())}


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------

def test_reference_order_statistics_and_quantiles_are_numpys():
    """the sorted column is np.sort's; quantiles within 1 ulp of ``np.quantile(method="linear")`` and the median of an
    even N bit-equal -- the agreement rule of tests/test_rank_diagnostics.py"""
    for N, seed in ((1200, 0), (47, 1), (48, 2), (9, 3)):
        x = _iid(seed, 1, N, 50)
        ref = summary_reference(x, probs=(0.05, 0.5, 0.95, 0.3), split=False)
        np.testing.assert_array_equal(ref.ordered, np.sort(x[0], axis=0))
        for k, p in enumerate((0.05, 0.5, 0.95, 0.3)):
            want = np.quantile(x[0], p, axis=0, method="linear")
            assert (np.abs(ref.quantiles[k] - want) <= np.spacing(np.abs(want))).all(), (N, p)
            if p == 0.5 and N % 2 == 0:
                np.testing.assert_array_equal(ref.quantiles[k], want)
            np.testing.assert_array_equal(ref.quantiles[k], quantile(x[0], p))
    halves = _halves(4, 2, 30, 9)
    halves[0, :4, 2] = [-0.0, 0.0, -0.0, 0.5]
    ordered = summary_reference(halves).ordered
    assert not np.signbit(ordered[ordered == 0.0]).any()                # -0.0 is written as +0.0


def test_reference_beta_quantiles_are_scipy_stats():
    ess = np.array([3.7, 12.0, 160.0, 1234.5, 16000.0, 33000.0])
    for p in PROBS:
        a, b, lo, hi, _ = beta_ranks(ess, p, 16384)
        alpha, beta = ess * p + 1.0, ess * (1.0 - p) + 1.0
        np.testing.assert_allclose(a, scipy.stats.beta.ppf(LOWER_TAIL, alpha, beta), rtol=1e-13, atol=0)
        np.testing.assert_allclose(b, scipy.stats.beta.ppf(UPPER_TAIL, alpha, beta), rtol=1e-13, atol=0)
        assert (a < p + 1.0 / ess).all() and (b > p - 1.0 / ess).all() and (lo <= hi).all()
        # one standard error of a proportion p estimated from ess draws, on either side
        np.testing.assert_allclose((b - a)[2:] / 2, np.sqrt(p * (1 - p) / ess[2:]), rtol=0.1)


def _arviz_hdi(column, mass):
    "ArviZ's _hdi for a unimodal sample, transcribed: the narrowest of the intervals that hold floor(mass n) steps"
    ary = np.sort(column)
    n = len(ary)
    interval_idx_inc = int(np.floor(mass * n))
    n_intervals = n - interval_idx_inc
    interval_width = np.subtract(ary[interval_idx_inc:], ary[:n_intervals], dtype=np.float64)
    min_idx = np.argmin(interval_width)
    return ary[min_idx], ary[min_idx + interval_idx_inc]


def test_reference_hdi_is_arvizs_unimodal_hdi():
    for seed, N, mass in ((0, 8, 0.94), (1, 40, 0.5), (2, 41, 0.94), (3, 200, 0.8)):
        x = np.exp(_iid(seed, 1, N, 12))                                # skewed: the HDI is not the central interval
        ref = summary_reference(x, hdi_prob=mass, split=False)
        for q in range(12):
            assert (ref.hdi_lower[q], ref.hdi_upper[q]) == _arviz_hdi(x[0, :, q], mass), (seed, q)
    tied = summary_reference(_halves(5, 1, 40, 12), hdi_prob=0.5, split=False)      # the first of equal widths
    ordered = tied.ordered
    widths = ordered[20:] - ordered[:20]
    assert ((widths == widths.min(axis=0)).sum(axis=0) > 1).any()
    np.testing.assert_array_equal(tied.hdi_lower, ordered[widths.argmin(axis=0), np.arange(12)])
    lo, hi = hdi(ordered, 0.5)
    np.testing.assert_array_equal(hi - lo, widths.min(axis=0))


def test_reference_moments_against_fsum():
    x = _iid(0, 4, 300, 40) * 3.0 + 7.0
    ref = summary_reference(x)
    N = 1200
    mean, m2, m4 = exact_moments(x.reshape(4, 2, 150, 40).reshape(N, 40))
    assert (np.abs(ref.mean - mean) <= N * EPS * np.abs(x).mean(axis=(0, 1))).all()
    for got, want in ((ref.m2, m2), (ref.m4, m4), (ref.sd, np.sqrt(m2 * N / (N - 1)))):
        assert (np.abs(got / want - 1.0) <= 16 * N * EPS).all()
    np.testing.assert_allclose(ref.sd, x.reshape(N, 40).std(axis=0, ddof=1), rtol=1e-12)
    flat = summary_reference(np.full((2, 10, 3), 0.1))
    assert (flat.mean == 0.1).all() and (flat.sd == 0.0).all() and (flat.quantiles == 0.1).all()
    assert (flat.hdi_lower == 0.1).all() and (flat.hdi_upper == 0.1).all()
    for part in ("ess_mean", "ess_sd", "mcse_mean", "mcse_sd", "ess_quantile", "mcse_quantile"):
        assert np.isnan(getattr(flat, part)).all(), part


def test_reference_iid_normal_draws_have_the_textbook_standard_errors():
    """mcse_mean = sd / sqrt(N) and mcse_sd = sd / sqrt(2 N) for iid normal draws, within the ESS estimate's own spread
    (ess / N of iid draws scatters by about 10 % at N = 1200, the standard errors by half of that)"""
    M, S, Q = 4, 300, 500
    N = M * S
    ref = summary_reference(_iid(0, M, S, Q))
    of_mean, of_sd = ref.mcse_mean / (ref.sd / math.sqrt(N)), ref.mcse_sd / (ref.sd / math.sqrt(2 * N))
    print("iid: mcse_mean sqrt(N) / sd mean", of_mean.mean(), "range", of_mean.min(), of_mean.max(),
          "mcse_sd sqrt(2 N) / sd mean", of_sd.mean(), "range", of_sd.min(), of_sd.max())
    assert 0.97 <= of_mean.mean() <= 1.03 and 0.8 <= of_mean.min() and of_mean.max() <= 1.25
    assert 0.95 <= of_sd.mean() <= 1.05 and 0.75 <= of_sd.min() and of_sd.max() <= 1.35
    # the standard error of the median of normal draws: sd sqrt(pi / 2) / sqrt(N)
    of_median = ref.mcse_quantile[1] / (ref.sd * math.sqrt(math.pi / 2 / N))
    assert 0.9 <= of_median.mean() <= 1.1
    # ... and an autocorrelated chain has fewer effective draws and a larger error
    slow = summary_reference(_ar1(np.random.default_rng(1), 0.9, M, S, 50))
    ratio = slow.mcse_mean / (slow.sd / math.sqrt(N))
    print("AR(1) 0.9: mcse_mean sqrt(N) / sd mean", ratio.mean())      # sqrt((1 + phi) / (1 - phi)) = 4.4
    assert 3.0 <= ratio.mean() <= 6.0


def _mp_betainc(a, b, x):
    """I_x(a, b) in mpmath's working precision: x^a (1 - x)^b / (a B(a, b)) 2F1(a + b, 1; a + 1; x), summed term by term
    below the mean and through 1 - I_{1-x}(b, a) above it, so that every term is positive and shrinks (mpmath's own
    betainc does not converge at parameters of 10^4: its series alternates)"""
    import mpmath
    if x * (a + b) > a:
        return 1 - _mp_betainc(b, a, 1 - x)
    front = mpmath.exp(a * mpmath.log(x) + b * mpmath.log(1 - x) + mpmath.loggamma(a + b) - mpmath.loggamma(a)
                       - mpmath.loggamma(b)) / a
    term = total = mpmath.mpf(1)
    k = 0
    while term > total * mpmath.mpf(10) ** (-mpmath.mp.dps):
        term *= (a + b + k) * x / (a + 1 + k)
        total += term
        k += 1
    return front * total


def measure_betaincinv(triples, digits=50):
    "the relative distances of scipy.special.betaincinv from the root of I_x(alpha, beta) = P in mpmath arithmetic"
    import mpmath
    out = []
    with mpmath.workdps(digits):
        for alpha, beta, P in triples:
            got = mpmath.mpf(float(scipy.special.betaincinv(alpha, beta, P)))
            al, be, target = mpmath.mpf(float(alpha)), mpmath.mpf(float(beta)), mpmath.mpf(P)
            root = mpmath.findroot(lambda t: _mp_betainc(al, be, t) - target, (got * (1 - 1e-9), got * (1 + 1e-9)),
                                   solver="illinois")
            out.append(float(abs(got - root) / root))
    return out


def gpu_case_triples(per_case=8):
    "(alpha, beta, P) of ``per_case`` quantities of every GPU case and probability"
    out = []
    for name in CASES:
        ess_q = _case(name)[2].ess_quantile
        for k, p in enumerate(PROBS):
            e = ess_q[k][np.isfinite(ess_q[k])][:per_case]
            out += [(v * p + 1.0, v * (1.0 - p) + 1.0, P) for v in e for P in (LOWER_TAIL, UPPER_TAIL)]
    return out


def test_beta_tolerance_is_ten_times_scipys_measured_distance():
    "a sample of the measurement behind AB_RTOL (the whole of it takes minutes): the recorded figure still holds"
    triples = gpu_case_triples(per_case=1)[::20]
    worst = max(measure_betaincinv(triples))
    print(f"scipy.special.betaincinv against mpmath over {len(triples)} roots: {worst:.2e} relative")
    assert worst <= SCIPY_BETAINCINV_DISTANCE and AB_RTOL == 10 * SCIPY_BETAINCINV_DISTANCE


def test_gpu_case_inputs_leave_no_quantity_out():
    """every GPU case's input keeps all margins of the restatement above the level at which a comparison may leave a
    quantity out, and is well conditioned for the moments' bound"""
    inputs = [(name, f32, _case(name, f32)) for name in CASES for f32 in ((False, True) if name in F32_CASES else (False,))]
    x, bad, clean = _nan_rule_inputs()
    inputs += [("nan_rule", False, (x, True, summary_reference(x))), ("nan_rule clean", False, (clean, True, summary_reference(clean)))]
    for name, f32, (x, split, ref) in inputs:
        N = _total(x.shape[0], x.shape[1], split)
        out = _left_out(ref, N)
        assert not any(out.values()), (name, f32, out)
        ok = np.isfinite(ref.sd) & (ref.sd > 0)
        assert (np.abs(ref.mean[ok]) <= 10 * ref.sd[ok]).all(), name
    for name, tq in TILE_GEOMETRY.items():
        assert D.summary_tile(_total(*GEOMETRY[name])) == tq
    ties = _case("ties")
    zero, minus = ties[0] == 0.0, np.signbit(ties[0])
    assert ((zero & minus).any(axis=(0, 1)) & (zero & ~minus).any(axis=(0, 1))).any()      # a column with -0.0 and 0.0
    assert _total(*_case("max_draws")[0].shape[:2], True) == MAX_DRAWS


# ---- CPU: argument checking -------------------------------------------------------------------------------------------

def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_hip, "lib", no_library)
    fn = D.posterior_summary
    with pytest.raises(ValueError, match="CUDA"):
        fn(torch.zeros(2, 16, 3))                                       # a CPU tensor
    with pytest.raises(ValueError, match="float32 or float64"):
        fn(torch.zeros(2, 16, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="chains, draws"):
        fn(torch.zeros(16))
    with pytest.raises(ValueError):
        fn(np.zeros((2, 16, 3)))
    with pytest.raises(ValueError, match="at least 4"):
        fn(torch.zeros(2, 7, 3))
    with pytest.raises(ValueError, match=f"at most {MAX_SEQ}"):
        fn(torch.zeros(1, MAX_SEQ + 1, 1), split=False)
    with pytest.raises(ValueError, match=f"at most {MAX_CHAINS}"):
        fn(torch.zeros(MAX_CHAINS + 1, 8, 1), split=False)
    # more than 16384 draws: 16385 has no factorisation into J <= 64 sequences of n <= 512 draws (5 x 29 x 113), so it is
    # refused as one sequence; the smallest count above the limit that the ESS kernel would take is 16388 = 34 x 482
    with pytest.raises(ValueError, match="at most"):
        fn(torch.zeros(1, 16385, 1), split=False)
    with pytest.raises(ValueError, match=f"16388 draws: at most {MAX_DRAWS}"):
        fn(torch.zeros(34, 482, 1), split=False)
    with pytest.raises(ValueError, match=f"16388 draws: at most {MAX_DRAWS}"):
        fn(torch.zeros(17, 964, 1))
    good = torch.zeros(2, 16, 3)
    for probs in ((0.0, 0.95), (0.05, 1.0), (-0.1, 0.5), (0.05, math.nan), 0.05, ("a", "b")):
        with pytest.raises(ValueError, match="probs"):
            fn(good, probs=probs)
    for mass in (0.0, 1.0, -0.5, math.nan, "a", None, 0.03):            # 0.03 x 32 draws: an interval of no step
        with pytest.raises(ValueError, match="hdi_prob"):
            fn(good, hdi_prob=mass)
    need = 64 * 16 * 32                                                 # 64 quantities of N = 32 draws
    with pytest.raises(ValueError, match=f"workspace_bytes.*{need} bytes"):
        fn(good, workspace_bytes=need - 1)
    with pytest.raises(ValueError, match="CUDA"):
        fn(good, workspace_bytes=need)                                  # enough: the next check is reached
    with pytest.raises(ValueError, match="CUDA"):
        fn(good, probs=(0.5,) * 7)                                      # any number of probabilities
    with pytest.raises(ValueError, match="CUDA"):
        D.weight_space_summary({"w": torch.zeros(16, 3)}, chains=2)
    with pytest.raises(ValueError, match="hdi_prob"):
        D.weight_space_summary({"w": torch.zeros(16, 3)}, chains=2, hdi_prob=2.0)
    with pytest.raises(ValueError, match="chains=M"):
        D.weight_space_summary({"w": torch.zeros(16, 3)})
    with pytest.raises(ValueError, match="CUDA"):
        D.function_space_summary([torch.zeros(8, 5, 3), torch.zeros(8, 5, 3)])
    with pytest.raises(ValueError, match="tables"):
        D.function_space_summary([torch.zeros(8, 5, 3), torch.zeros(8, 5, 4)])
    with pytest.raises(ValueError):
        D.summary_tile(MAX_DRAWS + 1)


def test_limits_mirror_the_header_and_the_library():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "sgmcmc_hip.h")) as f:
        macros = dict(re.findall(r"^#define SGMCMC_SUMMARY_(\w+) (\d+)", f.read(), re.M))
    assert {k: int(v) for k, v in macros.items()} == dict(MAX_DRAWS=_hip.SUMMARY_MAX_DRAWS, MAX_TILE=_hip.SUMMARY_MAX_TILE)
    assert D.SUMMARY_MAX_DRAWS == 16384 and D.SUMMARY_CHUNK == _hip.SUMMARY_MAX_TILE
    assert D.SUMMARY_DRAW_BYTES == 16 and D.SUMMARY_QUANTITY_BYTES == 0
    assert {"posterior_summary", "weight_space_summary", "function_space_summary"} <= set(D.__all__)
    assert D.PosteriorSummary._fields == FIELDS and D.PosteriorSummaryParts._fields == PART_FIELDS
    lib = _hip.lib()                                                    # host arithmetic only: no GPU is needed
    for N in list(range(0, 70)) + [255, 256, 257, 1023, 1024, 1025, 1200, 8192, 8193, MAX_DRAWS, MAX_DRAWS + 1]:
        tq = lib.sgmcmc_summary_tile_quantities(N)
        if 4 <= N <= MAX_DRAWS:
            pad = max(4, 1 << (N - 1).bit_length())
            assert tq == D.summary_tile(N) >= 1 and pad >= N and (pad // 2 < N or pad == 4)
            assert pad * tq * 8 <= 128 * 1024 and (tq == 64 or 2 * pad * tq * 8 > 128 * 1024)
        else:
            assert tq == 0


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
    assert got.shape == want.shape and (np.isnan(got) == nan).all(), what
    assert (got[~nan].view(np.int64) == want[~nan].view(np.int64)).all(), what


def _abi_sorted(x_dev, split):
    "sgmcmc_summary_sort through the C ABI (x_dev [M, S, Q] with a contiguous last dimension) -> [N, Q]"
    M, S, Q = x_dev.shape
    out = torch.full((_total(M, S, split), Q), -7.25, dtype=torch.float64, device=x_dev.device)
    err = _hip.lib().sgmcmc_summary_sort(x_dev.data_ptr(), int(x_dev.dtype == torch.float64), x_dev.stride(0),
                                         x_dev.stride(1), M, S, Q, int(split), out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    assert err == 0
    return out


def _check_against(x_dev, split, ref, what, **kw):
    "every part of posterior_summary(x_dev) (any layout) against the restatement; returns the device results"
    got = D.posterior_summary(x_dev, PROBS, HDI_PROB, split, parts=True, **kw)
    plain = D.posterior_summary(x_dev, PROBS, HDI_PROB, split, **kw)
    assert got._fields == PART_FIELDS and plain._fields == FIELDS and _all_same_bits(plain, got[:len(FIELDS)])
    shape, P = tuple(x_dev.shape[2:]), len(PROBS)
    for k, t in got._asdict().items():
        per_prob = k in ("quantiles", "mcse_quantile", "ess_quantile", "a", "b", "lo", "hi")
        assert t.shape == ((P,) + shape if per_prob else shape), k
        assert t.dtype == (torch.int32 if k in ("lo", "hi") else torch.float64), k
    g = {k: _np(v).reshape(P, -1) if v.dim() > len(shape) else _np(v).reshape(-1) for k, v in got._asdict().items()}
    xs = _np(x_dev).astype(np.float64).reshape(x_dev.shape[0], x_dev.shape[1], -1)
    M, S, Q = xs.shape
    N = _total(M, S, split)
    out = _left_out(ref, N)
    assert sum(out.values()) <= 1e-3 * Q, (what, out)

    # selections and singly rounded subtractions: bit-equal
    _assert_bit_equal(_np(_abi_sorted(x_dev.reshape(M, S, Q), split)), ref.ordered, (what, "sorted"))
    for k in ("quantiles", "hdi_lower", "hdi_upper"):
        _assert_bit_equal(g[k], getattr(ref, k), (what, k))

    # moments against correctly rounded sums
    fine = ~np.isnan(ref.mean)
    v = ref.ordered[:, fine]                                            # any order: fsum is exact
    mean, m2, m4 = exact_moments(v)
    assert np.isnan(g["mean"][~fine]).all() and np.isnan(g["sd"][~fine]).all()
    err_mean = np.abs(g["mean"][fine] - mean)
    bound = N * EPS * np.abs(v).mean(axis=0)
    varies = m2 > 0
    assert (g["m2"][fine][~varies] == 0).all() and (g["sd"][fine][~varies] == 0).all()
    assert (g["mean"][fine][~varies] == mean[~varies]).all()
    rel = {k: np.abs(g[k][fine][varies] / want[varies] - 1.0)
           for k, want in (("m2", m2), ("m4", m4), ("sd", np.sqrt(m2 * N / (N - 1))))}
    print(f"{what}: Q {Q} N {N} left out {out} mean err / bound {np.max(err_mean / np.maximum(bound, 1e-300), initial=0):.2e} "
          + " ".join(f"{k} rel err / bound {np.max(e, initial=0) / (16 * N * EPS):.2e}" for k, e in rel.items()))
    assert (err_mean <= bound).all(), what
    for k, e in rel.items():
        assert (e <= 16 * N * EPS).all(), (what, k)

    # effective sample sizes and the standard errors that follow from them
    keep_mean, keep_sd, keep_q = ref.margin_mean >= MARGIN, ref.margin_sd >= MARGIN, ref.margin_quantile >= MARGIN
    for k, keep in (("ess_mean", keep_mean), ("mcse_mean", keep_mean), ("ess_sd", keep_sd), ("mcse_sd", keep_sd),
                    ("ess_quantile", keep_q)):
        np.testing.assert_allclose(g[k][keep], getattr(ref, k)[keep], rtol=RTOL, atol=0, equal_nan=True,
                                   err_msg=f"{what} {k}")

    # the beta quantiles at the device's own ess_q, the ranks and the order statistics they select
    worst = 0.0
    cols = np.arange(Q)
    for k, p in enumerate(PROBS):
        a, b, lo, hi, margin = beta_ranks(g["ess_quantile"][k], p, N)
        for name, want in (("a", a), ("b", b)):
            have = g[name][k]
            assert (np.isnan(have) == np.isnan(want)).all(), (what, name, p)
            ok = ~np.isnan(want)
            worst = max(worst, float(np.max(np.abs(have[ok] / want[ok] - 1.0), initial=0.0)))
        keep = (margin >= (RTOL + AB_RTOL) * N) & keep_q[k]
        assert (~keep).sum() <= 1e-3 * Q
        np.testing.assert_array_equal(g["lo"][k][keep], lo[keep], err_msg=f"{what} lo {p}")
        np.testing.assert_array_equal(g["hi"][k][keep], hi[keep], err_msg=f"{what} hi {p}")
        with np.errstate(all="ignore"):
            want = np.where(lo < 0, np.nan, (ref.ordered[hi, cols] - ref.ordered[lo, cols]) / 2.0)
        _assert_bit_equal(g["mcse_quantile"][k][keep], want[keep], (what, "mcse_quantile", p))
        np.testing.assert_array_equal(g["lo"][k][keep_q[k]], ref.lo[k][keep_q[k]], err_msg=f"{what} lo against the restatement")
        np.testing.assert_array_equal(g["hi"][k][keep_q[k]], ref.hi[k][keep_q[k]], err_msg=f"{what} hi against the restatement")
        _assert_bit_equal(g["mcse_quantile"][k][keep_q[k]], ref.mcse_quantile[k][keep_q[k]], (what, "mcse_quantile", p))
    print(f"{what}: a, b against scipy at the device's ess_q: {worst:.2e} relative (allowed {AB_RTOL:.1e})")
    assert worst <= AB_RTOL, (what, worst)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != "layouts"])
def test_every_part_against_the_restatement(name):
    """draw counts around a padding boundary of the sorting network (N = 4, 8, nine draws split, 1023, 1024, 1025, 1200),
    quantity counts around the tile width at three tile widths, the most draws (one column per workgroup), ties with
    -0.0, Cauchy draws and AR(1) chains"""
    x, split, ref = _case(name)
    _check_against(_dev(x), split, ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_dtypes_and_strided_inputs(f32):
    x, split, ref = _case("layouts", f32)
    M, S, Q = x.shape
    xd = _dev(x)
    base = _check_against(xd, split, ref, "contiguous")
    wide = torch.zeros(M, S + 3, Q + 5, dtype=xd.dtype, device=xd.device)
    wide[:, :S, :Q] = xd                                                # chain stride > S Q, draw stride > Q
    transposed = xd.permute(2, 0, 1).contiguous().permute(1, 2, 0)      # the quantity stride is not 1: made contiguous
    layouts = {"gathered view": xd.reshape(M * S, Q).unflatten(0, (M, S)), "padded": wide[:, :S, :Q],
               "transposed": transposed}
    assert layouts["padded"].stride(0) > S * Q and not layouts["transposed"][0, 0].is_contiguous()
    for what, v in layouts.items():
        assert _all_same_bits(D.posterior_summary(v, PROBS, HDI_PROB, split, parts=True), base), what
    assert _same_bits(_abi_sorted(wide[:, :S, :Q], split), _abi_sorted(xd, split))
    x3 = xd.reshape(M, S, Q // 7, 7)                                    # trailing dims: results take their shape
    got3 = D.posterior_summary(x3, PROBS, HDI_PROB, split, parts=True)
    assert got3.mean.shape == (Q // 7, 7) and got3.quantiles.shape == (3, Q // 7, 7) and got3.lo.shape == (3, Q // 7, 7)
    assert _all_same_bits([t.reshape(b.shape) for t, b in zip(got3, base)], base)
    if f32:                                                             # widening on load = widening on the host
        assert _all_same_bits(D.posterior_summary(xd.double(), PROBS, HDI_PROB, split, parts=True), base)


@pytest.mark.gpu
def test_results_are_deterministic_and_independent_of_chunk_and_neighbours():
    x, split, ref = _case("layouts")
    xd = _dev(x)
    M, S, Q = x.shape
    N = _total(M, S, split)
    a = D.posterior_summary(xd, PROBS, HDI_PROB, split, parts=True)
    assert _all_same_bits(D.posterior_summary(xd, PROBS, HDI_PROB, split, parts=True), a)       # two calls
    part = D.posterior_summary(xd[..., :65], PROBS, HDI_PROB, split, parts=True)
    assert _all_same_bits(part, [v[..., :65] for v in a])
    shifted = D.posterior_summary(xd[..., 3:], PROBS, HDI_PROB, split, parts=True)   # another lane phase, other neighbours
    assert _all_same_bits(shifted, [v[..., 3:] for v in a])
    small = 64 * 16 * N                                                 # chunks of 64 quantities: 64 + 64 + 5
    assert Q > 2 * 64
    for workspace in (small, 2 * small + 63):                           # two chunkings
        assert _all_same_bits(D.posterior_summary(xd, PROBS, HDI_PROB, split, parts=True, workspace_bytes=workspace), a)
    # other probabilities, an odd and an even count of them, and another mass: the rest is unchanged
    probs = (0.1, 0.8, 0.5, 0.25)
    other = D.posterior_summary(xd, probs, 0.5, split, parts=True)
    want = summary_reference(x, probs, 0.5, split)
    assert _all_same_bits(other[:6], a[:6]) and _same_bits(other.quantiles[2], a.quantiles[1])
    assert _same_bits(other.mcse_quantile[2], a.mcse_quantile[1]) and _same_bits(other.ess_quantile[2], a.ess_quantile[1])
    for k in ("quantiles", "hdi_lower", "hdi_upper"):
        _assert_bit_equal(_np(getattr(other, k)), getattr(want, k), k)
    np.testing.assert_allclose(_np(other.ess_quantile), want.ess_quantile, rtol=RTOL)
    one = D.posterior_summary(xd, (0.8,), 0.5, split, parts=True)
    assert _all_same_bits([t[0] for t in one[6:9]], [t[1] for t in other[6:9]])
    none = D.posterior_summary(xd, (), 0.5, split)
    assert none.quantiles.shape == (0, Q) and _all_same_bits(none[:6], a[:6])


@pytest.mark.gpu
def test_nan_rule_and_its_neighbours():
    x, bad, clean = _nan_rule_inputs()
    ref = summary_reference(x)
    got = _check_against(_dev(x), True, ref, "nan rule")
    for k in PART_FIELDS:
        v = _np(getattr(got, k)).reshape(-1, 72).astype(np.float64)
        if k in ("lo", "hi"):
            assert (v[:, bad] == -1).all() and (v[:, ~bad] >= 0).all(), k
            continue
        assert np.isnan(v[:, [5, 66]]).all() and np.isfinite(v[:, ~bad]).all(), k       # a non-finite draw: NaN in everything
        constant = v[:, [7, 9]]
        if k in ("mean", "quantiles", "hdi_lower", "hdi_upper"):
            assert (constant == np.array([2.0, 0.1])).all(), k
        elif k in ("sd", "m2", "m4"):
            assert (constant == 0.0).all(), k
        else:
            assert np.isnan(constant).all(), k
    other = D.posterior_summary(_dev(clean), PROBS, HDI_PROB, True, parts=True)
    good = torch.from_numpy(~bad).to("cuda:0")
    assert _all_same_bits([v[..., good] for v in other], [v[..., good] for v in got])    # neighbours unaffected
    # a real +inf is not taken for the padding of the sorting network: N = 40 is padded to 64
    ordered = _np(_abi_sorted(_dev(x), True))
    assert np.isnan(ordered[:, [5, 66]]).all() and np.isfinite(ordered[:, ~bad]).all()


@pytest.mark.gpu
def test_c_abi_refuses_out_of_range_arguments_and_writes_nothing():
    lib = _hip.lib()
    Q, sentinel = 5, -7.25
    x = torch.randn(34, 482, Q, dtype=torch.float64, device="cuda:0")
    N = 2 * 2 * 8                                                       # of the accepted call: 2 chains x 16 draws, split
    f64 = dict(dtype=torch.float64, device="cuda:0")
    ordered, csq = torch.full((N, Q), sentinel, **f64), torch.full((N, Q), sentinel, **f64)
    rows = torch.full((12, Q), sentinel, **f64)
    ranks = torch.full((2, Q), -7, dtype=torch.int32, device="cuda:0")
    ess = torch.full((Q,), 20.0, **f64)
    cs, ds = x.stride(0), x.stride(1)
    stream = torch.cuda.current_stream().cuda_stream
    r = [rows[i].data_ptr() for i in range(12)]

    def sort(xp=x.data_ptr(), cs=cs, chains=2, draws=16, Q=Q, split=1, out=ordered.data_ptr()):
        return lib.sgmcmc_summary_sort(xp, 1, cs, ds, chains, draws, Q, split, out, stream)

    def moments(xp=x.data_ptr(), cs=cs, chains=2, draws=16, Q=Q, split=1, mean=r[0], out=csq.data_ptr()):
        return lib.sgmcmc_summary_moments(xp, 1, cs, ds, chains, draws, Q, split, mean, r[1], r[2], r[3], out, stream)

    def quantiles(src=ordered.data_ptr(), chains=2, draws=16, split=1, p=0.3, Q=Q, out=r[4]):
        return lib.sgmcmc_summary_quantile(src, chains, draws, split, p, Q, out, stream)

    def interval(src=ordered.data_ptr(), chains=2, draws=16, split=1, p=0.9, Q=Q, out=r[5]):
        return lib.sgmcmc_summary_hdi(src, chains, draws, split, p, Q, out, r[6], stream)

    def mcse_q(src=ordered.data_ptr(), chains=2, draws=16, split=1, p=0.3, Q=Q, out=r[7], e=ess.data_ptr()):
        return lib.sgmcmc_summary_mcse_quantile(src, chains, draws, split, p, e, Q, out, r[8], r[9],
                                                ranks[0].data_ptr(), ranks[1].data_ptr(), stream)

    every = (sort, moments, quantiles, interval, mcse_q)
    # (chains, draws, split): chains = 0; n = 3; n > MAX_SEQ; J > MAX_CHAINS; N = 16388 = 34 x 482 unsplit and 17 x 964 split
    refused = [(0, 16, 1), (2, 7, 1), (2, 3, 0), (2, MAX_SEQ + 1, 0), (MAX_CHAINS // 2 + 1, 8, 1), (1, 16385, 0),
               (34, 482, 0), (17, 964, 1)]
    for chains, draws, split in refused:
        for fn in every:
            assert fn(chains=chains, draws=draws, split=split) == INVALID_VALUE, (fn.__name__, chains, draws, split)
    for fn in every:
        assert fn(Q=0) == INVALID_VALUE                                 # no quantities
    assert sort(cs=-1) == INVALID_VALUE and moments(cs=-1) == INVALID_VALUE
    assert sort(xp=None) == INVALID_VALUE and sort(out=None) == INVALID_VALUE
    assert moments(xp=None) == INVALID_VALUE and moments(mean=None) == INVALID_VALUE and moments(out=None) == INVALID_VALUE
    for fn in (quantiles, interval, mcse_q):
        assert fn(src=None) == INVALID_VALUE and fn(out=None) == INVALID_VALUE
        for bad_p in (0.0, 1.0, -0.5, 1.5, math.nan):
            assert fn(p=bad_p) == INVALID_VALUE, (fn.__name__, bad_p)
    assert interval(p=0.01) == INVALID_VALUE and mcse_q(e=None) == INVALID_VALUE          # a window of no step
    assert lib.sgmcmc_summary_mcse(r[1], r[2], r[3], None, r[10], Q, r[10], r[11], stream) == INVALID_VALUE
    assert lib.sgmcmc_summary_mcse(r[1], r[2], r[3], ess.data_ptr(), r[10], 0, r[10], r[11], stream) == INVALID_VALUE
    torch.cuda.synchronize()
    assert all((t == sentinel).all() for t in (ordered, csq, rows)) and (ranks == -7).all()
    # ... and the accepted call is the Python layer's
    assert sort() == 0 and moments() == 0 and quantiles() == 0 and interval() == 0 and mcse_q() == 0
    torch.cuda.synchronize()
    want = D.posterior_summary(x[:2, :16].contiguous(), (0.3,), 0.9, True, parts=True)
    assert _all_same_bits((rows[0], rows[1], rows[2], rows[3], rows[4], rows[5], rows[6]),
                          (want.mean, want.sd, want.m2, want.m4, want.quantiles[0], want.hdi_lower, want.hdi_upper))
    a, b, lo, hi, _ = beta_ranks(np.full(Q, 20.0), 0.3, N)
    np.testing.assert_allclose(_np(rows[8]), a, rtol=AB_RTOL)
    np.testing.assert_allclose(_np(rows[9]), b, rtol=AB_RTOL)
    np.testing.assert_array_equal(_np(ranks), np.stack([lo, hi]))
    np.testing.assert_array_equal(_np(rows[7]), (_np(ordered)[hi, np.arange(Q)] - _np(ordered)[lo, np.arange(Q)]) / 2)


@pytest.mark.gpu
def test_weight_space_and_function_space_summaries():
    M, S = 3, 12
    g = torch.Generator().manual_seed(0)
    shapes = {"net.0.weight": (7, 5), "net.0.bias": (7,), "scale": ()}
    chains = []
    for m in range(M):
        d = {k: torch.randn((S,) + s, generator=g).to("cuda:0") for k, s in shapes.items()}
        d["net.1.running_mean"] = torch.randn((S, 7), generator=g, dtype=torch.float64).to("cuda:0")
        d["net.1.num_batches_tracked"] = torch.full((S,), 3, device="cuda:0")
        d["steps"] = torch.arange(S, device="cuda:0") * 10
        chains.append(d)
    names = set(shapes) | {"net.1.running_mean"}
    gathered = {k: torch.cat([c[k] for c in chains]) for k in chains[0]}
    both = (D.weight_space_summary(chains), D.weight_space_summary(gathered, chains=M))
    for k in names:
        stacked = torch.stack([c[k] for c in chains])
        want = D.posterior_summary(stacked)
        assert want.mean.shape == tuple(chains[0][k].shape[1:]) and want.quantiles.shape[0] == 3
        for got in both:                                                # the same skips as weight_space
            assert set(got) == names == set(D.weight_space(chains)) and type(got[k]) is D.PosteriorSummary
            assert _all_same_bits(got[k], want), k
    other = D.weight_space_summary(chains, split=False, probs=(0.5,), hdi_prob=0.8, parts=True)
    stacked = torch.stack([c["scale"] for c in chains])
    assert type(other["scale"]) is D.PosteriorSummaryParts
    assert _all_same_bits(other["scale"], D.posterior_summary(stacked, (0.5,), 0.8, False, parts=True))

    g = torch.Generator().manual_seed(1)
    tables = [torch.log_softmax(torch.randn((10, 9, 4), generator=g, dtype=torch.float64), -1).to("cuda:0")
              for _ in range(3)]
    probs = torch.stack(tables).exp()
    got = D.function_space_summary(tables)
    assert type(got) is D.PosteriorSummary and got.mean.shape == (9, 4) and got.quantiles.shape == (3, 9, 4)
    assert _all_same_bits(got, D.posterior_summary(probs))
    # the mean is the ensemble's predictive probability (the unsplit sequences hold every draw)
    full = D.function_space_summary(tables, split=False)
    torch.testing.assert_close(full.mean, probs.mean(dim=(0, 1)), rtol=1e-13, atol=0)
    torch.testing.assert_close(full.mean.sum(-1), torch.ones(9, dtype=torch.float64, device="cuda:0"), rtol=1e-13, atol=0)
    assert (full.mcse_mean > 0).all() and (full.hdi_lower <= full.quantiles[1]).all()
