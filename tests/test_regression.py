"""Regression predictive scores on the device (bnn_priors_amd/regression.py, csrc/regress_hip.inc; definitions in
include/sgmcmc_hip.h, restated in tests/regression_reference.py).

On the CPU the restatement is held to independent code (adaptive quadrature of the CRPS integral, mpmath at 40 digits,
the one-Gaussian closed form, scipy.stats one-liners, brentq, ks_1samp, searchsorted) and the wrappers to their argument
checks.  On the GPU the kernels are held to the restatement.

Tolerances.  They are measured, not guessed: the restatement is evaluated on the GPU tests' own inputs (CASES) in
np.float64 and in np.longdouble (80-bit, eps 1.1e-19), the largest deviation per quantity is recorded, and the GPU
tolerance is 4 x that (the factor allows for a device erf / erfc / exp an ulp from libm's and another summation order).

  crps      relative to its first term (1/E) sum_i A(y - mu_i, sigma_i):   measured 6.72e-16 (CRPS_DEVIATION = 6.8e-16)
  lpd       absolute (the y of the "tail" regime has z^2 / 2 = 32):        measured 1.21e-14 (LPD_DEVIATION = 1.3e-14)
  pit       absolute; also the CDF deviation of the quantile criterion:    measured 3.32e-16 (PIT_DEVIATION = 3.4e-16)
  moments   mean (relative to mean_e |mu_e|), var_aleatoric and
            var_epistemic (relative to themselves):                        measured 8.06e-16 (MOMENT_DEVIATION = 8.1e-16)

``test_the_recorded_deviations_are_the_measured_ones`` re-measures them.  A quantile q is not compared with a root: it
passes if the 80-bit |F(q) - p| <= 4 PIT_DEVIATION + 2 ulp(q) f(q) (f the mixture's density: adjacent doubles differ by
ulp(q) f(q) in F) and q lies in the hull of the components' own quantiles.  Counts are integers and must be exact;
sq_err and var are one fp64 operation on other outputs and must be those bits.  The Kolmogorov-Smirnov distance is a
maximum of correctly rounded quotients minus inputs, the same operations on both sides: 2^-52 covers it; the
calibration error is a sum of J terms below 1 in another order: J 2^-53.
"""
import functools
import math

import numpy as np
import pytest
import torch

from bnn_priors_amd import evaluation as ev
from bnn_priors_amd import regression as reg
from regression_reference import (LAYOUTS, REGIMES, abs_moment, broadcast, cdf_reference, density_reference, erf,
                                  hull_reference, mixture_reference, normal_cdf, pit_reference, quantile_reference,
                                  random_case)

CRPS_DEVIATION = 6.8e-16
LPD_DEVIATION = 1.3e-14
PIT_DEVIATION = 3.4e-16
MOMENT_DEVIATION = 8.1e-16
CRPS_TOL, LPD_TOL, PIT_TOL, MOMENT_TOL = (4 * d for d in (CRPS_DEVIATION, LPD_DEVIATION, PIT_DEVIATION, MOMENT_DEVIATION))

TILE = reg.TILE
# a pruned product.  E: the 16 slices and their tails, the tile and its neighbours (tile + 1: the first split triangle,
# one chunk holding two tile pairs with different I), 300 (three chunks of two pairs) and 900 (18 partials per entry:
# more than the 16 slices that add them); the two large shapes meet the sizes up to the tile (+ 1 for the odd one)
SAMPLES = (1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 300, 900)
SHAPES = ((1, 1), (2, 3), (257, 1), (50, 2))


def _kept(E, N, D):
    if E > TILE + 1:
        return N * D <= 6
    return E <= 65 or E == TILE + 1 or (N, D) != (257, 1)


CASES = tuple((E, N, D, LAYOUTS[(i + j) % 3], REGIMES[(i + 2 * j + (i // 4)) % 4])
              for i, E in enumerate(SAMPLES) for j, (N, D) in enumerate(SHAPES) if _kept(E, N, D))
QUANTILE_PROBS = (0.001, 0.025, 0.25, 0.5, 0.95, 0.999)
QUANTILE_CASES = tuple(c for c in CASES if c[0] <= TILE + 1)[::2]
FIELDS = ("mean", "var_aleatoric", "var_epistemic", "var", "sq_err", "lpd", "pit", "crps")


@functools.lru_cache(maxsize=None)
def _case(E, N, D, layout, regime):
    "the inputs of a case and the restatement's fp64 and 80-bit answers: computed once, read-only"
    rng = np.random.default_rng(100000 * E + 100 * N + 10 * D + LAYOUTS.index(layout))
    mean, scale, y = random_case(rng, E, N, D, layout, regime)
    want = mixture_reference(mean, scale, y)
    wide = mixture_reference(mean, scale, y, np.longdouble)
    for a in (mean, scale, y, *want.values(), *wide.values()):
        a.setflags(write=False)
    return mean, scale, y, want, wide


def _deviations(got, wide, mean):
    "the deviation of each quantity from the 80-bit restatement, in the measure its tolerance is stated in"
    ld = np.longdouble

    def worst(x):
        return float(np.max(x))
    spread = np.abs(np.asarray(mean, ld)).sum(0) / mean.shape[0]
    moments = [np.abs(got["mean"] - wide["mean"]) / spread]
    for k in ("var_aleatoric", "var_epistemic"):
        moments.append(np.where(wide[k] == 0, np.abs(got[k] - wide[k]), np.abs(got[k] - wide[k]) / np.where(wide[k] == 0, 1, wide[k])))
    return {"crps": worst(np.abs(got["crps"] - wide["crps"]) / wide["crps_first"]),
            "lpd": worst(np.abs(got["lpd"] - wide["lpd"])), "pit": worst(np.abs(got["pit"] - wide["pit"])),
            "moments": max(worst(m) for m in moments)}


# ---- CPU: the restatement against independent code --------------------------------------------------------------------

def test_the_80_bit_error_function_matches_mpmath():
    import mpmath
    rng = np.random.default_rng(0)
    x = np.r_[rng.uniform(-7.5, 7.5, 300), 0.0, 1 / 16, -1 / 16, 7.0, 7.0625, 9.0, -30.0, 0.5 ** 40].astype(np.longdouble)
    got = erf(x, np.longdouble)
    with mpmath.workdps(40):
        want = np.array([np.longdouble(mpmath.nstr(mpmath.erf(mpmath.mpf(float(v))), 30)) for v in x])
    assert float(np.abs(got - want).max()) <= 3e-19
    assert float(np.abs(erf(x.astype(np.float64)) - want).max()) <= 2.3e-16


def _integrand_crps(mu, sg, y):
    from scipy.integrate import quad
    from scipy.stats import norm

    def f(x):
        return (norm.cdf((x - mu) / sg).mean() - (x >= y)) ** 2
    pts = np.sort(np.r_[mu, y])
    lo, hi = pts[0] - 12 * sg.max(), pts[-1] + 12 * sg.max()
    knots = np.r_[lo, pts, hi]
    return sum(quad(f, a, b, epsabs=1e-13, epsrel=1e-12, limit=200)[0] for a, b in zip(knots[:-1], knots[1:]) if b > a)


def test_restatement_crps_is_the_integral_of_the_squared_cdf_gap():
    rng = np.random.default_rng(1)
    for E, spread, sigma in ((1, 1.0, 0.5), (2, 1.0, 0.3), (5, 2.0, 0.5), (17, 1.0, 1.0), (40, 0.2, 1.5)):
        mean = spread * rng.normal(size=(E, 3, 1))
        scale = sigma * rng.uniform(0.5, 1.5, (E, 3, 1))
        y = rng.normal(size=(3, 1)) * spread
        got = mixture_reference(mean, scale, y)["crps"]
        for n in range(3):
            want = _integrand_crps(mean[:, n, 0], scale[:, n, 0], y[n, 0])
            assert abs(got[n, 0] - want) <= 1e-10 * max(1.0, want), (E, n, got[n, 0], want)


def test_restatement_crps_matches_mpmath_at_40_digits():
    import mpmath
    rng = np.random.default_rng(2)
    for E, regime in ((3, "tight"), (9, "outlier"), (33, "wide"), (12, "tail")):
        mean, scale, y = random_case(rng, E, 2, 1, "END", regime)
        got64 = mixture_reference(mean, scale, y)
        got80 = mixture_reference(mean, scale, y, np.longdouble)
        with mpmath.workdps(40):
            def A(m, s):
                return m * mpmath.erf(m / (s * mpmath.sqrt(2))) + 2 * s * mpmath.npdf(m / s)
            for n in range(2):
                mu = [mpmath.mpf(float(v)) for v in mean[:, n, 0]]
                sg = [mpmath.mpf(float(v)) for v in scale[:, n, 0]]
                yy = mpmath.mpf(float(y[n, 0]))
                first = sum(A(yy - m, s) for m, s in zip(mu, sg)) / E
                pairs = sum(A(mu[i] - mu[j], mpmath.sqrt(sg[i] ** 2 + sg[j] ** 2)) for i in range(E) for j in range(i + 1, E))
                crps = first - (pairs + sum(sg) / mpmath.sqrt(mpmath.pi)) / E ** 2
                assert abs(mpmath.mpf(float(got64["crps"][n, 0])) - crps) <= 4e-15 * first, (E, regime)
                hi = float(got80["crps"][n, 0])                        # the 80-bit value as two doubles, exactly
                wide = mpmath.mpf(hi) + mpmath.mpf(float(got80["crps"][n, 0] - np.longdouble(hi)))
                assert abs(wide - crps) <= 2e-18 * first, (E, regime)


def test_restatement_one_gaussian_has_the_closed_form():
    from scipy.stats import norm
    rng = np.random.default_rng(3)
    mean, scale, y = rng.normal(size=(1, 40, 2)), rng.uniform(0.1, 2.0, (1, 40, 2)), rng.normal(size=(40, 2))
    got = mixture_reference(mean, scale, y)
    z = (y - mean[0]) / scale[0]
    want = scale[0] * (z * (2 * norm.cdf(z) - 1) + 2 * norm.pdf(z) - 1 / math.sqrt(math.pi))
    np.testing.assert_allclose(got["crps"], want, rtol=0, atol=1e-15)
    assert (got["var_epistemic"] == 0).all() and np.array_equal(got["var"], scale[0] ** 2)


def test_restatement_pit_and_density_match_scipy():
    from scipy.special import logsumexp
    from scipy.stats import norm
    rng = np.random.default_rng(4)
    for regime in REGIMES:
        mean, scale, y = random_case(rng, 7, 30, 2, "ED", regime)
        mu, sg = broadcast(mean, scale)
        got = mixture_reference(mean, scale, y)
        np.testing.assert_allclose(got["pit"], norm.cdf(y, mu, sg).mean(0), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(got["lpd"], logsumexp(norm.logpdf(y, mu, sg), axis=0) - math.log(7), rtol=0, atol=1e-13)
        np.testing.assert_allclose(got["mean"], mu.mean(0), rtol=0, atol=1e-15)
        np.testing.assert_allclose(got["var_epistemic"], mu.var(0), rtol=1e-13)
        np.testing.assert_allclose(got["var_aleatoric"], (sg ** 2).mean(0), rtol=1e-14)
        np.testing.assert_allclose(cdf_reference(y, mean, scale), got["pit"], rtol=1e-14, atol=1e-300)
        np.testing.assert_allclose(density_reference(y, mean, scale), np.exp(got["lpd"]), rtol=1e-12)
    z = np.array([-8.5, -3.0, 0.0, 3.0, 8.5])
    # (the argument z / sqrt 2 is rounded once: a relative 2^-53 there is a relative z^2 2^-53 in a tail's value)
    assert (np.abs(normal_cdf(z) - norm.cdf(z)) <= 2.3e-16 * (2 + z * z) * norm.cdf(z)).all()


def test_restatement_quantiles_match_brentq():
    from scipy.optimize import brentq
    rng = np.random.default_rng(5)
    probs = np.array(QUANTILE_PROBS)
    z = reg.normal_quantile(probs).numpy()
    from scipy.special import ndtri
    assert np.abs(z - ndtri(probs)).max() <= 4e-16 * np.abs(z).max()
    for regime in REGIMES:
        mean, scale, _ = random_case(rng, 7, 3, 2, "END", regime)        # (7: no level is a k / E, where F has a plateau)
        got = quantile_reference(mean, scale, probs, z)
        lo, hi = hull_reference(mean, scale, z)
        assert ((lo <= got) & (got <= hi)).all()
        for qi, p in enumerate(probs):
            for n in range(3):
                for d in range(2):
                    f = functools.partial(lambda x, n, d: cdf_reference(np.full((3, 2), x), mean, scale)[n, d] - p, n=n, d=d)
                    want = brentq(f, lo[qi, n, d] - 1e-9, hi[qi, n, d] + 1e-9, xtol=1e-15, rtol=1e-15)
                    assert abs(got[qi, n, d] - want) <= 1e-12 * max(1.0, abs(want)) + 4e-16 / density_reference(
                        np.full((3, 2), want), mean, scale)[n, d], (regime, p)


def test_restatement_pit_calibration_matches_scipy_and_searchsorted():
    from scipy.stats import ks_1samp, uniform
    rng = np.random.default_rng(6)
    levels, central = np.array(reg.DEFAULT_LEVELS), np.array([0.5, 0.9, 0.95])
    for n, kind in ((1, "u"), (2, "u"), (50, "u"), (257, "beta"), (1000, "ties")):
        u = rng.random(n) if kind == "u" else rng.beta(2.0, 0.7, n) if kind == "beta" else rng.integers(0, 21, n) / 20
        got = pit_reference(u, levels, central)
        assert abs(got["ks"] - ks_1samp(u, uniform.cdf).statistic) <= 1e-15
        s = np.sort(u)
        assert np.array_equal(got["counts"], np.searchsorted(s, levels, side="right"))
        assert np.array_equal(got["cover"], np.searchsorted(s, (1 + central) / 2, side="right")
                              - np.searchsorted(s, (1 - central) / 2, side="left"))
        assert abs(got["calibration_error"] - np.mean((got["counts"] / n - levels) ** 2)) <= 1e-16


def test_the_recorded_deviations_are_the_measured_ones():
    "fp64 against 80-bit on the GPU tests' own inputs: the recorded figure bounds it and is not padded beyond 2 x"
    assert np.finfo(np.longdouble).eps < 2e-19
    worst = {"crps": 0.0, "lpd": 0.0, "pit": 0.0, "moments": 0.0}
    for case in CASES:
        mean, _, _, want, wide = _case(*case)
        for k, v in _deviations(want, wide, mean).items():
            worst[k] = max(worst[k], v)
    print("largest fp64 - longdouble deviations", worst)
    for k, recorded in (("crps", CRPS_DEVIATION), ("lpd", LPD_DEVIATION), ("pit", PIT_DEVIATION), ("moments", MOMENT_DEVIATION)):
        assert recorded / 2 <= worst[k] <= recorded, (k, worst[k], recorded)


def test_the_split_restated_in_python_is_the_library_s():
    from bnn_priors_amd import _hip
    lib = _hip.lib()
    for E, N, D in [(c[0], c[1], c[2]) for c in CASES] + [(1000, 50, 1), (1000, 1000, 1), (4096, 1, 1), (reg.MAX_SAMPLES, 3, 1)]:
        assert lib.sgmcmc_gmix_workspace_bytes(E, N, D) == 8 * N * D * reg.pair_split(E, N, D), (E, N, D)
    assert lib.sgmcmc_gmix_workspace_bytes(reg.MAX_SAMPLES + 1, 1, 1) == -1 and lib.sgmcmc_gmix_workspace_bytes(1, 0, 1) == -1
    assert reg.MAX_SAMPLES >= 4096 and reg.pair_split(TILE, 1, 1) == 1 and reg.pair_split(TILE + 1, 1, 1) == 2
    assert reg.pair_split(300, 2, 3) == 3 and reg.pair_split(900, 1, 1) == 18 and reg.pair_split(1000, 1000, 1) == 3


def test_wrappers_reject_bad_arguments_before_any_launch(monkeypatch):
    from bnn_priors_amd import _hip

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_hip, "lib", no_library)
    mean, scale, y = torch.zeros(4, 8, 2), torch.ones(4), torch.zeros(8, 2)
    for bad in (torch.zeros(8, 2), np.zeros((4, 8, 2)), torch.zeros(4, 8, 2, 1)):
        with pytest.raises(ValueError, match="mean must"):
            reg.predictive(bad, scale)
    for bad in (torch.zeros(0, 8, 2), torch.zeros(4, 0, 2), torch.zeros(4, 8, 0)):
        with pytest.raises(ValueError, match="at least one"):
            reg.predictive(bad, scale)
    with pytest.raises(ValueError, match="samples"):
        reg.predictive(torch.zeros(reg.MAX_SAMPLES + 1, 1, 1), torch.ones(1))
    for bad in ([1.0] * 4, torch.ones(3), torch.ones(4, 3), torch.ones(4, 8), torch.ones(4, 7, 2), torch.ones(4, 8, 2, 1),
                torch.ones(2, 4, 8, 2)):
        with pytest.raises(ValueError, match="scale"):
            reg.predictive(mean, bad)
        with pytest.raises(ValueError, match="scale"):
            reg.quantiles(mean, bad, [0.5])
    for bad in (torch.zeros(8), torch.zeros(8, 3), [[0.0] * 2] * 8):
        with pytest.raises(ValueError, match="y must|CUDA"):
            reg.predictive(mean, scale, bad)
    for ok_scale in (torch.ones(4), torch.ones(4, 2), torch.ones(4, 1, 1), torch.ones(4, 8, 2), torch.ones(())):
        with pytest.raises(ValueError, match="CUDA"):
            reg.predictive(mean, ok_scale, y)
    for bad in ([], [0.0], [1.0], [0.5, 1.5], [0.5] * (reg.MAX_QUANTILES + 1), 0.5):
        with pytest.raises(ValueError, match="level"):
            reg.quantiles(mean, scale, bad)
    with pytest.raises(ValueError, match="CUDA"):
        reg.quantiles(mean, scale, [0.5])
    with pytest.raises(ValueError, match=r"\[N\] tensor"):
        reg.pit_calibration(torch.zeros(4, 2))
    with pytest.raises(ValueError, match="rows"):
        reg.pit_calibration(torch.zeros(0))
    with pytest.raises(ValueError, match="rows"):
        reg.pit_calibration(torch.zeros(reg.MAX_ROWS + 1))
    with pytest.raises(ValueError, match="CUDA"):
        reg.pit_calibration(torch.full((4,), 0.5))
    with pytest.raises(ValueError, match="tensors"):
        reg.interval_score([0.0], torch.ones(1), torch.ones(1), 0.9)
    with pytest.raises(ValueError, match="between 0 and 1"):
        reg.interval_score(torch.zeros(1), torch.ones(1), torch.ones(1), 1.0)
    # the Winkler score: the width inside, plus 2 / (1 - c) times the miss outside
    s = reg.interval_score(torch.tensor([0.0, 0.0, 0.0]), torch.tensor([2.0, 2.0, 2.0]), torch.tensor([1.0, -1.0, 2.5]), 0.9)
    torch.testing.assert_close(s, torch.tensor([2.0, 22.0, 12.0]))
    # evaluate_regression: a categorical likelihood, and a model that is not on the device
    from test_evaluation import _setup
    net, loader, samples, _ = _setup("classificationdensenet", n=16, E=2)
    with pytest.raises(ValueError, match="Normal likelihood"):
        ev.regression_tables(net, loader, samples)
    net, loader, samples = _regression_setup("cpu")
    with pytest.raises(ValueError, match="between 0 and 1"):
        ev.evaluate_regression(net, loader, samples, central=(0.5, 1.0))
    with pytest.raises(ValueError, match="CUDA"):
        ev.evaluate_regression(net, loader, samples)


def _regression_setup(device, n=40, E=5):
    from bnn_priors_amd import models
    torch.manual_seed(0)
    net = models.DenseNet(1, 1, 10, noise_std=0.1).to(device).eval()
    x = torch.linspace(-2, 2, n).reshape(n, 1)
    with torch.no_grad():                       # targets the fabricated posterior explains: |z| of a few, as in CASES
        y = net(x.to(device)).mean.cpu() + 0.1 * torch.randn(n, 1)
    g = torch.Generator().manual_seed(1)
    samples = {k: (v.unsqueeze(0) + 0.05 * torch.randn((E,) + tuple(v.shape), generator=g).to(device)).clone()
               for k, v in net.state_dict().items()}
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x.to(device), y.to(device)), batch_size=16)
    return net, loader, samples


def test_regression_tables_on_the_host_hold_each_sample_s_prediction():
    net, loader, samples = _regression_setup("cpu")
    mean, scale, y = ev.regression_tables(net, loader, samples)
    assert mean.shape == scale.shape == (5, 40, 1) and y.shape == (40, 1) and mean.dtype == y.dtype == torch.float64
    assert (scale == torch.tensor(0.1).double()).all() and torch.equal(y, loader.dataset.tensors[1].double())
    for e in (0, 4):
        net.load_state_dict({k: v[e] for k, v in samples.items()})
        with torch.no_grad():
            torch.testing.assert_close(mean[e], net(loader.dataset.tensors[0]).mean.double(), rtol=1e-5, atol=1e-6)


# ---- GPU --------------------------------------------------------------------------------------------------------------

def _dev(a):
    return torch.as_tensor(np.array(a)).cuda()           # (a copy: the shared inputs are read-only)


def _host(g):
    return {k: None if v is None else v.cpu().numpy() for k, v in g._asdict().items()}


def _bits(g):
    return tuple(None if v is None else v.cpu().numpy().tobytes() for v in g)


@pytest.mark.gpu
@pytest.mark.parametrize("E,N,D,layout,regime", CASES)
def test_predictive_matches_the_restatement(E, N, D, layout, regime):
    mean, scale, y, _, wide = _case(E, N, D, layout, regime)
    g = reg.predictive(_dev(mean), _dev(scale), _dev(y))
    got = _host(g)
    assert all(got[k].shape == (N, D) and got[k].dtype == np.float64 for k in FIELDS)
    dev = _deviations(got, wide, mean)
    print((E, N, D, layout, regime), "split", reg.pair_split(E, N, D), "deviations", dev)
    assert dev["crps"] <= CRPS_TOL and dev["lpd"] <= LPD_TOL and dev["pit"] <= PIT_TOL and dev["moments"] <= MOMENT_TOL, dev
    assert np.array_equal(got["var"], got["var_aleatoric"] + got["var_epistemic"])
    assert np.array_equal(got["sq_err"], (y - got["mean"]) ** 2)
    assert (got["crps"] >= -CRPS_TOL * np.asarray(wide["crps_first"], np.float64)).all()
    # ... and without y: the same bits, and no field that needs it
    h = reg.predictive(_dev(mean), _dev(scale))
    assert h.sq_err is None and h.lpd is None and h.pit is None and h.crps is None
    assert _bits(h)[:4] == _bits(g)[:4]
    if layout != "END":                                # the strides are the layout: the expanded table gives the same bits
        full = np.ascontiguousarray(broadcast(mean, scale)[1])
        assert _bits(reg.predictive(_dev(mean), _dev(full), _dev(y))) == _bits(g)


@pytest.mark.gpu
def test_two_calls_give_identical_bits_and_the_rows_may_come_in_any_order():
    rng = np.random.default_rng(11)
    for case in ((TILE + 1, 50, 2, "ED", "tight"), (300, 2, 3, "END", "outlier"), (65, 257, 1, "E", "wide")):
        mean, scale, y = _case(*case)[:3]
        probs = list(QUANTILE_PROBS)
        a, b = (reg.predictive(_dev(mean), _dev(scale), _dev(y)) for _ in range(2))
        qa, qb = (reg.quantiles(_dev(mean), _dev(scale), probs) for _ in range(2))
        assert _bits(a) == _bits(b) and torch.equal(qa, qb)
        p = rng.permutation(case[1])
        sc = scale[:, p] if case[3] == "END" else scale
        c = reg.predictive(_dev(mean[:, p]), _dev(sc), _dev(y[p]))
        for name, u, v in zip(FIELDS, a, c):
            assert u.cpu().numpy()[p].tobytes() == v.cpu().numpy().tobytes(), name
        assert torch.equal(reg.quantiles(_dev(mean[:, p]), _dev(sc), probs), qa[:, torch.as_tensor(p).cuda()])
        table = reg._pit_columns(a.pit, list(reg.DEFAULT_LEVELS), [0.5, 0.9, 0.95])       # every output in one launch
        for d in range(case[2]):
            one, two = reg.pit_calibration(a.pit[:, d]), reg.pit_calibration(c.pit[:, d])
            assert (one.ks, one.calibration_error) == (two.ks, two.calibration_error)
            assert torch.equal(one.freq, two.freq) and torch.equal(one.coverage, two.coverage)
            assert table[d, :2].tolist() == [one.ks, one.calibration_error]
            assert torch.equal(table[d, 3:] / case[1], torch.cat([one.freq, one.coverage]))


@pytest.mark.gpu
@pytest.mark.parametrize("E", (4096, reg.MAX_SAMPLES))
def test_a_collapsed_mixture_is_its_one_gaussian_at_the_largest_sizes(E):
    """E equal components are one Gaussian: every pair term is A(0, sigma sqrt 2) = 2 sigma / sqrt(pi), so the closed
    forms of one Gaussian hold the tiled pair sum (528 and 33,024 tile pairs, 264 and 1,024 partials per entry) to the
    recorded tolerances without a table of all pairs on the host."""
    ld = np.longdouble
    mu, sg, y = np.array([[0.25], [-1.5]]), np.array([[0.75], [2.0]]), np.array([[1.0], [-1.25]])
    assert reg.pair_split(E, 2, 1) == (264 if E == 4096 else 1024)
    g = _host(reg.predictive(_dev(np.broadcast_to(mu, (E, 2, 1))), _dev(np.broadcast_to(sg, (E, 2, 1))), _dev(y)))
    z = (y.astype(ld) - mu) / sg
    pi = 4 * np.arctan(ld(1))
    phi = np.exp(-z * z / 2) / np.sqrt(2 * pi)
    first = np.asarray(abs_moment(y.astype(ld) - mu, sg.astype(ld), ld))
    crps = sg * (z * erf(z / np.sqrt(ld(2)), ld) + 2 * phi - 1 / np.sqrt(pi))
    assert float((np.abs(g["crps"] - crps) / first).max()) <= CRPS_TOL
    assert float(np.abs(g["pit"] - normal_cdf(z, ld)).max()) <= PIT_TOL
    assert float(np.abs(g["lpd"] - (np.log(phi) - np.log(sg.astype(ld)))).max()) <= LPD_TOL
    assert np.array_equal(g["mean"], mu) and (g["var_epistemic"] == 0).all() and np.array_equal(g["var"], sg * sg)
    q = reg.quantiles(_dev(np.broadcast_to(mu, (E, 2, 1))), _dev(np.broadcast_to(sg, (E, 2, 1))), [0.05, 0.5]).cpu().numpy()
    assert np.array_equal(q, mu + sg * reg.normal_quantile([0.05, 0.5]).numpy().reshape(2, 1, 1))


@pytest.mark.gpu
def test_nan_and_a_scale_that_is_not_positive_stay_in_their_own_entry():
    mean, scale, y = _case(TILE + 1, 50, 2, "ED", "tight")[:3]
    full = np.ascontiguousarray(broadcast(mean, scale)[1])
    clean = reg.predictive(_dev(mean), _dev(full), _dev(y))
    clean_q = reg.quantiles(_dev(mean), _dev(full), [0.1, 0.9])
    m, s, yy = mean.copy(), full.copy(), y.copy()
    m[100, 7, 1] = np.nan
    s[3, 20, 0] = 0.0
    s[TILE, 21, 1] = -1.0
    s[5, 22, 0] = np.nan
    yy[30, 1] = np.nan
    hit = np.zeros((50, 2), bool)
    hit[[7, 20, 21, 22, 30], [1, 0, 1, 0, 1]] = True
    g = reg.predictive(_dev(m), _dev(s), _dev(yy))
    for name, a, b in zip(FIELDS, g, clean):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.isnan(a[hit]).all(), name
        assert a[~hit].tobytes() == b[~hit].tobytes(), name           # every other entry keeps its bits
    q = reg.quantiles(_dev(m), _dev(s), [0.1, 0.9]).cpu().numpy()
    hit[30, 1] = False                                                 # (the quantiles do not read y)
    assert np.isnan(q[:, hit]).all() and q[:, ~hit].tobytes() == clean_q.cpu().numpy()[:, ~hit].tobytes()
    with pytest.raises(ValueError, match="NaN"):
        reg.pit_calibration(g.pit[:, 1])


@pytest.mark.gpu
@pytest.mark.parametrize("E,N,D,layout,regime", QUANTILE_CASES)
def test_quantiles_solve_the_80_bit_cdf_inside_the_hull(E, N, D, layout, regime):
    mean, scale = _case(E, N, D, layout, regime)[:2]
    probs = np.array(QUANTILE_PROBS)
    z = reg.normal_quantile(probs).numpy()
    q = reg.quantiles(_dev(mean), _dev(scale), list(probs)).cpu().numpy()
    assert q.shape == (len(probs), N, D)
    lo, hi = hull_reference(mean, scale, z)
    assert ((lo <= q) & (q <= hi)).all()
    if E == 1:
        assert q.tobytes() == lo.tobytes() == (broadcast(mean, scale)[0] + broadcast(mean, scale)[1] * z.reshape(-1, 1, 1, 1))[:, 0].tobytes()
    gap = np.abs(cdf_reference(q, mean, scale, np.longdouble) - probs.reshape(-1, 1, 1).astype(np.longdouble))
    slack = 4 * PIT_DEVIATION + 2 * np.spacing(np.abs(q)) * density_reference(q, mean, scale)
    print((E, N, D, layout, regime), "largest |F(q) - p|", float(gap.max()), "largest share of its bound", float((gap / slack).max()))
    assert (gap <= slack).all(), float((gap / slack).max())


@pytest.mark.gpu
def test_pit_calibration_matches_the_restatement():
    rng = np.random.default_rng(12)
    levels, central = list(reg.DEFAULT_LEVELS), [0.5, 0.9, 0.95]
    for n, kind in ((1, "u"), (2, "u"), (50, "u"), (257, "beta"), (1025, "ties"), (4099, "u")):
        u = rng.random(n) if kind == "u" else rng.beta(2.0, 0.7, n) if kind == "beta" else rng.integers(0, 21, n) / 20
        for lv, ce in ((levels, central), ([0.5], []), (list(np.linspace(0, 1, 1026)[1:-1]), [0.999])):
            got = reg.pit_calibration(_dev(u), lv, ce)
            want = pit_reference(u, lv, ce)
            assert abs(got.ks - want["ks"]) <= 2.0 ** -52
            assert np.array_equal(got.freq.numpy(), want["counts"] / n)                  # integer counts, exact
            assert np.array_equal(got.coverage.numpy(), want["cover"] / n) and got.coverage.shape == (len(ce),)
            assert abs(got.calibration_error - want["calibration_error"]) <= len(lv) * 2.0 ** -53
    exact = reg.pit_calibration(_dev((np.arange(100) + 0.5) / 100), [0.25, 0.5], [0.5])
    assert abs(exact.ks - 0.005) <= 2.0 ** -52 and exact.calibration_error == 0.0 and exact.coverage.tolist() == [0.5]


@pytest.mark.gpu
def test_evaluate_regression_on_a_dense_net():
    net, loader, samples = _regression_setup("cuda:0")
    central = (0.5, 0.9, 0.95)
    got = ev.evaluate_regression(net, loader, samples, central=central)
    names = ["rmse", "lpd", "crps", "pit_ks", "calibration_error", "var_aleatoric", "var_epistemic"] + [
        f"{k}_{c}" for c in ("0.5", "0.9", "0.95") for k in ("coverage", "width", "interval_score")]
    assert list(got) == names and all(type(v) is float for v in got.values())
    mean, scale, y = ev.regression_tables(net, loader, samples)
    assert mean.shape == scale.shape == (5, 40, 1) and y.shape == (40, 1) and mean.dtype == torch.float64 and mean.is_cuda
    last = {k: v[-1] for k, v in samples.items()}
    assert all(torch.equal(v, last[k]) for k, v in net.state_dict().items())      # the model holds the last sample
    m, s, yy = mean.cpu().numpy(), scale.cpu().numpy(), y.cpu().numpy()
    wide = mixture_reference(m, s, yy, np.longdouble)
    assert float(np.abs(wide["lpd"]).max()) <= 33         # the range LPD_DEVIATION was measured on (z^2 / 2 = 32)
    avg = 40 * 2.0 ** -53                  # the mean of 40 entries, added in whatever order: relative to their mean size
    first = float(wide["crps_first"].mean())
    assert abs(got["crps"] - float(wide["crps"].mean())) <= CRPS_TOL * first + avg * float(wide["crps"].mean())
    assert abs(got["lpd"] - float(wide["lpd"].mean())) <= LPD_TOL + avg * float(np.abs(wide["lpd"]).mean())
    host = torch.distributions.Normal(mean, scale).log_prob(y).logsumexp(0) - math.log(5)
    assert abs(got["lpd"] - host.mean().item()) <= LPD_TOL + avg * float(np.abs(wide["lpd"]).mean())
    # the mean's deviation, at most MOMENT_TOL mean_e |mu_e|, moves a squared error by 2 |y - mean| times itself
    msq = float(wide["sq_err"].mean())
    slack = 2 * float(np.sqrt(wide["sq_err"]).mean()) * MOMENT_TOL * np.abs(m).mean(0).max() + (avg + 4e-16) * msq
    assert abs(got["rmse"] - math.sqrt(msq)) <= slack / (2 * got["rmse"]) + 2.3e-16 * got["rmse"]
    for k in ("var_aleatoric", "var_epistemic"):
        assert abs(got[k] - float(wide[k].mean())) <= (MOMENT_TOL + avg) * float(wide[k].mean()), k
    pit = reg.predictive(mean, scale, y).pit
    assert float(np.abs(pit.cpu().numpy() - wide["pit"]).max()) <= PIT_TOL
    cal = pit_reference(pit[:, 0].cpu().numpy(), reg.DEFAULT_LEVELS, central)
    assert abs(got["pit_ks"] - cal["ks"]) <= 2.0 ** -52 and abs(got["calibration_error"] - cal["calibration_error"]) <= 19 * 2.0 ** -53
    probs = [(1 - c) / 2 for c in central] + [(1 + c) / 2 for c in central]
    q = reg.quantiles(mean, scale, probs).cpu().numpy()
    gap = np.abs(cdf_reference(q, m, s, np.longdouble) - np.asarray(probs, np.longdouble).reshape(-1, 1, 1))
    assert (gap <= 4 * PIT_DEVIATION + 2 * np.spacing(np.abs(q)) * density_reference(q, m, s)).all()
    for i, c in enumerate(("0.5", "0.9", "0.95")):
        lo, hi = q[i], q[3 + i]
        assert got[f"coverage_{c}"] == ((lo <= yy) & (yy <= hi)).mean()
        assert abs(got[f"width_{c}"] - (hi - lo).mean()) <= avg * (hi - lo).mean()
        score = (hi - lo) + 2 / (1 - float(c)) * (np.maximum(lo - yy, 0) + np.maximum(yy - hi, 0))
        assert abs(got[f"interval_score_{c}"] - score.mean()) <= (avg + 4 * 2.0 ** -53) * score.mean()
