"""Sampler temperature diagnostics on the device (bnn_priors_amd/temperature.py, csrc/temper_hip.inc; definitions in
include/sgmcmc_hip.h, restated in tests/temperature_reference.py with mpmath at 50 digits; the reference's own outputs in
tests/golden/temperature.npz, written by tests/golden/make_temperature_goldens.py).

Tolerances.  None is free:

  log-tail   |lt - lt_exact| <= TOL max(1, |lt_exact|), TOL = 32 eps: the bound tests/test_goodness_of_fit.py holds the same
             quantity to.  The points are r = 1 + s / sqrt(a) formed in double and taken as the exact numbers they are
             (x = a r exactly), s in {-8, -6, -1, 0, 1, 6, 8}, at the sizes of the issue, at the kernel's switch in a
             (a = 100: d = 199, 200, 201) and at its switch in u = r - 1 (the doubles on both sides of +-0.3).
             Device, measured on an MI355X: MEASURED_LOG_TAIL below, printed by test_log_tails_on_the_grid.
  quantile   the 50-digit log-tail at the device's bound r is within 2 TOL max(1, |log p|) of log p plus the effect of
             the one rounding of r, eps |x dlog F / dx| computed in mpmath.  Against the golden _gamma_confidence values:
             scipy's own measured distance from the 50-digit quantile on that grid (SCIPY_PPF_DISTANCE, re-measured by
             test_scipy_quantile_distance_is_the_recorded_one) plus the same allowance, expressed in r.
             Device, measured: MEASURED_QUANTILE below (the share of the allowance that is used).
  coverage   exact: integer counts.  Every est / temperature of the golden table is at least 1e-9 (relative) away from
             every 50-digit interval end (asserted), so no rounding of an end decides a count.
  mean, se, EWMA   tests/test_raob.py's rule: four times the float64 restatement's own distance from the same expression
             in longdouble plus 4 ulp of the largest magnitude (max-norms).  alpha = 0 is bitwise.

MEASURED_LOG_TAIL = 4.18 eps at d = 3, r = 1 + 1 / sqrt(1.5) (series, the band a <= x < a + 1); the same arithmetic in fp64
                    on the host: 4.7 eps there, 1.6 eps at most where the uniform expansion is used (d >= 200)
MEASURED_QUANTILE = 0.441 of the allowance at most (d = 1e7, c = 0.05, upper end); the log-tail distance itself reaches
                    9425 eps at d = 2^31 - 1, where one rounding of r moves the log-tail by up to 1.2e5 eps
"""
import functools
import math
import os

import mpmath as mp
import numpy as np
import pytest
import scipy.stats
import torch

import temperature_reference as ref
from bnn_priors_amd import _hip
from bnn_priors_amd import temperature as tp

EPS = ref.EPS
TOL = 32 * EPS
SCIPY_PPF_DISTANCE = 9.7 * EPS            # measured with scipy 1.15.3: 9.61 eps (d = 1, c = 0.999)
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temperature.npz")
SIZES = (1, 2, 3, 7, 100, 199, 200, 201, 19999, 20000, 20002, 36864, 78400, 10 ** 6, 10 ** 7, 2 ** 31 - 1)
SIGMAS = (-8, -6, -1, 0, 1, 6, 8)
SWITCH_SIZES = (200, 20000, 10 ** 7)     # ... where r - 1 crosses +-SGMCMC_TEMPER_UNIFORM_U
CONFIDENCES6 = (.05, .25, .5, .75, .95, .999)
SWITCH_QUANTILE_SIZES = (199, 200, 201)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def _grid():
    "[n, K] doubles r (NaN where the point is not positive) for SIZES, then the switch points for SWITCH_SIZES"
    rows = [[1.0 + s / math.sqrt(d / 2.0) for d in SIZES] for s in SIGMAS]
    grid = np.array(rows, dtype=np.float64)
    grid[~(grid > 0)] = np.nan
    u = _hip.TEMPER_UNIFORM_U
    edges = [1.0 + v for e in (u, -u) for v in (np.nextafter(e, 0.0), e, np.nextafter(e, 2 * e))]
    switch = np.array([[e] * len(SWITCH_SIZES) for e in edges], dtype=np.float64)
    return grid, switch


@functools.lru_cache(maxsize=None)
def _grid_reference():
    "the 50-digit (log P, log Q) at every point of _grid(): computed once per process"
    out = []
    for table, sizes in zip(_grid(), (SIZES, SWITCH_SIZES)):
        exact = np.empty(table.shape + (2,), dtype=object)
        for i in range(table.shape[0]):
            for k, d in enumerate(sizes):
                exact[i, k] = (None, None) if table[i, k] != table[i, k] else ref.log_tails(d, table[i, k])
        out.append(exact)
    return out


@functools.lru_cache(maxsize=None)
def _golden_margin():
    "the smallest relative distance of an est / temperature of the golden table from a 50-digit interval end"
    g = golden()
    with np.errstate(all="ignore"):
        ratio = g["est"] / g["temperature"][:, None]
    worst = math.inf
    for k, d in enumerate(g["sizes"]):
        for c in g["confidences"]:
            for end in ref.interval(int(d), c):
                col = ratio[np.isfinite(ratio[:, k]), k]
                worst = min(worst, float(np.min(np.abs(col - float(end)) / float(end))))
    return worst


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_arguments_are_checked_on_the_host():
    assert "temperature_report" in tp.__all__ and "chi2_interval" in tp.__all__
    x = torch.ones(4, 3, dtype=torch.float64)
    for call in (lambda: tp.ewma(x, 0.5), lambda: tp.weighted_temperature(x, (1, 2, 3)),
                 lambda: tp.chi2_tails(x, (1, 2, 3)), lambda: tp.chi2_interval((1, 2), device="cpu"),
                 lambda: tp.kinetic_coverage(x, 1.0, (1, 2, 3), bounds=torch.ones(3, 5, 2, dtype=torch.float64))):
        with pytest.raises(ValueError, match="CUDA|no CPU"):
            call()
    for bad in ((), (0,), (2 ** 31,), (1.5,), (True,)):
        with pytest.raises(ValueError):
            tp._sizes(bad)
    assert tp._sizes({"a": 3, "b": 2 ** 31 - 1}) == [3, 2 ** 31 - 1]
    for bad in ((), (0.0,), (1.0,), (0.5, float("nan")), tuple([0.5] * (tp.MAX_LEVELS + 1))):
        with pytest.raises(ValueError):
            tp._confidences(bad)
    for alpha in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            tp.ewma(x, alpha)
    with pytest.raises(ValueError, match="temperature"):
        tp.temperature_report({"steps": np.arange(3)}, {"a": 1})
    with pytest.raises(ValueError, match="no size"):
        tp.temperature_report({"steps": np.arange(3), "temperature": np.ones(3), "est_temperature/a": np.ones(3)}, {"b": 1},
                              device="cuda")
    model = torch.nn.Linear(3, 2)
    assert tp.get_sizes(model) == {"weight": 6, "bias": 2}


def test_abi_carries_the_temperature_entry_points():
    names = ("sgmcmc_temper_tails", "sgmcmc_temper_quantile", "sgmcmc_temper_steps", "sgmcmc_temper_ewma")
    assert all(n in _hip.EXPORTS for n in names) and _hip.ABI_VERSION >= 24
    lib = _hip.lib()
    assert all(hasattr(lib, n) for n in names)


def test_the_golden_is_consistent_with_itself_and_the_restatement():
    g = golden()
    est, temp, K = g["est"], g["temperature"], len(g["sizes"])
    with np.errstate(all="ignore"):
        ratio = est / temp[:, None]
    inside = (g["lower"].T[:, None, :] <= ratio[None]) & (ratio[None] <= g["upper"].T[:, None, :])      # [C, S, K]
    share = inside.sum(-1) / K
    assert (share == g["coverage_a0"]).all()
    assert (share[:, 11] == 0).all() and (share[:, 23] == 0).all()          # the NaN row, the zero-temperature row
    assert (share[:, 3:30:2] == g["coverage_masked"]).all()
    smooth = ref.ewma(share, 0.7)
    assert np.max(np.abs(smooth - g["coverage_a07"])) <= ref.bound(smooth, ref.ewma(share, 0.7, np.longdouble))
    w = g["sizes"].astype(float)
    for tag, table in (("kinetic", est), ("config", g["config"])):
        m64, s64 = ref.weighted_var_se(w, table)
        ml, sl = ref.weighted_var_se(w, table, np.longdouble)
        ok = np.isfinite(m64)
        assert (ok == np.isfinite(g[tag + "_mean"])).all() and ok.sum() >= len(ok) - 1
        assert np.max(np.abs(g[tag + "_mean"][ok] - m64[ok])) <= ref.bound(m64, ml)
        assert np.max(np.abs(g[tag + "_se"][ok] - s64[ok])) <= ref.bound(s64, sl)
    for tag, alpha in (("a0", 0.0), ("a05", 0.5), ("a0999", 0.999)):
        y64, yl = ref.ewma(g["ewma_input"], alpha), ref.ewma(g["ewma_input"], alpha, np.longdouble)
        assert np.max(np.abs(g["ewma_" + tag] - y64)) <= ref.bound(y64, yl)
    assert _golden_margin() >= 1e-9


def test_reference_tails_against_scipy_where_scipy_is_sound():
    """scipy's chi2.logcdf / logsf is good to a few eps for d <= 78400 within 8 standard deviations (and 1.1e5 eps off at
    d = 1e6: not asked here).  1e-13 max(1, |lt|) is the accuracy class of scipy's incomplete gamma function; measured with
    scipy 1.15.3: 77.4 eps = 1.7e-14."""
    grid, _ = _grid()
    exact, _ = _grid_reference()
    worst = 0.0
    for k, d in enumerate(SIZES):
        if d > 78400:
            continue
        for i in range(grid.shape[0]):
            r = grid[i, k]
            if r != r:
                continue
            lp, lq = exact[i, k]
            dist = scipy.stats.chi2(df=d, scale=1.0 / d)
            for mine, theirs in ((lp, dist.logcdf(r)), (lq, dist.logsf(r))):
                worst = max(worst, float(abs(mine - theirs) / max(1, abs(mine))))
    print(f"reference vs scipy: {worst / EPS:.2f} eps")
    assert worst <= 1e-13


def test_reference_methods_agree():
    "gammainc, the quadrature near the bulk and the 50-digit expansions beyond it: 1e-30 of each other where all exist"
    worst = mp.mpf(0)
    for d in (200, 20000, 10 ** 6):
        a = mp.mpf(d) / 2
        for s in (-30, -10.5, -10, -8, -1, 0, 1, 8, 10, 10.5, 30):
            x = a * mp.mpf(1.0 + s / math.sqrt(d / 2.0))
            if not x > 0:
                continue
            try:
                exact = (mp.gammainc(a, 0, x, regularized=True), mp.gammainc(a, x, mp.inf, regularized=True))
            except mp.libmp.NoConvergence:
                continue
            other = ref._by_quadrature(a, x) if abs(s) <= 10 else ref._by_expansion(a, x)
            side = 0 if s < 0 else 1                      # the tail that is integrated or expanded
            worst = max(worst, abs(mp.log(exact[side]) - mp.log(other[side])) / max(1, abs(mp.log(exact[side]))))
    assert worst <= mp.mpf(10) ** -30


def test_scipy_quantile_distance_is_the_recorded_one():
    g = golden()
    worst, at = 0.0, None
    for i, d in enumerate(g["grid_sizes"]):
        for j, c in enumerate(g["grid_confidences"]):
            lo = ref.quantile(int(d), (1.0 - c) / 2.0, False, g["grid_lower"][i, j])
            hi = ref.quantile(int(d), 1.0 - (1.0 + c) / 2.0, True, g["grid_upper"][i, j])
            e = float(max(abs(g["grid_lower"][i, j] - lo) / lo, abs(g["grid_upper"][i, j] - hi) / hi))
            if e > worst:
                worst, at = e, (int(d), float(c))
    print(f"scipy chi2.ppf vs the 50-digit quantile: {worst / EPS:.2f} eps at {at}")
    assert 0 < worst <= SCIPY_PPF_DISTANCE


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_log_tails_on_the_grid():
    worst, at = 0.0, None
    for table, exact, sizes in zip(_grid(), _grid_reference(), (SIZES, SWITCH_SIZES)):
        r = torch.from_numpy(table).to(DEV)
        lower, upper = (v.cpu().numpy() for v in tp.chi2_tails(r, sizes, log=True))
        p, q = (v.cpu().numpy() for v in tp.chi2_tails(r, sizes, log=False))
        for i in range(table.shape[0]):
            for k, d in enumerate(sizes):
                if table[i, k] != table[i, k]:
                    assert all(v[i, k] != v[i, k] for v in (lower, upper, p, q))
                    continue
                for got, plain, want in ((lower[i, k], p[i, k], exact[i, k][0]), (upper[i, k], q[i, k], exact[i, k][1])):
                    scale = max(1.0, float(abs(want)))
                    dist = float(abs(mp.mpf(float(got)) - want)) / scale
                    if dist > worst:
                        worst, at = dist, (d, float(table[i, k]))
                    assert dist <= TOL, (d, table[i, k], got, float(want), dist / EPS)
                    t = mp.exp(want)
                    if t > 1e-300:
                        assert abs(mp.mpf(float(plain)) - t) <= (TOL * scale + EPS) * t, (d, table[i, k], plain, float(t))
                assert p[i, k] + q[i, k] == pytest.approx(1.0, abs=2 * EPS)
    print(f"worst log-tail distance: {worst / EPS:.2f} eps at (d, r) = {at}")


@pytest.mark.gpu
def test_tails_at_the_edges_of_the_domain():
    r = torch.tensor([[0.0, -1.0, math.inf, math.nan, 1e-300, 1e300, 40.0, 1e-3]], dtype=torch.float64, device=DEV).t()
    r = r.expand(8, 3)                                                    # a view with stride 0
    lower, upper = (v.cpu().numpy() for v in tp.chi2_tails(r, (1, 640, 2 ** 31 - 1), log=True))
    assert (lower[:2] == -math.inf).all() and (upper[:2] == 0).all()
    assert (lower[2] == 0).all() and (upper[2] == -math.inf).all()
    assert np.isnan(lower[3]).all() and np.isnan(upper[3]).all()
    assert np.isfinite(lower[4]).all() and (upper[4] > -1e-100).all() and (lower[5] == 0).all()
    for i in (6, 7):                                                      # far tails: finite logarithms, against 50 digits
        for k, d in enumerate((1, 640)):
            lp, lq = ref.log_tails(d, float(r[i, 0]))
            assert abs(mp.mpf(float(lower[i, k])) - lp) <= TOL * max(1, abs(lp))
            assert abs(mp.mpf(float(upper[i, k])) - lq) <= TOL * max(1, abs(lq))
    assert np.isfinite(upper[6, 2]) and upper[6, 2] < -1e9 and np.isfinite(lower[7, 2]) and lower[7, 2] < -1e9
    flat = tp.chi2_tails(r[6], (1, 640, 2 ** 31 - 1), log=True)                       # a [K] ratio: [K] results
    assert flat[0].shape == flat[1].shape == (3,) and (flat[0].cpu().numpy() == lower[6]).all()
    f32 = tp.chi2_tails(r.float(), (1, 640, 2 ** 31 - 1), log=True)[0].cpu().numpy()
    assert (f32[6] == lower[6]).all()                                     # 40 is exact in fp32


@pytest.mark.gpu
def test_quantiles_round_trip_and_match_the_golden():
    g = golden()
    sizes = [int(d) for d in g["grid_sizes"]]
    assert tuple(g["grid_confidences"]) == CONFIDENCES6
    got = tp.chi2_interval(sizes, CONFIDENCES6, device=DEV).cpu().numpy()
    assert got.shape == (len(sizes), 6, 2)
    worst, used = 0.0, 0.0
    for k, d in enumerate(sizes):
        for j, c in enumerate(CONFIDENCES6):
            for side, prob, gold in ((0, (1.0 - c) / 2.0, g["grid_lower"][k, j]), (1, 1.0 - (1.0 + c) / 2.0, g["grid_upper"][k, j])):
                r = float(got[k, j, side])
                assert 0 < r < math.inf
                logp = mp.log(mp.mpf(prob))
                xh = ref.sensitivity(d, r, bool(side))
                allowed = 2 * TOL * max(1, abs(logp)) + EPS * xh
                dist = abs(ref.log_tails(d, r)[side] - logp)
                used = max(used, float(dist / allowed))
                worst = max(worst, float(dist / max(1, abs(logp))))
                assert dist <= allowed, (d, c, side, r, float(dist / EPS), float(allowed / EPS))
                assert abs(r - gold) <= (SCIPY_PPF_DISTANCE + float(allowed / xh)) * gold, (d, c, side, r, gold)
    print(f"quantiles: at most {used:.3f} of the allowance; worst log-tail distance {worst / EPS:.1f} eps "
          "(that is the one rounding of r at the largest sizes)")
    # the kernel's switch in a (d = 199, 200, 201): at c = .999 the ends lie near u = -0.29 and +0.36, so the Newton steps
    # cross the switch in u as well.  No golden is needed for the round trip.
    extra = tp.chi2_interval(SWITCH_QUANTILE_SIZES, CONFIDENCES6, device=DEV).cpu().numpy()
    for k, d in enumerate(SWITCH_QUANTILE_SIZES):
        for j, c in enumerate(CONFIDENCES6):
            for side, prob in ((0, (1.0 - c) / 2.0), (1, 1.0 - (1.0 + c) / 2.0)):
                r = float(extra[k, j, side])
                logp = mp.log(mp.mpf(prob))
                allowed = 2 * TOL * max(1, abs(logp)) + EPS * ref.sensitivity(d, r, bool(side))
                dist = abs(ref.log_tails(d, r)[side] - logp)
                used = max(used, float(dist / allowed))
                assert dist <= allowed, (d, c, side, r, float(dist / EPS), float(allowed / EPS))
    assert extra[1, 5, 0] - 1 > -_hip.TEMPER_UNIFORM_U and extra[1, 5, 1] - 1 > _hip.TEMPER_UNIFORM_U      # (as said above)
    print(f"with d = 199, 200, 201: at most {used:.3f} of the allowance")
    lo = tp.chi2_quantile((1, 640), [0.0, 1.0, 0.5], upper=False, device=DEV).cpu().numpy()
    assert (lo[:, 0] == 0).all() and (lo[:, 1] == math.inf).all()
    deep = tp.chi2_quantile((640, 10 ** 6), [-800.0, -1e4], upper=True, log=True, device=DEV).cpu().numpy()
    for k, d in enumerate((640, 10 ** 6)):
        for m, t in enumerate((-800.0, -1e4)):
            r = float(deep[k, m])
            assert abs(ref.log_tails(d, r)[1] - t) <= 2 * TOL * abs(t) + EPS * ref.sensitivity(d, r, True), (d, t, r)


@pytest.mark.gpu
def test_coverage_equals_the_golden_counts():
    g = golden()
    assert _golden_margin() >= 1e-9
    sizes, K, S = [int(d) for d in g["sizes"]], len(g["sizes"]), len(g["steps"])
    est = torch.from_numpy(g["est"]).to(DEV)
    temp = torch.from_numpy(g["temperature"]).to(DEV)
    share, smooth, per_tensor, finite = tp.kinetic_coverage(est, temp, sizes, tuple(g["confidences"]), ewma_alpha=0.7)
    assert share.shape == (5, S) and per_tensor.shape == (K, 5) and per_tensor.dtype == torch.int64
    assert (share.cpu().numpy() == g["coverage_a0"]).all()
    assert (share[:, 11] == 0).all() and (share[:, 23] == 0).all()
    want = ref.ewma(g["coverage_a0"], 0.7)
    assert np.max(np.abs(smooth.cpu().numpy() - g["coverage_a07"])) <= ref.bound(want, ref.ewma(g["coverage_a0"], 0.7, np.longdouble))
    with np.errstate(all="ignore"):
        ratio = g["est"] / g["temperature"][:, None]
    assert int(finite) == int(np.isfinite(ratio).sum()) == (S - 2) * K
    inside = (g["lower"][None] <= ratio[:, :, None]) & (ratio[:, :, None] <= g["upper"][None])         # [S, K, C]
    assert (per_tensor.cpu().numpy() == inside.sum(0)).all()
    assert (per_tensor.sum(0).cpu().numpy() == np.rint(g["coverage_a0"].sum(1) * K)).all()
    # the same bits again, for a transposed view, for fp32 storage of an fp32 table, and with a scalar temperature
    again = tp.kinetic_coverage(est, temp, sizes, tuple(g["confidences"]), ewma_alpha=0.7)
    view = est.t().contiguous().t()
    assert view.stride() == (1, S)
    strided = tp.kinetic_coverage(view, temp, sizes, tuple(g["confidences"]), ewma_alpha=0.7)
    wide = torch.zeros(S, 2 * K, dtype=torch.float64, device=DEV)
    wide[:, ::2] = est
    strided2 = tp.kinetic_coverage(wide[:, ::2], temp, sizes, tuple(g["confidences"]), ewma_alpha=0.7)
    for other in (again, strided, strided2):
        assert all(torch.equal(a.view(torch.int64) if a.is_floating_point() else a,
                               b.view(torch.int64) if b.is_floating_point() else b)
                   for a, b in zip((share, smooth, per_tensor, finite), other))
    masked = tp.kinetic_coverage(est[3:30:2], temp[3:30:2], sizes, tuple(g["confidences"]))[0]
    assert (masked.cpu().numpy() == g["coverage_masked"]).all()


@pytest.mark.gpu
def test_interval_ends_are_inclusive():
    "temperature = 1 and est bit-equal to the device's own ends: inside; one ulp beyond: outside"
    sizes = (1, 2, 10, 640, 36864)
    bounds = tp.chi2_interval(sizes, device=DEV)                                   # [K, C, 2]
    K, C = bounds.shape[:2]
    rows = []
    for c in range(C):
        for side in (0, 1):
            rows.append(bounds[:, c, side])
            rows.append(torch.nextafter(bounds[:, c, side], torch.full_like(bounds[:, c, side], -1.0 if side == 0 else 1e9)))
    est = torch.stack(rows)                                                        # [4 C, K]
    share, _, per_tensor, finite = tp.kinetic_coverage(est, 1.0, sizes, bounds=bounds)
    share = share.cpu().numpy() * K
    for c in range(C):
        for side in (0, 1):
            on, beyond = 4 * c + 2 * side, 4 * c + 2 * side + 1
            # an end of level c lies inside every wider level and outside every narrower one
            want_on = [K if cc >= c else 0 for cc in range(C)]
            want_beyond = [K if cc > c else 0 for cc in range(C)]
            assert list(share[:, on]) == want_on, (c, side, share[:, on])
            assert list(share[:, beyond]) == want_beyond, (c, side, share[:, beyond])
    assert int(finite) == est.numel() and (per_tensor.sum(0).cpu().numpy() == share.sum(1)).all()
    zero = tp.kinetic_coverage(est, 0.0, sizes, bounds=bounds)
    assert (zero[0] == 0).all() and (zero[2] == 0).all() and int(zero[3]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,C", [(700, 255, 16), (700, 257, 16), (70001, 3, 5)])
def test_step_table_counts_on_every_route(S, K, C):
    """K C + 1 = 4081 counts are gathered in LDS, 4113 go to memory directly; 70,001 steps are 274 tiles for 256 workgroups,
    so some walk two.  Hand-made intervals; est / temperature is one correctly rounded division on both sides: exact."""
    rng = np.random.default_rng(S + K)
    est = rng.uniform(0.0, 2.0, size=(S, K))
    est[rng.integers(0, S, 20), rng.integers(0, K, 20)] = np.nan
    temp = rng.choice([0.5, 1.0, 0.75], size=S)
    half = (np.arange(C) + 1.0) / (C + 1.0)
    bounds = np.stack([np.broadcast_to(1.0 - half, (K, C)), np.broadcast_to(1.0 + half, (K, C))], axis=2) * rng.uniform(0.9, 1.1, (K, 1, 1))
    ratio = est / temp[:, None]
    inside = (bounds[None, :, :, 0] <= ratio[:, :, None]) & (ratio[:, :, None] <= bounds[None, :, :, 1])        # [S, K, C]
    share, _, per_tensor, finite = tp.kinetic_coverage(torch.from_numpy(est).to(DEV), torch.from_numpy(temp).to(DEV),
                                                       [7] * K, bounds=torch.from_numpy(np.ascontiguousarray(bounds)).to(DEV))
    assert (share.cpu().numpy() == inside.sum(1).T / K).all()
    assert (per_tensor.cpu().numpy() == inside.sum(0)).all() and int(finite) == int(np.isfinite(ratio).sum())


def _table(S, K, seed):
    rng = np.random.default_rng(seed)
    sizes = [int(v) for v in np.concatenate([[1, 36864], rng.integers(1, 5000, size=K - 2)])]
    est = np.stack([0.7 * rng.chisquare(d, size=S) / d for d in sizes], axis=1)
    return sizes, est


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5, 65])
def test_weighted_mean_and_standard_error(K):
    for S in (1, 2, 63, 64, 65, 1025):
        sizes, est = _table(S, K, 100 * K + S)
        w = np.array(sizes, dtype=float)
        m64, s64 = ref.weighted_var_se(w, est)
        ml, sl = ref.weighted_var_se(w, est, np.longdouble)
        for table in (torch.from_numpy(est).to(DEV), torch.from_numpy(np.ascontiguousarray(est.T)).to(DEV).t()):
            mean, se = (v.cpu().numpy() for v in tp.weighted_temperature(table, sizes))
            assert mean.shape == se.shape == (S,)
            assert np.max(np.abs(mean - ml.astype(np.float64))) <= ref.bound(m64, ml), (S, K)
            assert np.max(np.abs(se - sl.astype(np.float64))) <= ref.bound(s64, sl), (S, K)
        f32 = torch.from_numpy(est).float().to(DEV)
        m32 = tp.weighted_temperature(f32, sizes)[0].cpu().numpy()
        ml32 = ref.weighted_var_se(w, f32.cpu().numpy(), np.longdouble)[0]
        assert np.max(np.abs(m32 - ml32.astype(np.float64))) <= ref.bound(ref.weighted_var_se(w, f32.cpu().numpy())[0], ml32)
    bad = torch.from_numpy(est).to(DEV).clone()
    bad[3, 1] = math.nan
    mean, se = tp.weighted_temperature(bad, sizes)
    assert mean[3] != mean[3] and se[3] != se[3] and torch.isfinite(mean[:3]).all() and torch.isfinite(mean[4:]).all()


@pytest.mark.gpu
def test_weighted_mean_matches_the_golden():
    g = golden()
    sizes, w = [int(d) for d in g["sizes"]], g["sizes"].astype(float)
    for tag, table in (("kinetic", g["est"]), ("config", g["config"])):
        mean, se = (v.cpu().numpy() for v in tp.weighted_temperature(torch.from_numpy(table).to(DEV), sizes))
        m64, s64 = ref.weighted_var_se(w, table)
        ml, sl = ref.weighted_var_se(w, table, np.longdouble)
        ok = np.isfinite(g[tag + "_mean"])
        assert (np.isfinite(mean) == ok).all() and (np.isfinite(se) == ok).all()
        assert np.max(np.abs(mean[ok] - g[tag + "_mean"][ok])) <= ref.bound(m64, ml)
        assert np.max(np.abs(se[ok] - g[tag + "_se"][ok])) <= ref.bound(s64, sl)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.999])
def test_ewma(alpha):
    for S in (1, 2, 63, 64, 65, 1025):
        for K in (2, 5, 65):
            _, est = _table(S, K, 7 * S + K)
            x = np.ascontiguousarray(est.T)                                        # [K rows, S]
            y64, yl = ref.ewma(x, alpha), ref.ewma(x, alpha, np.longdouble)
            dev = torch.from_numpy(x).to(DEV)
            y = tp.ewma(dev, alpha)
            assert y.shape == (K, S) and y.dtype == torch.float64
            if alpha == 0.0:
                assert torch.equal(y.view(torch.int64), dev.view(torch.int64))
            else:
                assert np.max(np.abs(y.cpu().numpy() - yl.astype(np.float64))) <= ref.bound(y64, yl), (S, K)
            strided = tp.ewma(torch.from_numpy(est).to(DEV).t(), alpha)           # the same rows as a transposed view
            assert torch.equal(strided.view(torch.int64), y.view(torch.int64))
            assert torch.equal(tp.ewma(dev[0], alpha).view(torch.int64), y[0].view(torch.int64))
    # a NaN poisons what follows it in its own row, and nothing else
    S, K = 1025, 5
    _, est = _table(S, K, 5)
    clean = torch.from_numpy(np.ascontiguousarray(est.T)).to(DEV)
    dirty = clean.clone()
    dirty[2, 700] = math.nan
    dirty[4, 0] = -0.0
    a, b = tp.ewma(clean, alpha), tp.ewma(dirty, alpha)
    assert torch.equal(a[:2].view(torch.int64), b[:2].view(torch.int64)) and torch.equal(a[3].view(torch.int64), b[3].view(torch.int64))
    assert torch.equal(a[2, :700].view(torch.int64), b[2, :700].view(torch.int64))
    if alpha == 0.0:
        assert torch.equal(b.view(torch.int64), dirty.view(torch.int64))          # -0.0 and the NaN's payload included
    else:
        assert torch.isnan(b[2, 700:]).all() and torch.isfinite(b[4]).all()


@pytest.mark.gpu
def test_ewma_keeps_an_infinite_value_where_the_scan_weights_underflow():
    """alpha = 1e-5 at S = 100,000: a thread owns 391 steps and alpha^391 = 0 in fp64.  Step by step an infinite value stays
    infinite in everything after it; the scan must not turn it into 0 * inf = NaN, nor lose it."""
    S, alpha = 100_000, 1e-5
    x = np.random.default_rng(3).standard_normal((3, S))
    x[0, 10], x[1, 50_000] = math.inf, -math.inf
    want = ref.ewma(x, alpha)
    assert np.isposinf(want[0, 10:]).all() and np.isneginf(want[1, 50_000:]).all() and np.isfinite(want[2]).all()
    y = tp.ewma(torch.from_numpy(x).to(DEV), alpha).cpu().numpy()
    assert (np.isposinf(y) == np.isposinf(want)).all() and (np.isneginf(y) == np.isneginf(want)).all()
    assert not np.isnan(y).any()
    ok = np.isfinite(want)
    assert np.max(np.abs(y[ok] - want[ok])) <= ref.bound(np.where(ok, want, 0.0), np.where(ok, ref.ewma(x, alpha, np.longdouble), 0.0))


def _write_metrics(saver, g, names):
    "the golden table as a runner logs it: per step the per-tensor columns, the /all rows and the target"
    for s, step in enumerate(g["steps"].tolist()):
        for k, n in enumerate(names):
            saver.add_scalar("est_temperature/" + n, float(g["est"][s, k]), step)
            saver.add_scalar("est_config_temp/" + n, float(g["config"][s, k]), step)
        saver.add_scalar("est_temperature/all", 1.0, step)
        saver.add_scalar("est_config_temp/all", 1.0, step)
        saver.add_scalar("temperature", float(g["temperature"][s]), step)
        saver.add_scalar("acceptance/is_sample", 1, step)


def test_columns_of_an_hdf5_metrics_file_keep_the_nested_datasets(tmp_path):
    from bnn_priors_amd import _h5, storage
    if not _h5.available():
        pytest.skip("libhdf5 (>= 1.10) not found on this machine")
    g = golden()
    names = [str(n) for n in g["names"]]
    memory = storage.MemoryMetrics()
    _write_metrics(memory, g, names)
    with storage.HDF5Metrics(tmp_path / "metrics.h5", "w", chunk_size=8) as saver:          # several chunks: 37 rows
        _write_metrics(saver, g, names)
    from_file, from_memory = tp._columns(tmp_path / "metrics.h5"), tp._columns(memory)
    assert {"steps", "temperature"} | {f"{p}/{n}" for p in ("est_temperature", "est_config_temp") for n in names} <= set(from_file)
    for key in ["temperature"] + ["est_temperature/" + n for n in names] + ["est_config_temp/" + n for n in names]:
        assert np.array_equal(np.asarray(from_file[key], dtype=np.float64), from_memory[key], equal_nan=True), key
    assert (from_file["steps"] == g["steps"]).all() and (from_memory["steps"] == g["steps"]).all()


@pytest.mark.gpu
def test_report_is_the_same_from_a_file_a_memory_sink_and_a_dict(tmp_path):
    from bnn_priors_amd import _h5, storage
    g = golden()
    names = [str(n) for n in g["names"]]
    sizes = dict(zip(names, (int(d) for d in g["sizes"])))
    memory = storage.MemoryMetrics()
    _write_metrics(memory, g, names)
    columns = dict({"steps": g["steps"], "temperature": g["temperature"]},
                   **{"est_temperature/" + n: g["est"][:, k] for k, n in enumerate(names)},
                   **{"est_config_temp/" + n: g["config"][:, k] for k, n in enumerate(names)})
    sources = {"memory": memory, "dict": columns}
    if _h5.available():
        with storage.HDF5Metrics(tmp_path / "metrics.h5", "w", chunk_size=8) as saver:
            _write_metrics(saver, g, names)
        sources["file"] = str(tmp_path / "metrics.h5")
        sources["path"] = tmp_path / "metrics.h5"
    reports = {k: tp.temperature_report(v, sizes, ewma_alpha=0.7, pit=True) for k, v in sources.items()}
    first = reports["dict"]
    assert (first["coverage"].cpu().numpy() == g["coverage_a0"]).all() and first["names"] == tuple(sorted(names))
    for tag, rep in reports.items():
        assert set(rep) == set(first), tag
        for key, value in first.items():
            if isinstance(value, torch.Tensor):
                a, b = value, rep[key]
                assert a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.is_floating_point() else a,
                                                          b.view(torch.int64) if b.is_floating_point() else b), (tag, key)
            else:
                assert value == rep[key], (tag, key)
    masked = tp.temperature_report(sources.get("file", memory), sizes, mask=slice(3, 30, 2))
    assert (masked["coverage"].cpu().numpy() == g["coverage_masked"]).all()


@pytest.mark.gpu
def test_ewma_matches_the_golden():
    g = golden()
    x = torch.from_numpy(g["ewma_input"]).to(DEV)
    for tag, alpha in (("a0", 0.0), ("a05", 0.5), ("a0999", 0.999)):
        y = tp.ewma(x, alpha).cpu().numpy()
        y64, yl = ref.ewma(g["ewma_input"], alpha), ref.ewma(g["ewma_input"], alpha, np.longdouble)
        if alpha == 0.0:
            assert (y == g["ewma_a0"]).all()
        else:
            assert np.max(np.abs(y - g["ewma_" + tag])) <= ref.bound(y64, yl)


@pytest.mark.gpu
def test_report_of_a_run_equals_its_pieces():
    """A VerletSGLDRunner on scenarios' product of Gaussians into a MemoryMetrics: the report is the pieces called one by
    one.  Nothing statistical is claimed about 240 steps of a chain."""
    import scenarios
    from bnn_priors_amd import goodness_of_fit, inference, models
    from bnn_priors_amd.storage import MemoryMetrics
    torch.manual_seed(0)
    model, _ = scenarios.make_model("gauss", models, torch.float32, device=DEV)
    x, y = torch.zeros(8, 1, device=DEV), torch.zeros(8, 1, device=DEV)
    data = torch.utils.data.TensorDataset(x, y)
    train = torch.utils.data.DataLoader(data, batch_size=1)
    test = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:0], y[:0]), batch_size=1)
    metrics = MemoryMetrics()
    runner = inference.VerletSGLDRunner(model=model, dataloader=train, dataloader_test=test, epochs_per_cycle=30,
                                        warmup_epochs=5, sample_epochs=10, learning_rate=1 / 32, skip=1, metrics_skip=1,
                                        temperature=0.75, momentum=0.9, sampling_decay="flat", cycles=1,
                                        metrics_saver=metrics, model_saver=None, seed=7, chain_id=0)
    runner.run()
    sizes = tp.get_sizes(model)
    names = [n for n, _ in model.named_parameters()]
    assert len(names) == 3 and all(sizes[n] == 50 for n in names)
    rep = tp.temperature_report(metrics, model, ewma_alpha=0.9, pit=True)
    S, K, C = len(rep["steps"]), 3, len(tp.CONFIDENCES)
    assert S >= 240 and rep["names"] == tuple(names)
    assert set(rep) == {"steps", "names", "sizes", "temperature", "confidences", "intervals", "coverage", "coverage_smoothed",
                        "coverage_per_tensor", "finite", "kinetic_mean", "kinetic_se", "config_mean", "config_se", "pit",
                        "log_lower", "log_upper"}
    shapes = dict(temperature=(S,), intervals=(K, C, 2), coverage=(C, S), coverage_smoothed=(C, S), coverage_per_tensor=(K, C),
                  finite=(), kinetic_mean=(S,), kinetic_se=(S,), config_mean=(S,), config_se=(S,), pit=(S, K),
                  log_lower=(S, K), log_upper=(S, K), sizes=(K,))
    for key, shape in shapes.items():
        assert tuple(rep[key].shape) == shape and rep[key].is_cuda, key
    steps, _ = metrics.column("temperature")
    assert (rep["steps"].numpy() == steps).all()
    est = torch.from_numpy(np.stack([metrics.column("est_temperature/" + n)[1] for n in names], 1)).to(DEV)
    cfg = torch.from_numpy(np.stack([metrics.column("est_config_temp/" + n)[1] for n in names], 1)).to(DEV)
    temp = torch.from_numpy(metrics.column("temperature")[1]).to(DEV)
    bits = lambda t: t.view(torch.int64) if t.is_floating_point() else t
    same = lambda a, b: torch.equal(bits(a), bits(b))
    d = [50, 50, 50]
    assert same(rep["intervals"], tp.chi2_interval(d, device=DEV))
    share, smooth, per_tensor, finite = tp.kinetic_coverage(est, temp, d, ewma_alpha=0.9)
    assert same(rep["coverage"], share) and same(rep["coverage_smoothed"], smooth)
    assert same(rep["coverage_per_tensor"], per_tensor) and same(rep["finite"], finite)
    assert same(rep["coverage_smoothed"], tp.ewma(share, 0.9))
    mean, se = tp.weighted_temperature(est, d)
    assert same(rep["kinetic_mean"], mean) and same(rep["kinetic_se"], se)
    mean, se = tp.weighted_temperature(cfg, d)
    assert same(rep["config_mean"], mean) and same(rep["config_se"], se)
    lower, upper = tp.chi2_tails(est, d, temperature=temp)
    assert same(rep["log_lower"], lower) and same(rep["log_upper"], upper)
    assert same(rep["pit"], tp.chi2_tails(est, d, log=False, temperature=temp)[0])
    with np.errstate(all="ignore"):                       # (the descent epochs run at temperature 0: inf, outside)
        assert int(finite) == int(np.isfinite(est.cpu().numpy() / temp.cpu().numpy()[:, None]).sum()) > 0
    # equal weights: the mean is the plain mean; a sub-range of the rows is the report of those rows
    ok = torch.isfinite(est).all(1)
    assert torch.allclose(rep["kinetic_mean"][ok], est[ok].mean(1), rtol=1e-14, atol=0)
    part = tp.temperature_report(metrics, sizes, mask=slice(10, 200, 3))
    assert same(part["coverage"], share[:, 10:200:3]) and (part["steps"].numpy() == steps[10:200:3]).all()
    # the PIT is what goodness_of_fit scores against the uniform law, as it stands
    u = rep["pit"][torch.isfinite(rep["pit"]).all(1)]
    table = goodness_of_fit.goodness_of_fit(u, fits={"uniform": (0., 1.)})
    assert 0.0 <= table["uniform"].ks <= 1.0 and table["uniform"].n == u.numel()
