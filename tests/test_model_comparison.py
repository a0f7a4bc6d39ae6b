"""PSIS-LOO and WAIC on the device (bnn_priors_amd/model_comparison.py, csrc/psis_hip.inc; the definition is in
include/sgmcmc_hip.h and restated in tests/psis_reference.py).

On the CPU: the restatement against what it should recover (generalised Pareto tails, a conjugate model's closed-form
leave-one-out densities), the module's argument checking, ``compare``'s arithmetic, and the two checks that carry the
GPU comparison rule.  On the GPU: the kernels against the restatement, every observation of every case.

Comparison rule:
* M, n2, the tail membership with its order, the cutoff (a selection), the non-finite flags and khat = inf: bit-equal;
* khat, sigma, lw, the pointwise outputs and the totals: rtol = 1e-9, atol = 1e-9, the project's rule for fixed-order
  fp64 sums (tests/test_chain_diagnostics.py).  It stands on ``test_summation_order_moves_no_output_by_1e_11``: over
  every GPU case the restatement evaluated with numpy's pairwise sums and with exactly rounded sums (``math.fsum``)
  differs by at most 2.9e-14 in units of (1 + |value|) -- 30,000 times below the rule.  The device's libm (exp, log,
  log1p, expm1 within a few ulp) enters at the same level as the order of summation: the largest difference between
  the device and the restatement over all cases below is 4.7e-13 in the same units (the total se of the 32,768-draw
  case; 3.1e-14 elsewhere);
* no observation is left out of any comparison.
M is decided by ceil(3 sqrt(S / r_eff)): ``test_gpu_case_inputs_keep_the_tail_length_away_from_rounding`` asserts that
no case's argument is within 1e-6 of an integer unless it is exactly one."""
import functools
import math

import numpy as np
import pytest
import scipy.stats
import torch

from chain_diag_reference import chain_diag_reference
from psis_reference import (FIELDS, LOG_DBL_MIN, compare as compare_reference, gpd_fit, k_threshold, logsumexp,
                            psis_column, psis_reference, tail_length, totals as totals_reference)

from bnn_priors_amd import _hip
from bnn_priors_amd import evaluation as ev
from bnn_priors_amd import model_comparison as mc

RTOL = ATOL = 1e-9
SPREAD = 1e-11
MARGIN = 1e-9
INVALID_VALUE = 1           # hipErrorInvalidValue


# ---- the families and the cases --------------------------------------------------------------------------------------

def _normal(rng, S, N):
    return -0.5 * rng.standard_normal((S, N)) ** 2


def _student(rng, S, N):
    return -2.0 * np.log1p(rng.standard_t(3, (S, N)) ** 2 / 3.0)


def _cauchy(rng, S, N):
    return -np.abs(rng.standard_cauchy((S, N)))


def _ties(rng, S, N):
    "ll rounded to halves (tied order statistics, n2 < M), -0.0 beside 0.0, one constant column"
    ll = np.round(_normal(rng, S, N) * 2.0) / 2.0
    ll[:6, 3] = [-0.0, 0.0, 0.0, -0.0, -0.5, 0.0]
    ll[:, 11] = -1.5
    return ll


def _floor(rng, S, N):
    "each column's range of ll exceeds 800: most draws lie below the cutoff's floor log DBL_MIN"
    return 8000.0 * rng.random((S, N))


def _make(family, seed, S, N):
    return lambda: (family(np.random.default_rng(seed), S, N), None)


def _per_lane(seed, S, N):
    rng = np.random.default_rng(seed)
    return _student(rng, S, N), rng.uniform(0.1, 1.5, N)


# name -> (ll [S, N] fp64, r_eff [N] or None)
CASES = {
    "lanes_1": _make(_normal, 1, 40, 1),
    "lanes_63": _make(_normal, 2, 40, 63),
    "lanes_65": _make(_student, 3, 40, 65),
    "lanes_130": _make(_normal, 4, 40, 130),
    "nofit_20": _make(_normal, 5, 20, 5),
    "fit_24": _make(_normal, 6, 24, 5),
    "fit_25": _make(_student, 7, 25, 5),
    "sqrt_400": _make(_normal, 8, 400, 5),
    "sqrt_2400": _make(_student, 9, 2400, 3),
    "longest": _make(_student, 10, 32768, 3),
    "ties": _make(_ties, 11, 60, 65),
    "floor": _make(_floor, 12, 50, 5),
    "heavy": _make(_cauchy, 13, 400, 65),
    "per_lane": lambda: _per_lane(14, 400, 65),
    "fp32": _make(_student, 15, 100, 65),
    "strided": _make(_normal, 16, 100, 65),
    "chunks": _make(_student, 17, 100, 300),
}
F32_CASES = ("fp32",)
EXPECTED_M = {"nofit_20": 4, "fit_24": 5, "fit_25": 5, "sqrt_400": 60, "sqrt_2400": 147, "longest": 544}


@functools.lru_cache(maxsize=None)
def _case(name):
    "(ll, r_eff, reference), computed once and shared; an fp32 case: the values rounded to fp32, seen widened"
    ll, r_eff = CASES[name]()
    if name in F32_CASES:
        ll = ll.astype(np.float32)
    ll.setflags(write=False)
    return ll, r_eff, psis_reference(ll.astype(np.float64), r_eff)


def _nan_rule_inputs():
    "(ll with a NaN, a +inf and a -inf; the mask of those columns; the clean draws)"
    clean = _normal(np.random.default_rng(18), 30, 72)
    ll = clean.copy()
    bad = np.zeros(72, dtype=bool)
    bad[[5, 64, 70]] = True
    ll[3, 5] = np.nan
    ll[29, 64] = np.inf
    ll[0, 70] = -np.inf
    return ll, bad, clean


def _ar1_ll(phi, M=4, S=100, N=65, seed=19):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((M, S, N))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi ** 2)
    for s in range(1, S):
        x[:, s] = phi * x[:, s - 1] + e[:, s]
    return -0.5 * x ** 2


# ---- CPU: the restatement --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [-0.3, 0.2, 0.7])
def test_reference_fit_recovers_generalised_pareto_tails(k):
    "200 replicates of n = 500 draws: the mean khat is the shrunk shape (n k + 5) / (n + 10) within 4 standard errors"
    n, reps = 500, 200
    rng = np.random.default_rng(0)
    draws = scipy.stats.genpareto.rvs(k, size=(reps, n), random_state=rng)
    khat = np.array([gpd_fit(np.sort(row))[0] for row in draws])
    want, err = (n * k + 5.0) / (n + 10.0), khat.std(ddof=1) / math.sqrt(reps)
    print("k", k, "mean khat", khat.mean(), "expected", want, "standard error", err)
    assert abs(khat.mean() - want) <= 4.0 * err


def test_reference_loo_matches_the_conjugate_normal_mean_model():
    """y_i ~ N(mu, 1), mu ~ N(0, 10^2), N = 50: PSIS-LOO from 4,000 exact posterior draws equals the closed-form
    log p(y_i | y_-i) of every observation within four Monte-Carlo standard errors (of the self-normalised estimate:
    sum_s w_s^2 (p_s - p_hat)^2 with the normalised weights, on the log scale divided by p_hat)."""
    rng = np.random.default_rng(1)
    N, S, tau2 = 50, 4000, 100.0
    y = rng.normal(0.7, 1.0, N)
    post_var = 1.0 / (1.0 / tau2 + N)
    mu = rng.normal(post_var * y.sum(), math.sqrt(post_var), S)
    ll = scipy.stats.norm.logpdf(y[None, :], mu[:, None], 1.0)
    ref = psis_reference(ll)
    loo_var = 1.0 / (1.0 / tau2 + N - 1)
    exact = scipy.stats.norm.logpdf(y, loo_var * (y.sum() - y), np.sqrt(1.0 + loo_var))
    w, p = np.exp(ref.lw), np.exp(ll)
    p_hat = (w * p).sum(axis=0)
    mcse = np.sqrt((w ** 2 * (p - p_hat) ** 2).sum(axis=0)) / p_hat
    z = (ref.elpd_loo - exact) / mcse
    print("largest |error| / mcse", np.abs(z).max(), "largest khat", ref.pareto_k.max())
    np.testing.assert_allclose(np.log(p_hat), ref.elpd_loo, rtol=1e-12, atol=1e-12)
    assert (np.abs(z) <= 4.0).all()
    assert ref.pareto_k.max() < 0.7


def test_reference_weights_sum_to_one_and_khat_is_inf_iff_the_tail_is_short():
    seen = set()
    for name in CASES:
        ll, r_eff, ref = _case(name)
        lse = np.array([logsumexp(ref.lw[:, i]) for i in range(ref.lw.shape[1])])
        np.testing.assert_allclose(lse, 0.0, atol=1e-12)
        np.testing.assert_array_equal(np.isposinf(ref.pareto_k), ref.n2 <= 4)
        assert (ref.n2 <= ref.M).all() and ((ref.tail_pos >= 0).sum(axis=0) == ref.n2).all()
        seen |= set((ref.n2 <= 4).tolist())
        if name in EXPECTED_M:
            assert (ref.M == EXPECTED_M[name]).all(), name
    assert seen == {True, False}
    assert np.isposinf(_case("nofit_20")[2].pareto_k).all() and np.isfinite(_case("fit_24")[2].pareto_k).all()


def test_reference_cases_reach_the_edges_they_are_named_for():
    ties = _case("ties")[2]
    assert (ties.n2 < ties.M).sum() >= 30 and ties.n2[11] == 0 and np.isposinf(ties.pareto_k[11])
    np.testing.assert_array_equal(ties.lw[:, 11], -np.log(60.0))                 # a constant column: uniform weights
    ll, _, floor = _case("floor")
    assert (np.ptp(ll, axis=0) > 800).all() and (floor.cut == LOG_DBL_MIN).all()
    assert (floor.n2 > 4).any() and (floor.n2 <= 4).any()
    assert (_case("heavy")[2].pareto_k > 1.0).sum() >= 30
    per_lane = _case("per_lane")[2]
    assert len(set(per_lane.M.tolist())) >= 10
    ll, bad, clean = _nan_rule_inputs()
    ref = psis_reference(ll)
    for f in FIELDS:
        assert np.isnan(getattr(ref, f)[bad]).all() and np.isfinite(getattr(ref, f)[~bad]).all(), f


def test_summation_order_moves_no_output_by_1e_11():
    """The tolerance derivation: every GPU case through the restatement once with numpy's pairwise sums and once with
    exactly rounded sums (math.fsum).  The largest |difference| / (1 + |value|) over every output of every column of
    every case is 2.9e-14 (a log weight of the cauchy case), asserted below 1e-11: 100 times below the rule's 1e-9."""
    worst = (0.0, None)
    inputs = [(name,) + _case(name)[:2] for name in CASES] + [("nan_rule", _nan_rule_inputs()[0], None)]
    inputs += [("nan_rule clean", _nan_rule_inputs()[2], None)]
    for phi in (0.0, 0.9):
        ll = _ar1_ll(phi)
        inputs.append((f"ar1 {phi}", ll.reshape(400, 65), chain_diag_reference(np.exp(ll), split=False).ess / 400.0))
    for name, ll, r_eff in inputs:
        ll = np.asarray(ll, dtype=np.float64)
        for i in range(ll.shape[1]):
            re = 1.0 if r_eff is None else r_eff[i]
            a, b = psis_column(ll[:, i], re), psis_column(ll[:, i], re, total=math.fsum)
            assert a["n2"] == b["n2"] and a["M"] == b["M"]
            for f in FIELDS + ("sigma", "lw"):
                va, vb = np.atleast_1d(a[f]), np.atleast_1d(b[f])
                np.testing.assert_array_equal(np.isfinite(va), np.isfinite(vb))
                ok = np.isfinite(va)
                if ok.any():
                    spread = float((np.abs(va[ok] - vb[ok]) / (1.0 + np.abs(vb[ok]))).max())
                    worst = max(worst, (spread, (name, i, f)))
    print("largest spread between numpy's order and math.fsum:", worst)
    assert worst[0] < SPREAD


def test_gpu_case_inputs_keep_the_tail_length_away_from_rounding():
    for name in CASES:
        ll, r_eff, _ = _case(name)
        S = ll.shape[0]
        for re in ([1.0] if r_eff is None else r_eff):
            arg = 3.0 * math.sqrt(S / re)
            exact = re == 1.0 and math.isqrt(S) ** 2 == S
            assert exact or abs(arg - round(arg)) >= 1e-6, (name, re)
            assert tail_length(S, re) == math.ceil(min(0.2 * S, arg))


def test_relative_eff_inputs_leave_no_observation_out():
    for phi in (0.0, 0.9):
        ref = chain_diag_reference(np.exp(_ar1_ll(phi)), split=False)
        assert (ref.margin >= MARGIN).all(), (phi, ref.margin.min())


# ---- CPU: the module -------------------------------------------------------------------------------------------------

def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was touched"))
    good = torch.zeros(10, 3, dtype=torch.float64)
    for fn in (mc.psis, mc.loo, mc.waic):
        for bad in (None, np.zeros((10, 3)), torch.zeros(10, 3, dtype=torch.int64), torch.zeros(10),
                    torch.zeros(2, 2, 5, 3), torch.zeros(4, 3), torch.zeros(mc.MAX_DRAWS + 1, 1), torch.zeros(10, 0),
                    good):                                                       # ... the last: not on the device
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError, match="workspace_bytes"):
            fn(good, workspace_bytes=100)
    for fn in (mc.psis, mc.loo):
        for r_eff in (np.ones(3), torch.ones(3), torch.ones(4, dtype=torch.float64),
                      torch.ones(1, 3, dtype=torch.float64)):
            with pytest.raises(ValueError, match="r_eff"):
                fn(good, r_eff=r_eff)
    for bad in (None, torch.zeros(10, 3), torch.zeros(2, 3, 5), torch.zeros(2, 10, 3, dtype=torch.int32),
                torch.zeros(2, 10, 3)):
        with pytest.raises(ValueError):
            mc.relative_eff(bad)
    for bad in (None, {}, {"a": 1.0}):
        with pytest.raises(ValueError):
            mc.compare(bad)
    a = mc.WaicResult(-3.0, 1.0, 0.5, torch.zeros(4, dtype=torch.float64))
    b = mc.LooResult(-3.0, 1.0, 0.5, -2.5, torch.zeros(4, dtype=torch.float64), torch.zeros(4), 0.7, 0, 0.1)
    with pytest.raises(ValueError):
        mc.compare({"a": a, "b": b})                                             # two kinds of estimate
    with pytest.raises(ValueError, match="observations"):
        mc.compare({"a": a, "b": a._replace(pointwise=torch.zeros(5, dtype=torch.float64))})
    with pytest.raises(ValueError):
        ev.evaluate_marglik(None, {"w": torch.zeros(3, 2)}, {"w": torch.zeros(4, 2)})


def test_compare_arithmetic_on_hand_made_pointwise_vectors():
    pw = {"a": np.array([-1.0, -2.0, -3.0, -4.0]), "b": np.array([-1.5, -1.5, -3.5, -4.5]),
          "c": np.array([-0.5, -2.0, -2.5, -4.0])}
    res = {n: mc.WaicResult(float(v.sum()), 0.25, 0.0, torch.from_numpy(v)) for n, v in pw.items()}
    rows = mc.compare(res)
    assert [r.name for r in rows] == ["c", "a", "b"]
    assert [r.elpd for r in rows] == [-9.0, -10.0, -11.0] and [r.elpd_diff for r in rows] == [0.0, -1.0, -2.0]
    # a - c = (-.5, 0, -.5, 0): variance 1/12, dse = sqrt(4 / 12); b - c = (-1, .5, -1, -.5): variance 0.5, sqrt(2)
    assert rows[0].dse == 0.0
    assert rows[1].dse == pytest.approx(math.sqrt(1.0 / 3.0), rel=1e-14)
    assert rows[2].dse == pytest.approx(math.sqrt(2.0), rel=1e-14)
    for row, (name, elpd, diff, dse) in zip(rows, compare_reference(pw)):
        assert (row.name, row.elpd, row.elpd_diff) == (name, elpd, diff) and row.dse == pytest.approx(dse, rel=1e-14)
    loo = {n: mc.LooResult(r.elpd_waic, 0.25, 0.0, 0.0, r.pointwise, torch.zeros(4), 0.7, 0, 0.0)
           for n, r in res.items()}
    assert [(r.name, r.elpd_diff) for r in mc.compare(loo)] == [("c", 0.0), ("a", -1.0), ("b", -2.0)]


def test_workspace_arithmetic_matches_the_header():
    assert mc.tail_rows(32768, False) == mc.tail_rows(32768, True) == mc.MAX_TAIL == 544
    assert mc.tail_rows(2400, False) == 147 and mc.tail_rows(2400, True) == 480 and mc.tail_rows(20, False) == 4
    assert mc.bytes_per_observation(2400, False) == 8 * 147 + 64 + 4800
    assert mc.k_threshold(2400) == 0.7 and mc.k_threshold(40) == k_threshold(40) == 1 - 1 / math.log10(40)
    lib = _hip.lib()
    for S, N, has in ((2400, 60000, 0), (2400, 64, 1), (5, 1, 0), (32768, 3, 1)):
        assert lib.sgmcmc_psis_workspace_bytes(S, N, has) == N * mc.bytes_per_observation(S, bool(has))
    assert lib.sgmcmc_psis_workspace_bytes(4, 1, 0) == -1 and lib.sgmcmc_psis_workspace_bytes(32769, 1, 0) == -1


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _np(t):
    return t.cpu().numpy()


def _device(ll, r_eff=None, workspace_bytes=None, is_ratio=False):
    """sgmcmc_psis_loo on a device tensor ``ll`` [S, N] (any draw stride) -> dict of numpy arrays shaped like the
    restatement's; with the default workspace (one chunk) also ``tail_pos`` read from the workspace's pos array"""
    S, N = ll.shape
    dev = ll.device
    has = r_eff is not None
    per = mc.bytes_per_observation(S, has)
    one_chunk = workspace_bytes is None
    nbytes = per * N if one_chunk else workspace_bytes
    work = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    pw = torch.full((6, N), -7.0, dtype=torch.float64, device=dev)
    fit = torch.full((2, N), -7.0, dtype=torch.float64, device=dev)
    counts = torch.full((2, N), -7, dtype=torch.int32, device=dev)
    lw = torch.full((S, N), -7.0, dtype=torch.float64, device=dev)
    tot = torch.full((9,), -7.0, dtype=torch.float64, device=dev)
    L = _hip.lib()
    stream = torch.cuda.current_stream().cuda_stream
    _hip.check(L.sgmcmc_psis_loo(ll.data_ptr(), int(ll.dtype == torch.float64), int(is_ratio), ll.stride(0), S, N,
                                 r_eff.data_ptr() if has else None, work.data_ptr(), nbytes, pw.data_ptr(),
                                 fit.data_ptr(), counts.data_ptr(), lw.data_ptr(), stream), "sgmcmc_psis_loo")
    _hip.check(L.sgmcmc_psis_totals(pw.data_ptr(), N, mc.k_threshold(S), tot.data_ptr(), stream), "sgmcmc_psis_totals")
    out = dict(zip(FIELDS, _np(pw)))
    out.update(sigma=_np(fit[0]), cut=_np(fit[1]), M=_np(counts[0]), n2=_np(counts[1]), lw=_np(lw),
               totals=dict(zip(mc.TOTALS, _np(tot).tolist())))
    if one_chunk:
        rows = mc.tail_rows(S, has)
        pos = work.view(torch.uint8)[(8 * rows + 64) * N:][:2 * S * N].view(torch.int16).view(S, N)
        pos = _np(pos).astype(np.int64) & 0xffff                                 # uint16: a row from the top, or 0xffff
        out["tail_pos"] = np.where(pos == 0xffff, -1, out["n2"][None, :] - 1 - pos)
    return out


def _assert_matches(got, ref, S, name=""):
    "the comparison rule of the module's docstring, every observation"
    np.testing.assert_array_equal(got["M"], ref.M, err_msg=name)
    np.testing.assert_array_equal(got["n2"], ref.n2, err_msg=name)
    if "tail_pos" in got:
        np.testing.assert_array_equal(got["tail_pos"], ref.tail_pos, err_msg=name)
    np.testing.assert_array_equal(got["cut"], ref.cut, err_msg=name)
    worst = {}
    for f in FIELDS + ("sigma", "lw"):
        a, b = got[f], getattr(ref, f)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{name} {f}")
        np.testing.assert_array_equal(np.isposinf(a), np.isposinf(b), err_msg=f"{name} {f}")
        ok = np.isfinite(b)
        worst[f] = float((np.abs(a[ok] - b[ok]) / (1.0 + np.abs(b[ok]))).max()) if ok.any() else 0.0
    want = totals_reference(ref, S)
    for f, v in want.items():
        ok = math.isfinite(v) and math.isfinite(got["totals"][f])
        worst["total " + f] = abs(got["totals"][f] - v) / (1.0 + abs(v)) if ok else 0.0
    print(name, "largest |device - restatement| / (1 + |value|):", max(worst.values()), max(worst, key=worst.get))
    for f in FIELDS + ("sigma", "lw"):
        np.testing.assert_allclose(got[f], getattr(ref, f), rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=f"{name} {f}")
    for f, v in want.items():
        np.testing.assert_allclose(got["totals"][f], v, rtol=RTOL, atol=ATOL, equal_nan=True,
                                   err_msg=f"{name} total {f}")
    assert got["totals"]["n_bad"] == want["n_bad"]
    return max(worst.values())


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n not in ("strided", "chunks")])
def test_device_matches_the_restatement(name):
    ll, r_eff, ref = _case(name)
    x = _cuda(ll)
    re = None if r_eff is None else _cuda(r_eff)
    assert x.dtype == (torch.float32 if name in F32_CASES else torch.float64)
    got = _device(x, re)
    _assert_matches(got, ref, ll.shape[0], name)
    # the public functions return the same bits
    res, wres = mc.loo(x, re), mc.waic(x)
    np.testing.assert_array_equal(_np(res.pointwise), got["elpd_loo"])
    np.testing.assert_array_equal(_np(res.pareto_k), got["pareto_k"])
    np.testing.assert_array_equal([res.elpd_loo, res.se, res.p_loo, res.lppd, res.n_bad, res.k_max], [
        got["totals"][k] for k in ("elpd_loo", "se_loo", "p_loo", "lppd", "n_bad", "k_max")])      # (N = 1: se is NaN)
    assert res.k_threshold == k_threshold(ll.shape[0])
    if r_eff is None:
        np.testing.assert_array_equal(_np(wres.pointwise), got["elpd_waic"])
        np.testing.assert_array_equal([wres.elpd_waic, wres.se, wres.p_waic],
                                      [got["totals"][k] for k in ("elpd_waic", "se_waic", "p_waic")])
    lw, k = mc.psis(-x, re)
    np.testing.assert_array_equal(_np(lw), got["lw"])
    np.testing.assert_array_equal(_np(k), got["pareto_k"])


@pytest.mark.gpu
def test_device_reads_a_strided_chain_table_in_place():
    "[M, S, N] as a view into a wider table: draw_stride > N, the chains one draw stride apart -- no copy"
    ll, _, ref = _case("strided")
    wide = torch.full((4, 25, 80), float("nan"), dtype=torch.float64, device="cuda:0")
    wide[:, :, :65] = _cuda(ll).view(4, 25, 65)
    view = wide[:, :, :65]
    table, E, N = mc._check(view, None, 256 << 20)
    assert (E, N) == (100, 65) and table.data_ptr() == wide.data_ptr() and table.stride() == (80, 1)
    got = _device(table)
    _assert_matches(got, ref, 100, "strided")
    res = mc.loo(view)
    np.testing.assert_array_equal(_np(res.pointwise), got["elpd_loo"])
    lw, k = mc.psis(-view)
    np.testing.assert_array_equal(_np(lw), got["lw"])


@pytest.mark.gpu
def test_chunking_changes_no_bit():
    ll, _, ref = _case("chunks")
    x = _cuda(ll)
    whole = _device(x)
    _assert_matches(whole, ref, 100, "chunks")
    small = 64 * mc.bytes_per_observation(100, False) + 100                      # 64 observations per chunk: 5 chunks
    got = _device(x, workspace_bytes=small)
    for f in FIELDS + ("sigma", "cut", "M", "n2", "lw"):
        np.testing.assert_array_equal(got[f], whole[f], err_msg=f)
    assert got["totals"] == whole["totals"]
    res = mc.loo(x, workspace_bytes=small)
    np.testing.assert_array_equal(_np(res.pointwise), whole["elpd_loo"])
    lw, k = mc.psis(-x, workspace_bytes=small)
    np.testing.assert_array_equal(_np(lw), whole["lw"])
    L = _hip.lib()
    tiny = torch.zeros(small // 8, dtype=torch.float64, device="cuda:0")
    pw = torch.zeros(6, 300, dtype=torch.float64, device="cuda:0")
    short = 63 * mc.bytes_per_observation(100, False)                           # not even one chunk of 64
    assert L.sgmcmc_psis_loo(x.data_ptr(), 1, 0, 300, 100, 300, None, tiny.data_ptr(), short, pw.data_ptr(), None, None,
                             None, None) == INVALID_VALUE
    assert L.sgmcmc_psis_loo(x.data_ptr(), 1, 0, 299, 100, 300, None, tiny.data_ptr(), small, pw.data_ptr(), None, None,
                             None, None) == INVALID_VALUE                        # draw_stride < N
    assert L.sgmcmc_psis_loo(x.data_ptr(), 1, 0, 300, 4, 300, None, tiny.data_ptr(), small, pw.data_ptr(), None, None,
                             None, None) == INVALID_VALUE                        # fewer than 5 draws
    assert L.sgmcmc_psis_loo(x.data_ptr(), 1, 0, 300, 100, 300, None, None, small, pw.data_ptr(), None, None, None,
                             None) == INVALID_VALUE
    assert L.sgmcmc_psis_totals(pw.data_ptr(), 0, 0.7, pw.data_ptr(), None) == INVALID_VALUE
    assert not pw.any()                                                          # nothing was launched


@pytest.mark.gpu
def test_nan_rule_leaves_the_neighbours_untouched():
    ll, bad, clean = _nan_rule_inputs()
    got, base = _device(_cuda(ll)), _device(_cuda(clean))
    _assert_matches(got, psis_reference(ll), 30, "nan_rule")
    _assert_matches(base, psis_reference(clean), 30, "nan_rule clean")
    for f in FIELDS + ("sigma", "cut", "lw"):
        assert np.isnan(got[f][..., bad]).all(), f
        np.testing.assert_array_equal(got[f][..., ~bad], base[f][..., ~bad], err_msg=f)
    assert (got["M"][bad] == 0).all() and (got["n2"][bad] == 0).all()
    assert all(math.isnan(got["totals"][k]) for k in mc.TOTALS if k != "n_bad")
    # an r_eff that is not a positive finite number: the same rule
    re = np.ones(72)
    re[[5, 64, 70]] = [np.nan, 0.0, np.inf]
    got = _device(_cuda(clean), _cuda(re))
    for f in FIELDS:
        assert np.isnan(got[f][bad]).all(), f
        np.testing.assert_array_equal(got[f][~bad], base[f][~bad], err_msg=f)


@pytest.mark.gpu
def test_two_calls_and_shifted_slices_give_the_same_bits():
    ll, _, _ = _case("lanes_130")
    x = _cuda(ll)
    a, b = _device(x), _device(x)
    part, shifted = _device(x[:, :100]), _device(x[:, 7:107])                    # views: draw_stride 130 > N
    for f in FIELDS + ("sigma", "cut", "M", "n2", "lw"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
        np.testing.assert_array_equal(part[f], a[f][..., :100], err_msg=f)
        np.testing.assert_array_equal(shifted[f], a[f][..., 7:107], err_msg=f)
    assert a["totals"] == b["totals"]


@pytest.mark.gpu
@pytest.mark.parametrize("phi", [0.0, 0.9])
def test_relative_eff_is_the_restatements_ess_over_the_draws(phi, monkeypatch):
    ll = _ar1_ll(phi)
    ref = chain_diag_reference(np.exp(ll), split=False)
    x = _cuda(ll)
    got = _np(mc.relative_eff(x))
    np.testing.assert_allclose(got, ref.ess / 400.0, rtol=RTOL, atol=0)
    monkeypatch.setattr(mc, "EFF_CHUNK_BYTES", 8 * 400 * 16)                      # 16 observations per chunk
    np.testing.assert_array_equal(_np(mc.relative_eff(x)), got)
    # ... and as r_eff it sets the tail's length per observation
    res = _device(x.view(400, 65), _cuda(got))
    _assert_matches(res, psis_reference(ll.reshape(400, 65), got), 400, f"ar1 {phi}")


def _fit(seed, scale, n=96, E=40, width=8):
    "a classificationdensenet of width 8 with E synthetic samples (two chains of E / 2, one after the other)"
    from bnn_priors_amd import models
    torch.manual_seed(0)
    x = torch.rand(n, 784)
    y = torch.arange(n) % 10
    net = models.get_model(x, y, "classificationdensenet", width=width, depth=3, weight_prior="gaussian", weight_loc=0.,
                           weight_scale=2 ** .5, bias_prior="gaussian", bias_loc=0., bias_scale=1., batchnorm=False,
                           weight_prior_params={}, bias_prior_params={})
    models.he_initialize(net)
    net = net.to("cuda:0").eval()
    g = torch.Generator().manual_seed(seed)
    samples = {}
    for k, v in net.state_dict().items():
        if v.is_floating_point():
            noise = scale * torch.randn((E,) + tuple(v.shape), generator=g).to(v.device)
            samples[k] = (v.unsqueeze(0) + noise * v.abs().mean()).clone()
        else:
            samples[k] = v.unsqueeze(0).repeat((E,) + (1,) * v.dim())
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x.to("cuda:0"), y.to("cuda:0")), batch_size=32)
    return net, loader, samples


@pytest.mark.gpu
def test_evaluate_loo_compare_and_marglik_end_to_end():
    fits, pointwise, results = {}, {}, {}
    for name, seed, scale in (("narrow", 1, 0.05), ("wide", 2, 0.2)):
        net, loader, samples = fits[name] = _fit(seed, scale)
        lps = ev.predictive_tables(net, loader, samples)[0]
        assert lps.shape == (40, 96) and lps.dtype == torch.float64
        table = _np(lps)
        for chains in (None, 2):
            got = ev.evaluate_loo(net, loader, samples, chains=chains)
            assert set(got) == {"elpd_loo", "elpd_loo_se", "p_loo", "elpd_waic", "p_waic", "pareto_k_max",
                                "pareto_k_bad"}
            assert all(isinstance(v, float) for v in got.values())
            r_eff = None
            if chains:
                diag = chain_diag_reference(np.exp(table.reshape(2, 20, 96)), split=False)
                assert (diag.margin >= MARGIN).all()
                r_eff = diag.ess / 40.0
            ref = psis_reference(table, r_eff)
            want = totals_reference(ref, 40)
            for key, ref_key in (("elpd_loo", "elpd_loo"), ("elpd_loo_se", "se_loo"), ("p_loo", "p_loo"),
                                 ("elpd_waic", "elpd_waic"), ("p_waic", "p_waic"), ("pareto_k_max", "k_max"),
                                 ("pareto_k_bad", "n_bad")):
                np.testing.assert_allclose(got[key], want[ref_key], rtol=RTOL, atol=ATOL,
                                           err_msg=f"{name} {chains} {key}")
        results[name] = mc.loo(lps)
        pointwise[name] = psis_reference(table).elpd_loo
    rows = mc.compare(results)
    for row, (name, elpd, diff, dse) in zip(rows, compare_reference(pointwise)):
        assert row.name == name
        np.testing.assert_allclose([row.elpd, row.elpd_diff, row.dse], [elpd, diff, dse], rtol=RTOL, atol=ATOL)
    assert rows[0].elpd_diff == 0.0 and rows[1].elpd_diff < 0.0 and rows[1].dse > 0.0
    # the reference's marginal-likelihood numbers: the model's own log_prior() per sample
    net, loader, samples = fits["narrow"]
    eval_samples = {k: v + 0.01 for k, v in list(samples.items())[:2]}
    got = ev.evaluate_marglik(net, samples, eval_samples)
    log_priors = []
    for e in range(40):
        net.load_state_dict({k: eval_samples.get(k, v)[e] for k, v in samples.items()})
        log_priors.append(net.log_prior().item())
    lp = torch.tensor(log_priors)
    assert got == {"simple_logmarglik": lp.logsumexp(0).item() - math.log(40), "mean_loglik": lp.mean().item(),
                   "simple_marglik": lp.exp().mean().item()}
