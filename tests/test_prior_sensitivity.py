"""Power-scaling sensitivity (bnn_priors_amd/prior_sensitivity.py, csrc/powerscale_hip.inc) against the definition in
include/sgmcmc_hip.h as tests/powerscale_reference.py restates it.

CPU: the restatement against independent sources -- a two-point closed form, mpmath at 50 digits for g, math.fsum for
the weighted mean, np.lexsort for the keyed sort, and a conjugate normal model whose exact power-scaled posterior is
known (plain self-normalised weights there: PSIS exists on the device only).

GPU: the device against the restatement, part by part.  The restatement receives the weights that the kernel read
(``parts=True``), so every operation but log1p is the same singly rounded operation in the same order:

* ``sorted`` and ``order``: selections under a total order -- identical (``order`` is compared on every column without a
  non-finite draw, where the definition fixes it, and is inside [0, N) on the others);
* ``wmean`` and ``wsd``: bit-equal, every quantity of every case;
* ``dist`` where every |delta| of the result is below 1/4 (the restatement reports it): bit-equal.  The cases named in
  ``SERIES_ONLY`` have no other quantities (asserted);
* ``dist`` where a delta takes the log1p form: numpy's log1p was measured against mpmath at 50 digits on those cases' own
  arguments (-delta and delta of every term of the ``LOG1P_CASES`` that takes the form, 8,854 arguments, on the CPU:
  ``test_log1p_tolerance_is_eighty_times_numpys_measured_distance``): 1.109e-16 relative at worst, recorded as
  NUMPY_LOG1P_DISTANCE = 1.11e-16.  The device gets ten times that (the AB_RTOL precedent of tests/test_posterior_summary.py),
  times 8 for g's worst amplification of a relative error of its two products, (|t1| + |t2|) / g = 7.8 at
  |delta| = 1/4: DIST_RTOL = 80 * 1.11e-16 = 8.88e-15, relative, on dist (whose square root halves what the sum
  carries; that half is left to the roundings of the sum's additions after a term that differs).  Measured on the
  MI355X: the device's dist is within 2.22e-16 of the restatement's in the four LOG1P_CASES (0 in two of them).
No quantity is left out of any comparison."""
import functools
import math

import numpy as np
import pytest
import torch

import powerscale_reference as ref

NUMPY_LOG1P_DISTANCE = 1.11e-16              # measured: see the module docstring
DIST_RTOL = 80 * NUMPY_LOG1P_DISTANCE
EPS = 2.0 ** -53
INVALID_VALUE = 1                            # hipErrorInvalidValue

# (M, S) of the draw counts: N = 5, 8, 9, 1023, 1024, 1025, 8192
GEOMETRY = {"n5": (1, 5), "n8": (2, 4), "n9": (3, 3), "n1023": (3, 341), "n1024": (4, 256), "n1025": (5, 205),
            "n8192": (8, 1024)}
# ... and the quantity counts around the sort's tile width TQ at three of them: TQ = 64, 8, 1
TILE_GEOMETRY = {"n8": 64, "n1024": 8, "n8192": 1}
NEAR_ONE = {1: (1.01,), 2: (1.0 / 1.01, 1.01), 5: (0.98, 0.99, 1.0, 1.01, 1.02)}        # A = 1, 2, 5: every delta small
FAR = (0.25, 4.0)                                                                        # ... and weights far from uniform


def _iid(seed, M, S, Q):
    return np.random.default_rng(seed).standard_normal((M, S, Q))


def _halves(seed, M, S, Q):
    "draws rounded to halves: tied order statistics, and -0.0 next to 0.0"
    return np.round(_iid(seed, M, S, Q) * 2.0) / 2.0


def _log_weights(x, alphas, width=1.0):
    """normalised log weights [N, A] of the powers ``alphas`` of a component that depends on the first and the last
    quantity's draws, log p = -clip(width x_0, -4, 4)^2 / 2 + clip(x_last, -5, 5) / 4 (so the weighted distribution of
    those columns does move, and log p spans at most 10.5)"""
    flat = x.reshape(-1, x.shape[-1]).astype(np.float64)
    lc = -0.5 * np.square(np.clip(width * np.nan_to_num(flat[:, 0], nan=0.3), -4.0, 4.0))
    lc = lc + 0.25 * np.clip(np.nan_to_num(flat[:, -1], nan=0.1), -5.0, 5.0)
    r = ref.ratios(lc, alphas)
    r = r - r.max(axis=0)
    return r - np.log(np.exp(r).sum(axis=0))


def _tile_counts(tq):
    return sorted({q for q in (1, tq - 1, tq, tq + 1, 2 * tq + 3) if q >= 1})


def _nan_rule_draws():
    x = _iid(11, 2, 20, 72)
    x[1, 13, 5] = np.inf
    x[:, :, 7] = 2.0                         # constant
    x[:, :, 9] = 0.1                         # constant, and the weighted sum of its copies is not a multiple of it
    x[0, 3, 66] = np.nan
    return x


def _zero_weights(x):
    lw = _log_weights(x, FAR)
    lw[::3, 0] = -np.inf                     # exact zeros, among them the smallest draws of some columns: delta = -1
    lw[:x.shape[1], 1] = -np.inf             # the whole first chain
    return lw


def _nan_weights(x):
    lw = _log_weights(x, NEAR_ONE[5])
    lw[7, 1] = np.nan
    lw[3, 3] = np.inf
    return lw


CASES = {}
for _i, (_name, (_M, _S)) in enumerate(GEOMETRY.items()):
    _A = (1, 2, 5)[_i % 3]
    CASES[_name] = (lambda M=_M, S=_S, A=_A, i=_i: (lambda x: (x, _log_weights(x, NEAR_ONE[A])))(
        _iid(i, M, S, 3 if M * S == 8192 else 5)))
for _name, _tq in TILE_GEOMETRY.items():
    _M, _S = GEOMETRY[_name]
    for _Q in _tile_counts(_tq):
        CASES[f"{_name}_q{_Q}"] = (lambda M=_M, S=_S, Q=_Q: (lambda x: (x, _log_weights(x, NEAR_ONE[2])))(
            _iid(100 + Q, M, S, Q)))
CASES.update({
    "ties": lambda: (lambda x: (x, _log_weights(x, NEAR_ONE[5])))(_halves(1, 3, 40, 65)),
    "cauchy": lambda: (lambda x: (x, _log_weights(x, NEAR_ONE[2])))(
        np.random.default_rng(2).standard_cauchy((4, 50, 65))),
    "nan_rule": lambda: (lambda x: (x, _log_weights(x, NEAR_ONE[2])))(_nan_rule_draws()),
    "nan_weights": lambda: (lambda x: (x, _nan_weights(x)))(_iid(3, 2, 20, 9)),
    "far_n9": lambda: (lambda x: (x, _log_weights(x, FAR, width=3.0)))(_iid(4, 3, 3, 70)),
    "far_n1025": lambda: (lambda x: (x, _log_weights(x, FAR, width=3.0)))(_iid(5, 5, 205, 9)),
    "far_ties": lambda: (lambda x: (x, _log_weights(x, FAR, width=3.0)))(_halves(6, 3, 40, 65)),
    "zero_weights": lambda: (lambda x: (x, _zero_weights(x)))(_iid(7, 3, 40, 9)),
})
LOG1P_CASES = ("far_n9", "far_n1025", "far_ties", "zero_weights")
SERIES_ONLY = tuple(n for n in CASES if n not in LOG1P_CASES)
F32_CASES = ("ties", "n1025")


@functools.lru_cache(maxsize=None)
def _case(name, f32=False):
    "(x [M, S, Q], log weights [N, A]), computed once and shared; f32: the draws rounded to fp32"
    x, lw = CASES[name]()
    if f32:
        x = x.astype(np.float32)
    x.setflags(write=False)
    lw.setflags(write=False)
    return x, lw


def _same_bits(a, b):
    "equal to the bit, a NaN matching any NaN"
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- CPU: the restatement against independent sources -----------------------------------------------------------------

def test_two_draws_closed_form():
    for p in (0.3, 0.5, 0.05, 0.999):
        m = (0.5 + p) / 2.0
        want = math.sqrt((0.5 * math.log2(0.5 / m) + p * math.log2(p / m)) / (0.5 + p))
        got = ref.distance_of_draws(np.array([[0.0], [1.0]]), np.array([[p], [1.0 - p]]))
        assert got.dist[0, 0] == pytest.approx(want, rel=1e-13, abs=1e-9 if p == 0.5 else 0)
        assert got.wmean[0, 0] == pytest.approx(1.0 - p, rel=1e-15)
        assert got.wsd[0, 0] == pytest.approx(math.sqrt(p * (1.0 - p)), rel=1e-14)
    assert ref.distance_of_draws(np.array([[0.0], [1.0]]), np.array([[0.3], [0.7]])).dist[0, 0] == pytest.approx(
        0.2134619335503, rel=1e-12)
    # ... and the distance does not depend on the scale of the weights or of the draws, nor on the order of the draws
    a = ref.distance_of_draws(np.array([[3.0], [-1.0], [0.5]]), np.array([[0.2], [0.5], [0.3]]))
    b = ref.distance_of_draws(np.array([[-10.0], [5.0], [30.0]]), np.array([[5.0], [3.0], [2.0]]))
    assert a.dist[0, 0] == pytest.approx(b.dist[0, 0], rel=1e-14)


def test_g_series_and_log1p_form_against_mpmath():
    deltas = np.concatenate([np.logspace(-8, np.log10(0.25), 60, endpoint=False), np.linspace(0.25, 1.0, 61),
                             [0.2499999999, np.nextafter(0.25, 0), 0.25, np.nextafter(0.25, 1), 0.2500000001]])
    deltas = np.concatenate([deltas, -deltas])
    got, small = ref.g(deltas)
    assert small.sum() == 2 * 62 and (small == (np.abs(deltas) < 0.25)).all()
    worst = {True: 0.0, False: 0.0}
    for d, v, s in zip(deltas, got, small):
        want = ref.g_exact(float(d))
        worst[bool(s)] = max(worst[bool(s)], abs(float((v - want) / want)))
    print(f"g against mpmath: series {worst[True]:.2e}, log1p form {worst[False]:.2e} relative")
    # the series: 17 roundings of a Horner chain of positive terms, and a remainder below (1/16)^17 / (17 * 33 * 15/16)
    assert worst[True] <= 20 * 2.0 ** -53
    # the log1p form: two products of a correctly rounded factor and log1p (an ulp), amplified by at most 7.8
    assert worst[False] <= 8 * 4 * 2.0 ** -53
    assert got[deltas == 1.0][0] == got[deltas == -1.0][0] == ref.TWO_LN2 == 2.0 * math.log(2.0)
    # both forms at the crossover: within the sum of the two bounds above of one another (measured: 4.4e-16)
    d = np.array([0.25, -0.25, np.nextafter(0.25, 0)])
    assert np.max(np.abs(ref.g_series(d) / ref.g_log1p(d) - 1.0)) <= (20 + 32) * 2.0 ** -53
    assert ref.COEFFS[0] == 1.0 and ref.COEFFS[15] == 1.0 / 496.0 and len(ref.COEFFS) == 16


def test_uniform_weights_give_no_distance():
    for N in (5, 9, 1000, 1025):
        x = _iid(N, 1, N, 4).reshape(N, 4)
        got = ref.distance_of_draws(x, np.stack([np.full(N, 1.0 / N), np.full(N, 3.0)], axis=1))
        assert (got.dist < 1e-10).all() and got.series.all()
        np.testing.assert_allclose(got.wmean, np.broadcast_to(x.mean(0), (2, 4)), rtol=0, atol=1e-13)
        np.testing.assert_allclose(got.wsd, np.broadcast_to(x.std(0), (2, 4)), rtol=1e-12)


def test_weighted_moments_against_fsum():
    for name in ("n9", "n1023", "cauchy", "far_n1025", "zero_weights"):
        x, lw = _case(name)
        flat, w = x.reshape(-1, x.shape[-1]), np.exp(lw)
        N = len(flat)
        got = ref.distance_of_draws(flat, w)
        for a in range(w.shape[1]):
            W = math.fsum(w[:, a])
            for q in range(0, flat.shape[1], 3):
                mean = math.fsum(w[:, a] * flat[:, q]) / W
                bound = N * 2.0 ** -53 * math.fsum(w[:, a] * np.abs(flat[:, q])) / W
                assert abs(got.wmean[a, q] - mean) <= bound, (name, a, q)
                var = math.fsum(w[:, a] * (flat[:, q] - mean) ** 2) / W
                assert got.wsd[a, q] == pytest.approx(math.sqrt(var), rel=N * 2.0 ** -52), (name, a, q)


def test_keyed_sort_against_lexsort():
    for name in ("ties", "nan_rule", "n8_q131", "n1025"):
        x, _ = _case(name)
        flat = x.reshape(-1, x.shape[-1])
        N, Q = flat.shape
        ordered, order, bad = ref.keyed_sort(flat)
        assert (bad == ~np.isfinite(flat).all(axis=0)).all()
        for q in range(Q):
            if bad[q]:
                assert np.isnan(ordered[:, q]).all() and (order[:, q] == np.arange(N)).all()
                continue
            want = np.lexsort((np.arange(N), flat[:, q]))
            assert (order[:, q] == want).all()
            assert _same_bits(ordered[:, q], flat[want, q] + 0.0) and not np.signbit(ordered[:, q][ordered[:, q] == 0]).any()
    assert np.signbit(_case("ties")[0]).any() and (_case("ties")[0] == 0).any()
    assert [ref.tile_quantities(N) for N in (4, 5, 8, 9, 128, 129, 1024, 1025, 4096, 4097, 8192, 8193)] == \
        [0, 64, 64, 64, 64, 32, 8, 4, 2, 1, 1, 0]


# tau, ybar, n -> the prototype's psi(prior), psi(likelihood) and the diagnosis
CONJUGATE = (((10.0, 0.5, 20), (0.00015, 0.086), 0), ((0.5, 3.0, 5), (0.335, 0.389), 1), ((0.3, 0.1, 1), (0.075, 0.0098), 2))


def test_conjugate_normal_model_reads_as_the_table_says():
    """theta ~ N(0, tau^2), n observations of unit variance with mean ybar: the posterior is N(n ybar / prec, 1 / prec),
    prec = 1 / tau^2 + n, and with the prior raised to alpha it is the same with 1 / tau^2 scaled by alpha."""
    rng = np.random.default_rng(0)
    alpha, S = 1.01, 4000
    for (tau, ybar, n), (psi_prior, psi_lik), code in CONJUGATE:
        prec = 1.0 / tau ** 2 + n
        theta = n * ybar / prec + rng.standard_normal(S) / math.sqrt(prec)
        comps = {"prior": -0.5 * theta ** 2 / tau ** 2, "likelihood": -0.5 * n * (theta - ybar) ** 2}
        psi, grad = {}, {}
        for name, lc in comps.items():
            r = ref.ratios(lc, (1.0 / alpha, alpha))
            d = ref.distance_of_draws(theta[:, None], np.exp(r - r.max(axis=0)))
            assert d.series.all()
            lo, hi = ((d.dist[a, 0], d.wmean[a, 0], d.wsd[a, 0]) for a in range(2))
            psi[name], grad[name], _ = ref.sensitivity(lo, hi, alpha)
            if name == "prior":
                for a, power in enumerate((1.0 / alpha, alpha)):
                    scaled = power / tau ** 2 + n
                    mc_se = 1.0 / math.sqrt(prec * S)             # of the plain mean; the weights are nearly uniform
                    assert abs(d.wmean[a, 0] - n * ybar / scaled) <= 3 * mc_se
        print((tau, ybar, n), psi)
        assert psi["prior"] == pytest.approx(psi_prior, rel=0.05) and psi["likelihood"] == pytest.approx(psi_lik, rel=0.05)
        got = ref.diagnosis(np.array([psi["prior"]]), np.array([psi["likelihood"]]), 0.05)
        assert got.dtype == np.int8 and got[0] == code


def _log1p_arguments():
    args = []
    for name in LOG1P_CASES:
        for f32 in (False,) + ((True,) if name in F32_CASES else ()):
            x, lw = _case(name, f32)
            got = ref.distance_of_draws(x.reshape(-1, x.shape[-1]).astype(np.float64), np.exp(lw), keep_args=True)
            assert not got.series.all() and len(got.log1p_args), name
            args.append(got.log1p_args)
    deltas = np.concatenate(args)
    return np.concatenate([deltas, -deltas])


def test_log1p_tolerance_is_eighty_times_numpys_measured_distance():
    args = _log1p_arguments()
    assert (np.abs(args) >= 0.25).all() and (np.abs(args) <= 1.0).all()
    worst = ref.log1p_distance(args)
    print(f"numpy's log1p against mpmath over {len(args)} arguments: {worst:.3e} relative")
    assert worst <= NUMPY_LOG1P_DISTANCE and DIST_RTOL == 80 * NUMPY_LOG1P_DISTANCE
    # g's amplification of a relative error of its two products is largest at the crossover
    for d in (0.25, 0.5, 0.9, 1.0):
        t1 = 0.0 if d >= 1 else (1 - d) * math.log1p(-d)
        t2 = (1 + d) * math.log1p(d)
        assert (abs(t1) + abs(t2)) / (t1 + t2) <= (7.9 if d == 0.25 else 7.8)


def test_series_only_cases_have_no_log1p_term():
    for name in SERIES_ONLY:
        if name.startswith("n8192_"):
            continue                         # the other quantity counts at 8,192 draws: n8192's construction
        x, lw = _case(name)
        got = ref.distance_of_draws(x.reshape(-1, x.shape[-1]), np.exp(lw))
        assert got.series.all() and np.nanmax(got.max_delta) < 0.25, name


def test_argument_checks_raise_before_the_library_is_touched(monkeypatch):
    from bnn_priors_amd import _hip
    from bnn_priors_amd import prior_sensitivity as ps

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_hip, "lib", no_library)
    x = torch.zeros(2, 5, 3, dtype=torch.float64)
    lw = torch.zeros(10, 2, dtype=torch.float64)
    lc = torch.zeros(10, dtype=torch.float64)
    bad = [
        (lambda: ps.weighted_distance(x, lw), "CUDA"),
        (lambda: ps.weighted_distance(x.numpy(), lw), "tensor"),
        (lambda: ps.weighted_distance(x.half(), lw), "float32 or float64"),
        (lambda: ps.weighted_distance(x[0, 0], lw), r"\[chains, draws"),
        (lambda: ps.weighted_distance(x[:, :2], lw), "4 draws"),
        (lambda: ps.weighted_distance(torch.zeros(1, 8193, 1), lw), "8193 draws"),
        (lambda: ps.weighted_distance(x, lw.float()), "float64 tensor of shape"),
        (lambda: ps.weighted_distance(x, lw[:9]), "float64 tensor of shape"),
        (lambda: ps.weighted_distance(x, lw[:, :0]), "weight vectors"),
        (lambda: ps.weighted_distance(x, lw, workspace_bytes=64 * 10 * 10 - 1), "too small"),
        (lambda: ps.weighted_distance(x, lw, workspace_bytes=None), "integer"),
        (lambda: ps.power_scale_weights(lc, (1.01,)), "CUDA"),
        (lambda: ps.power_scale_weights(lc.float(), (1.01,)), "float64"),
        (lambda: ps.power_scale_weights(lc.reshape(1, 2, 5), (1.01,)), "draws"),
        (lambda: ps.power_scale_weights(lc[:4], (1.01,)), "4 draws"),
        (lambda: ps.power_scale_weights(lc, ()), "positive"),
        (lambda: ps.power_scale_weights(lc, (1.01, 0.0)), "positive"),
        (lambda: ps.power_scale_weights(lc, (-2.0,)), "positive"),
        (lambda: ps.power_scale_weights(lc, (float("inf"),)), "positive"),
        (lambda: ps.power_scale_weights(lc, 1.01), "sequence"),
        (lambda: ps.power_scale_sensitivity(x, {"prior": lc}), "CUDA"),
        (lambda: ps.power_scale_sensitivity(x, {"prior": lc}, alpha=1.0), "differ from 1"),
        (lambda: ps.power_scale_sensitivity(x, {"prior": lc}, alpha=-1.0), "positive"),
        (lambda: ps.power_scale_sensitivity(x, {"prior": lc}, threshold=0.0), "threshold"),
        (lambda: ps.power_scale_sensitivity(x, {}), "non-empty dict"),
        (lambda: ps.power_scale_sensitivity(x, lc), "non-empty dict"),
        (lambda: ps.power_scale_sensitivity(x, {"prior": lc[:9]}), "holds 9 draws"),
        (lambda: ps.power_scale_sensitivity(x, {"prior": lc.float()}), "float64"),
        (lambda: ps.power_scale_sequence(x, lc, (0.9, 1.1)), "CUDA"),
        (lambda: ps.power_scale_sequence(x, lc, (0.9, 0.0)), "positive"),
        (lambda: ps.power_scale_sequence(x, lc[:7], (0.9,)), "holds 7 draws"),
        (lambda: ps.sort_tile(4), "outside"),
    ]
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
    assert [ps.sort_tile(N) for N in (5, 128, 129, 1024, 8192)] == [ref.tile_quantities(N) for N in (5, 128, 129, 1024, 8192)]
    assert (ps.MIN_DRAWS, ps.MAX_DRAWS, ps.TILE_CELLS) == (ref.MIN_DRAWS, ref.MAX_DRAWS, ref.TILE_CELLS)


def test_header_constants_and_table_agree():
    import os
    import re
    from bnn_priors_amd import _hip
    with open(os.path.join(_hip.INCLUDE_DIR, "sgmcmc_hip.h")) as f:
        header = f.read()
    values = dict(re.findall(r"#define SGMCMC_POWERSCALE_(\w+) ([0-9.]+)", header))
    assert int(values["MAX_DRAWS"]) == _hip.POWERSCALE_MAX_DRAWS == ref.MAX_DRAWS
    assert int(values["TILE_CELLS"]) == _hip.POWERSCALE_TILE_CELLS == ref.TILE_CELLS
    assert float(values["TWO_LN2"]) == ref.TWO_LN2
    for name in ("sgmcmc_powerscale_tile_quantities", "sgmcmc_powerscale_sort", "sgmcmc_powerscale_distance"):
        assert name in _hip.EXPORTS and re.search(rf"^int {name}\(", header, re.M)
    assert _hip.ABI_VERSION >= 28


# ---- GPU: the device against the restatement ----------------------------------------------------------------------------

def _cuda(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")          # a writable copy


def _np(t):
    return t.detach().cpu().numpy()


def _assert_matches(x, got, what):
    "a ``WeightedDistanceParts`` of the draws x [M, S, Q] against the restatement fed with the weights the kernel read"
    flat = x.reshape(-1, x.shape[-1]).astype(np.float64)
    N, Q = flat.shape
    ordered, order, bad = ref.keyed_sort(flat)
    assert _same_bits(_np(got.sorted), ordered), (what, "sorted")
    have = _np(got.order).astype(np.int64)
    assert (have[:, ~bad] == order[:, ~bad]).all(), (what, "order")
    assert ((have >= 0) & (have < N)).all(), (what, "order in range")
    want = ref.distance(_np(got.sorted), have, _np(got.weights))
    A = got.weights.shape[1]
    dist, mean, sd = (_np(t).reshape(A, Q) for t in (got.dist, got.mean, got.sd))
    assert _same_bits(mean, want.wmean), (what, "wmean")
    assert _same_bits(sd, want.wsd), (what, "wsd")
    assert (np.isnan(dist) == np.isnan(want.dist)).all(), (what, "dist NaN")
    fixed = want.series | np.isnan(want.dist)
    assert _same_bits(np.where(fixed, dist, 0.0), np.where(fixed, want.dist, 0.0)), (what, "dist, series only")
    worst = float(np.max(np.abs(dist[~fixed] / want.dist[~fixed] - 1.0), initial=0.0))
    print(f"{what}: {(~fixed).sum()} of {fixed.size} distances with log1p terms, {worst:.2e} relative (allowed "
          f"{DIST_RTOL:.2e}); max |delta| {np.nanmax(want.max_delta):.3g}")
    assert worst <= DIST_RTOL, (what, worst)
    live = ~np.isnan(want.dist)
    assert ((dist[live] >= 0.0) & (dist[live] <= 1.0)).all(), (what, "dist in [0, 1]")
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_against_restatement(name):
    from bnn_priors_amd import prior_sensitivity as ps
    x, lw = _case(name)
    got = ps.weighted_distance(_cuda(x), _cuda(lw), parts=True)
    assert isinstance(got, ps.WeightedDistanceParts) and got.dist.shape == (lw.shape[1], x.shape[-1])
    want = _assert_matches(x, got, name)
    assert want.series.all() == (name in SERIES_ONLY)
    again = ps.weighted_distance(_cuda(x), _cuda(lw))
    assert all(_same_bits(_np(a), _np(b)) for a, b in zip(again, got[:3]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", F32_CASES)
def test_device_against_restatement_fp32_draws(name):
    from bnn_priors_amd import prior_sensitivity as ps
    x, lw = _case(name, True)
    assert x.dtype == np.float32
    _assert_matches(x, ps.weighted_distance(_cuda(x), _cuda(lw), parts=True), f"{name} fp32")


@pytest.mark.gpu
def test_nan_constant_and_weight_rules():
    from bnn_priors_amd import prior_sensitivity as ps
    x, lw = _case("nan_rule")
    got = ps.weighted_distance(_cuda(x), _cuda(lw))
    dist, mean, sd = (_np(t) for t in got)
    for q in (5, 66):                                                             # an inf, a NaN
        assert np.isnan(dist[:, q]).all() and np.isnan(mean[:, q]).all() and np.isnan(sd[:, q]).all()
    for q, value in ((7, 2.0), (9, 0.1)):                                         # constant columns
        assert (dist[:, q] == 0).all() and (mean[:, q] == value).all() and (sd[:, q] == 0).all()
    rest = np.setdiff1d(np.arange(72), (5, 7, 9, 66))
    assert np.isfinite(dist[:, rest]).all() and (dist[:, rest] > 0).all() and (sd[:, rest] > 0).all()
    x, lw = _case("nan_weights")
    dist, mean, sd = (_np(t) for t in ps.weighted_distance(_cuda(x), _cuda(lw)))
    for t in (dist, mean, sd):
        assert np.isnan(t[[1, 3]]).all() and np.isfinite(t[[0, 2, 4]]).all()      # a NaN weight, an infinite weight
    assert (dist[2] < 1e-10).all()                                                # alpha = 1: uniform weights
    x, lw = _case("zero_weights")
    none = np.full_like(lw, -np.inf)                                              # W = 0
    assert all(np.isnan(_np(t)).all() for t in ps.weighted_distance(_cuda(x), _cuda(none)))


@pytest.mark.gpu
def test_strided_views_and_workspaces_change_no_bit():
    from bnn_priors_amd import prior_sensitivity as ps
    x, lw = _case("n8_q131")
    M, S, Q = x.shape
    want = ps.weighted_distance(_cuda(x), _cuda(lw), parts=True)
    big = torch.full((M, S + 3, Q + 5), float("nan"), dtype=torch.float64, device="cuda:0")
    view = big[:, 1:S + 1, 2:Q + 2]
    view.copy_(_cuda(x))
    assert view.stride(0) != S * view.stride(1) and view.stride(1) != Q and not view.is_contiguous()
    shaped = _cuda(x).reshape(M, S, Q, 1)
    for other in (ps.weighted_distance(view, _cuda(lw), parts=True),
                  ps.weighted_distance(_cuda(x), _cuda(lw), workspace_bytes=64 * 10 * M * S, parts=True),
                  ps.weighted_distance(_cuda(x), _cuda(lw), workspace_bytes=128 * 10 * M * S + 7, parts=True)):
        assert all(_same_bits(_np(a), _np(b)) for a, b in zip(other[:4], want[:4]))
        assert torch.equal(other.order, want.order)
    assert ps.weighted_distance(shaped, _cuda(lw)).dist.shape == (lw.shape[1], Q, 1)
    # a quantity's result does not depend on which other quantities or weight vectors are in the call
    part = ps.weighted_distance(_cuda(x[:, :, 60:70]), _cuda(lw[:, 1:]))
    assert all(_same_bits(_np(a), _np(b)[1:, 60:70]) for a, b in zip(part, want[:3]))
    empty = ps.weighted_distance(_cuda(x)[:, :, :0], _cuda(lw))
    assert empty.dist.shape == (lw.shape[1], 0)


@pytest.mark.gpu
def test_c_abi_refuses_bad_shapes():
    from bnn_priors_amd import _hip, prior_sensitivity as ps
    L = _hip.lib()
    assert [L.sgmcmc_powerscale_tile_quantities(N) for N in (4, 5, 8, 9, 128, 129, 1024, 1025, 8192, 8193)] == \
        [ref.tile_quantities(N) for N in (4, 5, 8, 9, 128, 129, 1024, 1025, 8192, 8193)]
    x = torch.zeros(2, 8, 4, dtype=torch.float64, device="cuda:0")
    vals = torch.full((16, 4), 7.0, dtype=torch.float64, device="cuda:0")
    idx = torch.full((16, 4), 7, dtype=torch.int16, device="cuda:0")
    w = torch.ones(16, 2, dtype=torch.float64, device="cuda:0")
    out = torch.full((3, 2, 4), 7.0, dtype=torch.float64, device="cuda:0")
    X, V, I, Wp = x.data_ptr(), vals.data_ptr(), idx.data_ptr(), w.data_ptr()
    D, Mn, Sd = (out[r].data_ptr() for r in range(3))
    sort_calls = [(None, 1, 32, 4, 2, 8, 4, V, I), (X, 1, 32, 4, 2, 8, 4, None, I), (X, 1, 32, 4, 2, 8, 4, V, None),
                  (X, 1, 32, 4, 0, 8, 4, V, I), (X, 1, 32, 4, 2, 0, 4, V, I), (X, 1, 32, 4, 2, 8, 0, V, I),
                  (X, 1, 32, 4, 1, 4, 4, V, I), (X, 1, 32, 4, 8193, 1, 4, V, I), (X, 1, 32, 4, 65536, 65536, 4, V, I),
                  (X, 1, -32, 4, 2, 8, 4, V, I), (X, 1, 32, -4, 2, 8, 4, V, I)]
    for args in sort_calls:
        assert L.sgmcmc_powerscale_sort(*args, None) == INVALID_VALUE, args
    dist_calls = [(None, I, 16, 4, Wp, 2, 4, D, Mn, Sd), (V, None, 16, 4, Wp, 2, 4, D, Mn, Sd),
                  (V, I, 16, 4, None, 2, 4, D, Mn, Sd), (V, I, 16, 4, Wp, 2, 4, None, Mn, Sd),
                  (V, I, 16, 4, Wp, 2, 4, D, None, Sd), (V, I, 16, 4, Wp, 2, 4, D, Mn, None),
                  (V, I, 4, 4, Wp, 2, 4, D, Mn, Sd), (V, I, 8193, 4, Wp, 2, 4, D, Mn, Sd), (V, I, 16, 0, Wp, 2, 4, D, Mn, Sd),
                  (V, I, 16, 4, Wp, 0, 4, D, Mn, Sd), (V, I, 16, 4, Wp, 65536, 4, D, Mn, Sd), (V, I, 16, 4, Wp, 2, 3, D, Mn, Sd)]
    for args in dist_calls:
        assert L.sgmcmc_powerscale_distance(*args, None) == INVALID_VALUE, args
    torch.cuda.synchronize()
    assert (vals == 7).all() and (idx == 7).all() and (out == 7).all()               # nothing was launched
    assert ps.MAX_VECTORS == 65535


def _component(seed, N, width=1.0):
    z = np.random.default_rng(seed).standard_normal(N)
    return -0.5 * np.square(width * z) - 3.0


@pytest.mark.gpu
def test_power_scale_weights_are_psis_of_the_ratios():
    from bnn_priors_amd import model_comparison as mc, prior_sensitivity as ps
    N, alphas = 1200, (0.5, 1.0 / 1.01, 1.0, 1.01, 2.0)
    lc = _cuda(_component(0, N, 2.0))
    got = ps.power_scale_weights(lc.view(4, 300), alphas)
    assert isinstance(got, ps.PowerScaleWeights) and got.log_weights.shape == (N, 5)
    assert _same_bits(_np(ps.power_scale_weights(lc, alphas).log_weights), _np(got.log_weights))
    ratios = _cuda(ref.ratios(_np(lc), alphas))
    assert _same_bits(_np(lc.reshape(-1, 1) * _cuda(np.array([a - 1.0 for a in alphas]))), _np(ratios))
    lw, k = mc.psis(ratios)
    assert _same_bits(_np(got.log_weights), _np(lw)) and _same_bits(_np(got.pareto_k), _np(k))
    w = np.exp(_np(lw))
    np.testing.assert_allclose(_np(got.ess), 1.0 / np.square(w).sum(axis=0), rtol=N * 2.0 ** -52)
    ess = _np(got.ess)
    assert ess[2] == pytest.approx(N, rel=1e-12) and np.isinf(_np(got.pareto_k)[2])          # alpha = 1: uniform
    assert (ess[[0, 4]] < ess[[1, 3]]).all() and (ess <= N * (1 + 1e-12)).all()
    np.testing.assert_allclose(w.sum(axis=0), 1.0, rtol=1e-12)
    bad = lc.clone()
    bad[17] = float("nan")
    assert np.isnan(_np(ps.power_scale_weights(bad, (1.01,)).log_weights)).all()


def _sensitivity_inputs():
    rng = np.random.default_rng(12)
    M, S, Q = 4, 300, 70
    theta = rng.standard_normal((M, S, 1))
    x = theta * rng.uniform(-1, 1, Q) + 0.5 * rng.standard_normal((M, S, Q))
    x[..., 0] = theta[..., 0]                # the parameter itself
    x[..., 1] = 2.5                          # a constant quantity
    comps = {"prior": -2.0 * np.square(theta[..., 0]), "likelihood": -1.5 * np.square(theta[..., 0] - 0.4),
             "prior:scale": rng.standard_normal((M, S))}
    return x, comps


@pytest.mark.gpu
def test_power_scale_sensitivity_against_the_restatement():
    from bnn_priors_amd import prior_sensitivity as ps
    x, comps = _sensitivity_inputs()
    M, S, Q = x.shape
    alpha, threshold = 1.01, 0.05
    dev = {n: _cuda(v) for n, v in comps.items()}
    got = ps.power_scale_sensitivity(_cuda(x), dev, alpha, threshold)
    assert isinstance(got, ps.PowerScaleSensitivity) and list(got.components) == list(comps)
    assert (got.alpha, got.threshold) == (alpha, threshold)
    ordered, order, _ = ref.keyed_sort(x.reshape(M * S, Q))
    psi = {}
    for name in comps:
        weights = ps.power_scale_weights(dev[name], (1.0 / alpha, alpha))
        d = ref.distance(ordered, order, _np(torch.exp(weights.log_weights)))         # the weights the kernel reads
        assert d.series.all()
        lo, hi = ((d.dist[a], d.wmean[a], d.wsd[a]) for a in range(2))
        want = ref.sensitivity(lo, hi, alpha)
        c = got.components[name]
        psi[name] = want[0]
        for have, ref_value, what in zip((c.psi, c.mean_gradient, c.sd_gradient), want, ("psi", "mean", "sd")):
            assert have.shape == (Q,) and _same_bits(_np(have), ref_value), (name, what)
        assert _same_bits(_np(c.pareto_k), _np(weights.pareto_k)) and _same_bits(_np(c.ess), _np(weights.ess))
        assert c.psi[1] == 0 and c.mean_gradient[1] == 0 and c.sd_gradient[1] == 0           # the constant quantity
    want = ref.diagnosis(psi["prior"], psi["likelihood"], threshold)
    assert got.diagnosis.dtype == torch.int8 and (_np(got.diagnosis) == want).all()
    assert want[0] == ps.CONFLICT and psi["prior:scale"].max() < threshold < psi["prior"][0]
    assert len(set(want.tolist())) >= 2
    # the codes follow the threshold: a strong prior reads as such once the likelihood's psi is below it
    high = ps.power_scale_sensitivity(_cuda(x), dev, alpha, float(psi["likelihood"][0]) * 1.01)
    assert int(high.diagnosis[0]) == (ps.STRONG_PRIOR if psi["prior"][0] >= psi["likelihood"][0] * 1.01 else ps.NONE)
    alone = ps.power_scale_sensitivity(_cuda(x).float().double(), {"likelihood": dev["likelihood"]}, alpha)
    assert alone.diagnosis is None and list(alone.components) == ["likelihood"]
    f32 = ps.power_scale_sensitivity(_cuda(x.astype(np.float32)), {"likelihood": dev["likelihood"]}, alpha)
    assert _same_bits(_np(f32.components["likelihood"].psi), _np(alone.components["likelihood"].psi))
    shaped = ps.power_scale_sensitivity(_cuda(x).reshape(M, S, 7, 10), dev, alpha)
    assert shaped.diagnosis.shape == (7, 10) and _same_bits(_np(shaped.components["prior"].psi).reshape(Q), psi["prior"])


@pytest.mark.gpu
def test_power_scale_sequence_against_the_restatement():
    from bnn_priors_amd import prior_sensitivity as ps
    x, comps = _sensitivity_inputs()
    M, S, Q = x.shape
    alphas = (0.99, 0.995, 0.999, 1.0, 1.001, 1.005, 1.01)
    lc = _cuda(comps["prior"])
    got = ps.power_scale_sequence(_cuda(x), lc, alphas)
    assert isinstance(got, ps.PowerScaleSequence) and got.alphas == alphas and got.dist.shape == (7, Q)
    weights = ps.power_scale_weights(lc, alphas)
    assert _same_bits(_np(got.pareto_k), _np(weights.pareto_k)) and _same_bits(_np(got.ess), _np(weights.ess))
    parts = ps.weighted_distance(_cuda(x), weights.log_weights, parts=True)
    assert _assert_matches(x, parts, "sequence").series.all()
    assert all(_same_bits(_np(a), _np(b)) for a, b in zip((got.dist, got.mean, got.sd), parts[:3]))
    dist = _np(got.dist)[:, 0]
    assert dist[3] < 1e-10 and (np.diff(dist[:4]) < 0).all() and (np.diff(dist[3:]) > 0).all()
    assert (np.diff(_np(got.sd)[:, 0]) < 0).all()    # a prior centred at 0, raised to a higher power, narrows theta


def _fit(seed, scale, n=96, E=40, width=8):
    "a classificationdensenet of width 8 with E perturbed samples (two chains of E / 2, one after the other)"
    from bnn_priors_amd import models
    torch.manual_seed(0)
    x = torch.rand(n + 32, 784)
    y = torch.arange(n + 32) % 10
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
    x, y = x.to("cuda:0"), y.to("cuda:0")
    loaders = [torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[a:b], y[a:b]), batch_size=32)
               for a, b in ((0, n), (n, n + 32))]
    return net, loaders[0], loaders[1], samples


@pytest.mark.gpu
def test_evaluate_prior_sensitivity_equals_the_pipeline_by_hand():
    from bnn_priors_amd import evaluation as ev, model_comparison as mc, prior, prior_sensitivity as ps
    net, train, test, samples = _fit(3, 0.005)
    E, alpha, threshold = 40, 1.01, 0.05
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    got = ev.evaluate_prior_sensitivity(net, train, test, samples, chains=2, per_prior=True, weights=True)
    assert not net.training and all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    net.train()
    plain = ev.evaluate_prior_sensitivity(net.eval(), train, test, samples)
    assert set(plain["components"]) == {"prior", "likelihood"}

    # by hand: the components
    names = [n for n, _ in prior.named_priors(net)]
    comps = {"prior": np.empty(E), **{f"prior:{n}": np.empty(E) for n in names}}
    with torch.no_grad():
        for s in range(E):
            net.load_state_dict({k: v[s] for k, v in samples.items()})
            comps["prior"][s] = float(net.log_prior().double())
            for n, pr in prior.named_priors(net):
                comps[f"prior:{n}"][s] = float(pr.log_prob().double())
    comps["likelihood"] = _np(ev.predictive_tables(net, train, samples)[0].sum(1))
    lps = _np(ev.predictive_tables(net, test, samples)[0])
    net.load_state_dict(before)
    assert list(got["components"]) == list(comps) and len(names) >= 2 and lps.shape == (E, 32)
    tables = [lps] + [_np(v).reshape(E, -1).astype(np.float64) for v in samples.values() if v.is_floating_point()]
    Q = sum(t.shape[1] for t in tables)
    assert got["quantities"] == Q and plain["quantities"] == 32 and Q > 32
    sorts = [ref.keyed_sort(t)[:2] for t in tables]
    psi, k = {}, {}
    for name, lc in comps.items():
        weights = ps.power_scale_weights(_cuda(lc), (1.0 / alpha, alpha))
        w = _np(torch.exp(weights.log_weights))                      # the weights the kernel reads
        parts = []
        for ordered, order in sorts:
            d = ref.distance(ordered, order, w)
            print(f"{name}: {ordered.shape[1]} quantities, max |delta| {np.nanmax(d.max_delta):.3g}")
            assert d.series.all()                                        # so that psi is fixed to the bit
            parts.append((d.dist[0] + d.dist[1]) / (2.0 * math.log2(alpha)))
        psi[name], k[name] = np.concatenate(parts), _np(weights.pareto_k).tolist()
    for name in comps:
        c = got["components"][name]
        assert set(c) == {"sensitive_fraction", "psi_max", "psi_median", "pareto_k"}
        assert all(type(c[key]) is float for key in ("sensitive_fraction", "psi_max", "psi_median"))
        assert c["sensitive_fraction"] == float((psi[name] >= threshold).mean())
        assert c["psi_max"] == float(psi[name].max())
        assert c["psi_median"] == float(np.sort(psi[name])[(Q - 1) // 2])            # torch's median: the lower middle
        assert c["pareto_k"] == k[name] and len(k[name]) == 2
    codes = ref.diagnosis(psi["prior"], psi["likelihood"], threshold)
    assert got["diagnosis"] == {"none": int((codes == 0).sum()), "conflict": int((codes == 1).sum()),
                                "strong_prior": int((codes == 2).sum())}
    assert sum(got["diagnosis"].values()) == Q
    limit = mc.k_threshold(E)
    assert got["pareto_k_bad"] == sum(v > limit for ks in k.values() for v in ks)
    assert (got["alpha"], got["threshold"]) == (alpha, threshold)
    assert plain["components"]["prior"]["psi_max"] == float(psi["prior"][:32].max())
    with pytest.raises(ValueError, match="chains"):
        ev.evaluate_prior_sensitivity(net, train, test, samples, chains=3)
