"""Fitting the data-driven priors on the device (bnn_priors_amd/prior_fit.py, csrc/fit_hip.inc; definitions in
include/sgmcmc_hip.h, restated in tests/prior_fit_reference.py).

On the CPU the restatement is held to independent code (numpy.cov, scipy.stats skew / kurtosis / multivariate_t /
<family>.fit, scipy.special, the package's own density and its autograd gradient) and the wrappers to their argument
checks.  On the GPU the kernels are held to the restatement.

Tolerances.  They are measured, not guessed: the restatement is evaluated on the GPU tests' own inputs in np.float64 and
in np.longdouble (80-bit), the largest deviation per quantity is recorded, and the GPU tolerance is 4 x that (the factor
allows for the kernels' other summation order and a device log / exp an ulp from libm's).

  moments   mean relative to the column's standard deviation, cov relative to sqrt(cov_aa cov_bb), skew relative to
            1 + |skew|, kurt relative to kurt + 3:                         measured 5.43e-13 (MOMENT_DEVIATION = 5.5e-13;
            the column 1e4 standard deviations from 0 sets it, the others stay below 2e-14)
  mvt       loc relative to sqrt(S_aa), scale_tril relative to sqrt(cov_aa cov_bb), df relative, loglik and the trace
            relative to |loglik|:                                          measured 1.82e-13 (MVT_DEVIATION = 1.9e-13)
  sums      the five sums of the element-wise families, relative to the sum of their terms' magnitudes:
                                                                           measured 2.19e-16 (SUM_DEVIATION = 2.3e-16)
  marginal  the fitted parameters of norm / laplace / dgamma / gennorm / t, relative:
                                                                           measured 7.12e-15 (PARAM_DEVIATION = 7.2e-15)
  nets      log_prior and its gradient (relative to the gradient's largest entry) of the data-driven nets built from the
            fp64 and the 80-bit tables: measured 0 (the tables round to the same float32 / float64 values), so the
            tolerance is 4 x the coarsest format of the tables, the float32 means: 2^-24 (NET_DEVIATION = 6e-8)

``test_the_recorded_deviations_are_the_measured_ones`` re-measures them.  Integer counts, ``iterations``, ``converged``
and ``df_at_bound`` must be equal.  The log-likelihood trace must not decrease by more than the pass's rounding:
4 MVT_DEVIATION |loglik|.

scipy's optimiser: ``<family>.fit`` stops at xtol = ftol = 1e-4 (Nelder-Mead defaults), so its mean log-likelihood can
exceed ours only by what that leaves.  Measured on MARGINAL_DATA, scipy's mean log-likelihood minus ours: never
positive (0 for laplace and norm, whose estimates are closed forms on both sides; -1e-12 .. -7e-10 for t, gennorm and
dgamma: ours is higher).  With a measured gap of 0 the bound is 4 x one rounding of a mean log-likelihood below 2 in
magnitude, 2^-51 (SCIPY_GAP = 4.5e-16).

The autograd gradient of the package's mean log density at the restatement's fixed point (tol = 1e-13), largest entry
over (loc, scale_tril, df): 80-bit run measured 4.27e-14 (FIXED_POINT_GRADIENT = 4.3e-14; the fp64 run 1.07e-13); the bound is 4 x that.
"""
import functools

import numpy as np
import pytest
import torch

import prior_fit_reference as ref

MOMENT_DEVIATION = 5.5e-13
MVT_DEVIATION = 1.9e-13
SUM_DEVIATION = 2.3e-16
PARAM_DEVIATION = 7.2e-15
NET_DEVIATION = 6e-8
SCIPY_GAP = 4.5e-16
FIXED_POINT_GRADIENT = 4.3e-14

LD = np.longdouble


def _t_vectors(rng, n, P, df, loc_scale=1.0):
    "n vectors of a P-variate t with a random scatter and location: Gaussian / sqrt(chi2 / df) (df = inf: Gaussian)"
    A = rng.standard_normal((P, P)) / np.sqrt(P) + np.eye(P)
    z = rng.standard_normal((n, P)) @ A.T
    if np.isfinite(df):
        z = z / np.sqrt(rng.chisquare(df, (n, 1)) / df)
    return 0.05 * (z + loc_scale * rng.standard_normal(P))


# name: (S, shape, P, event_dim, permute, dtype, df of the data, view)
#   events: 1, 257 and a count that is no multiple of the tile and needs more than one workgroup, per P in {1, 9, 25};
#   F = 3 through (1, 0, 2, 3) with event_dim = 3; views: "t" a transposed stack, "s" every second sample of a longer one
CASES = {
    "p1_one": (1, (1,), 1, None, None, "float64", 4, ""),
    "p1_257": (257, (1,), 1, None, None, "float32", 4, ""),
    "p1_1300": (100, (13,), 1, None, None, "float32", 2.5, "s"),
    "p9_one": (1, (1, 1, 3, 3), 9, None, None, "float32", 4, ""),
    "p9_257": (1, (257, 1, 3, 3), 9, None, None, "float64", 4, "t"),
    "p9_1100": (11, (20, 5, 3, 3), 9, None, None, "float32", 50, ""),
    "p25_257": (1, (257, 1, 5, 5), 25, None, None, "float32", 2.5, ""),
    "p25_500": (5, (10, 10, 5, 5), 25, None, None, "float64", 4, "s"),
    "f3_350": (70, (3, 5, 3, 3), 9, 3, (1, 0, 2, 3), "float64", 4, ""),
    "f3_350_f32": (70, (3, 5, 3, 3), 9, 3, (1, 0, 2, 3), "float32", 2.5, "s"),
    "far_mean": (3, (100, 1, 3, 3), 9, None, None, "float64", 4, ""),
    "gauss": (1, (257, 1, 3, 3), 9, None, None, "float64", np.inf, ""),
}
MVT_CASES = ("p1_1300", "p9_257", "p9_1100", "p25_500", "f3_350", "f3_350_f32", "gauss", "p1_257", "p25_257")
MVT_ARGS = {"p9_1100": dict(max_iter=60), "gauss": dict(df_bounds=(2.01, 25.)), "p25_257": dict(max_iter=40)}


@functools.lru_cache(maxsize=None)
def _stack(name):
    "the stack of a case as a read-only numpy array of its dtype"
    S, shape, P, event_dim, permute, dtype, df, view = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    n = S * int(np.prod(shape)) // P
    F = 1 if event_dim is None else int(np.prod([shape[p] for p in permute][len(shape) - event_dim:])) // P
    x = _t_vectors(rng, n // F, F * P, df)                     # an event's vectors share the mixing variable
    if name == "far_mean":
        x[:, 4] += 1e4 * x[:, 4].std()
    if permute is None:
        w = x.reshape((S,) + shape)
    else:
        w = x.reshape((S,) + tuple(shape[p] for p in permute))
        w = np.transpose(w, (0,) + tuple(1 + int(i) for i in np.argsort(permute)))
    w = np.ascontiguousarray(w).astype(dtype)
    w.setflags(write=False)
    return w


def _device_stack(name):
    "the stack on the GPU: contiguous, or the case's non-contiguous view of a larger allocation"
    w = torch.from_numpy(_stack(name).copy()).cuda()
    view = CASES[name][7]
    if view == "t":                                             # stored with its last two dimensions swapped
        return w.transpose(-1, -2).contiguous().transpose(-1, -2)
    if view == "s":                                             # every second sample of a stack twice as long
        big = torch.zeros((2 * w.shape[0],) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
        big[::2] = w
        return big[::2]
    return w


@functools.lru_cache(maxsize=None)
def _moments_ref(name, wide):
    S, shape, P, event_dim, permute = CASES[name][:5]
    E = ref.events_of(_stack(name), P, event_dim, permute)
    return ref.moments_reference(E.reshape(-1, P), 1, LD if wide else np.float64)


@functools.lru_cache(maxsize=None)
def _mvt_ref(name, wide):
    S, shape, P, event_dim, permute = CASES[name][:5]
    E = ref.events_of(_stack(name), P, event_dim, permute)
    return ref.fit_mvt_reference(E, dtype=LD if wide else np.float64, **MVT_ARGS.get(name, {}))


def _moment_deviation(got, wide):
    sd = np.sqrt(np.diag(wide["cov"]))
    dev = [np.max(np.abs(got["mean"] - wide["mean"]) / sd),
           np.max(np.abs(got["cov"] - wide["cov"]) / np.outer(sd, sd)),
           np.max(np.abs(got["skew"] - wide["skew"]) / (1 + np.abs(wide["skew"]))),
           np.max(np.abs(got["kurt"] - wide["kurt"]) / (wide["kurt"] + 3)),
           abs(got["pooled_mean"] - wide["pooled_mean"]) / np.sqrt(wide["pooled_var"]),
           abs(got["pooled_var"] - wide["pooled_var"]) / wide["pooled_var"],
           abs(got["pooled_skew"] - wide["pooled_skew"]) / (1 + abs(wide["pooled_skew"])),
           abs(got["pooled_kurt"] - wide["pooled_kurt"]) / (wide["pooled_kurt"] + 3)]
    return float(max(dev))


def _mvt_deviation(got, wide):
    sd = np.sqrt(np.diag(wide["S"]))
    L = wide["scale_tril"]
    cs = np.sqrt(np.diag(L @ L.T))
    k = min(len(got["trace"]), len(wide["trace"]))
    dev = [np.max(np.abs(got["loc"] - wide["loc"]) / sd),
           np.max(np.abs(got["scale_tril"] - L) / np.outer(cs, cs)),
           abs(got["df"] - wide["df"]) / wide["df"],
           abs(got["loglik"] - wide["loglik"]) / abs(wide["loglik"]),
           np.max(np.abs(got["trace"][:k] - wide["trace"][:k]) / abs(wide["loglik"])) if k else 0.0]
    return float(max(dev))


MARGINAL_DATA = {"t3": (3, 0.1, 0.0), "t8_shifted": (8, 2.0, 0.3), "gauss": (np.inf, 0.5, 0.0)}


@functools.lru_cache(maxsize=None)
def _marginal_data(name):
    df, scale, loc = MARGINAL_DATA[name]
    rng = np.random.default_rng(len(name))
    x = loc + scale * _t_vectors(rng, 3000, 1, df, loc_scale=0.0).reshape(-1) / 0.05
    x.setflags(write=False)
    return x, loc


@functools.lru_cache(maxsize=None)
def _marginal_ref(name, wide):
    x, loc = _marginal_data(name)
    return ref.fit_marginal_reference(x, loc=loc, dtype=LD if wide else np.float64)


def _sum_deviation(x, loc, beta):
    d = np.abs(x.astype(LD) - LD(loc))
    d = d[d != 0]
    l, p = np.log(d), np.exp(LD(beta) * np.log(d))
    mags = np.array([d.sum(), np.abs(l).sum(), p.sum(), np.abs(p * l).sum(), (p * l * l).sum()])
    got = ref.abs_stats_reference(x, loc, beta)[2]
    wide = ref.abs_stats_reference(x, loc, beta, LD)[2]
    return float(np.max(np.abs(got - wide) / mags)), mags


def _param_deviation(got, wide, fams):
    return max(float(abs(g - w) / abs(w)) for fam in fams for g, w in zip(got[fam][0], wide[fam][0]) if w != 0)


# ---------------------------------------------------------------------------------------------------------- CPU: restatement

def test_moments_restatement_against_numpy_and_scipy():
    import scipy.stats as st
    for name in ("p9_1100", "far_mean", "p25_257", "p1_1300"):
        P = CASES[name][2]
        X = ref.events_of(_stack(name), P).reshape(-1, P).astype(np.float64)
        m = _moments_ref(name, False)
        assert m["n"] == X.shape[0]
        np.testing.assert_allclose(m["mean"], X.mean(0), rtol=1e-12)
        np.testing.assert_allclose(m["cov"], np.cov(X, rowvar=False).reshape(P, P), rtol=1e-9, atol=1e-18)
        np.testing.assert_allclose(m["skew"], st.skew(X, axis=0, bias=True), rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(m["kurt"], st.kurtosis(X, axis=0, bias=True), rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(m["pooled_skew"], st.skew(X.reshape(-1), bias=True), rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(m["pooled_kurt"], st.kurtosis(X.reshape(-1), bias=True), rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(m["pooled_var"], X.var(), rtol=1e-9)


def test_far_mean_keeps_its_digits_and_special_columns_are_reported():
    X = ref.events_of(_stack("far_mean"), 9).reshape(-1, 9).astype(LD)
    exact = ((X[:, 4] - X[:, 4].mean()) ** 2).mean()
    assert abs(_moments_ref("far_mean", False)["var"][4] - exact) / exact < 1e-13      # 1e4 standard deviations from 0
    X = np.array(_stack("p9_1100")).reshape(-1, 9).astype(np.float64)
    X[:, 2] = 0.25
    m = ref.moments_reference(X)
    assert m["var"][2] == 0 and m["cov"][2, 2] == 0 and np.isnan(m["skew"][2]) and np.isnan(m["kurt"][2])
    assert np.isfinite(np.delete(m["skew"], 2)).all()
    X[7, 3] = np.inf
    m = ref.moments_reference(X)
    assert m["bad"] == 1 and np.isnan(m["mean"]).all() and np.isnan(m["cov"]).all() and np.isnan(m["pooled_kurt"])


def test_loglik_restatement_against_scipy_and_the_package_density():
    import scipy.stats as st
    from bnn_priors_amd.prior import distributions
    f = _mvt_ref("p9_257", False)
    E = ref.events_of(_stack("p9_257"), 9).astype(np.float64)
    want = st.multivariate_t(loc=f["loc"], shape=f["S"], df=f["df"]).logpdf(E[:, 0]).sum()
    assert ref.mvt_loglik(E, f["loc"], f["S"], f["df"]) == pytest.approx(want, rel=1e-12)
    assert f["loglik"] == pytest.approx(want, rel=1e-12)
    f = _mvt_ref("f3_350", False)                                                        # F = 3: one mixing variable
    E = ref.events_of(_stack("f3_350"), 9, 3, (1, 0, 2, 3)).astype(np.float64)
    dist = distributions.MultivariateT(torch.Size([3, 9]), df=float(f["df"]), loc=torch.from_numpy(f["loc"]),
                                       scale_tril=torch.from_numpy(f["scale_tril"]))
    assert f["loglik"] == pytest.approx(float(dist.log_prob(torch.from_numpy(E)).sum()), rel=1e-12)


def test_em_restatement_trace_never_decreases_and_reaches_the_fixed_point():
    for name in ("p1_1300", "p9_257", "f3_350", "f3_350_f32"):
        f = _mvt_ref(name, False)
        tr = np.append(f["trace"], f["loglik"])
        assert f["converged"] and f["iterations"] < 500
        assert np.diff(tr).min() >= -4 * MVT_DEVIATION * abs(f["loglik"]), name
    f = _mvt_ref("p1_1300", False)                                                       # df = 2.5 data
    assert f["loglik"] > f["trace"][0] + 1.0 and f["df"] < 5


def test_fixed_point_has_zero_gradient_of_the_package_density():
    from bnn_priors_amd.prior import distributions
    E = ref.events_of(_stack("f3_350"), 9, 3, (1, 0, 2, 3)).astype(np.float64)
    grads = {}
    for wide in (False, True):
        f = ref.fit_mvt_reference(E, tol=1e-13, dtype=LD if wide else np.float64)
        loc = torch.tensor(np.asarray(f["loc"], np.float64), requires_grad=True)
        L = torch.tensor(np.asarray(f["scale_tril"], np.float64), requires_grad=True)
        df = torch.tensor(float(f["df"]), dtype=torch.float64, requires_grad=True)
        dist = distributions.MultivariateT(torch.Size([3, 9]), df=df, loc=loc, scale_tril=L)
        (dist.log_prob(torch.from_numpy(E)).sum() / E.shape[0]).backward()
        grads[wide] = max(float(loc.grad.abs().max()), float(torch.tril(L.grad).abs().max()), abs(float(df.grad)))
    print("fixed-point gradient: fp64 run", grads[False], "80-bit run", grads[True])
    assert grads[True] <= FIXED_POINT_GRADIENT
    assert grads[False] <= 4 * FIXED_POINT_GRADIENT


@pytest.mark.parametrize("name", sorted(MARGINAL_DATA))
def test_marginal_restatement_against_scipy_fit(name):
    import scipy.stats as st
    x, loc = _marginal_data(name)
    got = _marginal_ref(name, False)
    for fam, dist, kw in (("laplace", st.laplace, dict(floc=loc)), ("dgamma", st.dgamma, dict(floc=loc)),
                          ("gennorm", st.gennorm, dict(floc=loc)), ("t", st.t, {}), ("norm", st.norm, {})):
        if fam == "t" and name == "gauss":
            continue                                             # no finite df: EM stops at max_iter, scipy anywhere
        theirs = dist.logpdf(x, *dist.fit(x, **kw)).mean()
        ours = dist.logpdf(x, *[float(v) for v in got[fam][0]]).mean()
        print(name, fam, "scipy - ours", theirs - ours)
        assert ours >= theirs - 4 * SCIPY_GAP, (fam, theirs - ours)
        assert float(got[fam][1]) == pytest.approx(ours, rel=1e-10, abs=1e-12)           # the reported mean loglik


def test_digamma_trigamma_and_log_gamma_against_scipy():
    import scipy.special as sp
    eps = 2.0 ** -52
    for x in np.exp(np.linspace(np.log(1e-3), np.log(1e5), 400)):
        # a recurrence of up to 10 terms below 1 / x (each rounded once), a log and a short series
        assert abs(ref.digamma(x) - sp.digamma(x)) <= 16 * eps * (1 / x + 3 + abs(sp.digamma(x)))
        assert abs(ref.trigamma(x) - sp.polygamma(1, x)) <= 16 * eps * sp.polygamma(1, x)
        assert abs(ref.log_gamma(x) - sp.gammaln(x)) <= 16 * eps * (abs(sp.gammaln(x)) + x * max(np.log(x), 1) + 25)


def test_host_solvers_agree_with_the_restatement():
    "prior_fit's host-side Newton solves (plain floats) are the restatement's"
    from bnn_priors_amd import prior_fit as pf
    for x in (1e-3, 0.3, 1.4616, 7.0, 10.0, 123.4, 1e5):
        assert pf._digamma(x) == pytest.approx(float(ref.digamma(x)), rel=1e-15, abs=1e-15)
        assert pf._trigamma(x) == pytest.approx(float(ref.trigamma(x)), rel=1e-15)
    for name in MARGINAL_DATA:
        x, loc = _marginal_data(name)
        want = _marginal_ref(name, False)
        n, zeros, sums = ref.abs_stats_reference(x, loc, 1.0)
        for got, fam in ((pf._laplace_params(n, sums, loc), "laplace"), (pf._dgamma_params(n, zeros, sums, loc), "dgamma"),
                         (pf._gennorm_params(lambda b: ref.abs_stats_reference(x, loc, b)[2], n, loc), "gennorm")):
            np.testing.assert_allclose(got[0], np.asarray(want[fam][0], np.float64), rtol=1e-12)
            assert got[1] == pytest.approx(float(want[fam][1]), rel=1e-12)


def test_argument_checks_name_the_limit():
    from bnn_priors_amd import prior_fit as pf
    w = torch.zeros(2, 4, 3, 3, 3)
    with pytest.raises(ValueError, match="CUDA tensor"):
        pf.moments(w, 9)
    with pytest.raises(ValueError, match="CUDA tensor"):
        pf.fit_mvt(w, 9)
    with pytest.raises(ValueError, match="CUDA tensor"):
        pf.fit_marginal(w)
    with pytest.raises(ValueError, match=r"P = 26: 1 \.\. 25"):
        pf.fit_mvt(torch.zeros(2, 4, 26), 26)
    with pytest.raises(ValueError, match="P = 5 does not divide the event"):
        pf.fit_mvt(w, 5, event_dim=2)
    with pytest.raises(ValueError, match="P = 6 does not divide the event"):
        pf.moments(w, 6)
    with pytest.raises(ValueError, match=r"unsupported permutation \(0, 1, 3, 2\).*\(1, 0, 2, 3\) with event_dim = 3"):
        pf.fit_mvt(w, 9, event_dim=2, permute=(0, 1, 3, 2))
    with pytest.raises(ValueError, match="unsupported permutation"):
        pf.fit_mvt(w, 9, event_dim=2, permute=(1, 0, 2, 3))
    with pytest.raises(ValueError, match="2 < lower"):
        pf.fit_mvt(w, 9, df_bounds=(2.0, 100.))
    with pytest.raises(ValueError, match="2 < lower"):
        pf.fit_mvt(w, 9, df_bounds=(1.5, 100.))
    with pytest.raises(ValueError, match=rf"at most {pf.MAX_F} vectors"):
        pf.fit_mvt(torch.zeros(1, 600, 2, 3, 3), 9, event_dim=3, permute=(1, 0, 2, 3))
    with pytest.raises(ValueError, match="3 of the 10 elements equal loc = 0.5.*at most 0"):
        pf._dgamma_params(10, 3, [1.0, 1.0, 1.0, 1.0, 1.0], 0.5)
    with pytest.raises(ValueError, match="unknown families"):
        pf.fit_marginal(w, ("cauchy",))
    g, event_dim, permute = pf._geometry(torch.zeros(7, 3, 5, 3, 3)[:, :, ::2], 9, 3, (1, 0, 2, 3))
    assert (g.P, g.F, g.events, g.f_stride, g.f_major, event_dim) == (9, 3, 21, 45, 1, 3)
    assert list(g.size) == [1, 1, 7, 3] and list(g.stride) == [0, 0, 135, 18] and list(g.pos)[:9] == list(range(9))
    assert pf.tile_events(9, 1) == 512 and pf.tile_events(25, 1) == 204 and pf.tile_events(9, 3) == 170


def _measure():
    "the deviations of the module's docstring: {quantity: largest fp64-to-80-bit deviation of the restatement}"
    out = {"moments": max(_moment_deviation(_moments_ref(n, False), _moments_ref(n, True)) for n in CASES
                          if CASES[n][0] * int(np.prod(CASES[n][1])) > CASES[n][2]),
           "mvt": max(_mvt_deviation(_mvt_ref(n, False), _mvt_ref(n, True)) for n in MVT_CASES),
           "sums": max(_sum_deviation(*_marginal_data(n), beta)[0] for n in MARGINAL_DATA for beta in (1.0, 0.7, 2.5)),
           "marginal": max(_param_deviation(_marginal_ref(n, False), _marginal_ref(n, True),
                                            [f for f in ("norm", "laplace", "dgamma", "gennorm", "t")
                                             if not (f == "t" and n == "gauss")]) for n in MARGINAL_DATA)}
    return out


def test_the_recorded_deviations_are_the_measured_ones():
    got = _measure()
    print(got)
    for key, recorded in (("moments", MOMENT_DEVIATION), ("mvt", MVT_DEVIATION), ("sums", SUM_DEVIATION),
                          ("marginal", PARAM_DEVIATION)):
        assert got[key] <= recorded <= max(2 * got[key], 2.0 ** -52 * 1.01), (key, got[key], recorded)
    for n in MVT_CASES:                                        # the integer outcomes do not depend on the precision
        a, b = _mvt_ref(n, False), _mvt_ref(n, True)
        assert (a["iterations"], a["converged"], a["df_at_bound"]) == (b["iterations"], b["converged"], b["df_at_bound"])


# ---------------------------------------------------------------------------------------------------------------- GPU: kernels

def _moments_dict(m):
    return dict(mean=m.mean.cpu().numpy(), cov=m.cov.cpu().numpy(), skew=m.skew.cpu().numpy(), kurt=m.kurt.cpu().numpy(),
                var=m.var.cpu().numpy(), pooled_mean=float(m.pooled_mean), pooled_var=float(m.pooled_var),
                pooled_skew=float(m.pooled_skew), pooled_kurt=float(m.pooled_kurt))


def _fit_dict(f):
    L = f.scale_tril.numpy()
    return dict(loc=f.loc.numpy(), scale_tril=L, df=f.df, loglik=f.loglik, trace=f.trace.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_moments_kernel_against_the_restatement(name):
    from bnn_priors_amd import prior_fit as pf
    S, shape, P, event_dim, permute = CASES[name][:5]
    w = _device_stack(name)
    assert w.is_contiguous() == (CASES[name][7] == "")
    ddof = int(S * int(np.prod(shape)) > P)                    # (one vector has no n - 1)
    m = pf.moments(w, P, event_dim, permute, ddof=ddof)
    wide = _moments_ref(name, True)
    assert m.n == wide["n"] and isinstance(m.n, int)
    again = pf.moments(w, P, event_dim, permute, ddof=ddof)
    for a, b in zip(m[1:], again[1:]):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b)      # two calls, the same bits
    if m.n == 1:                                               # one vector: its mean, no spread
        np.testing.assert_array_equal(m.mean.cpu().numpy(), np.asarray(wide["mean"], np.float64))
        assert bool(m.zero_variance.all()) and bool(torch.isnan(m.skew).all()) and bool((m.var == 0).all())
        return
    dev = _moment_deviation(_moments_dict(m), wide)
    print(name, "moments deviation", dev)
    assert dev <= 4 * MOMENT_DEVIATION
    assert not bool(m.zero_variance.any())


@pytest.mark.gpu
def test_moments_kernel_special_inputs():
    from bnn_priors_amd import prior_fit as pf
    x = np.array(_stack("p9_1100"))
    x[..., 0, 2] = 0.25                                        # a column of zero variance: reported, not divided by
    m = pf.moments(torch.from_numpy(x).cuda(), 9)
    want = ref.moments_reference(x.reshape(-1, 9).astype(np.float64), 1, LD)
    assert m.zero_variance.tolist() == [a == 2 for a in range(9)]
    assert float(m.var[2]) == 0 and float(m.cov[2, 2]) == 0 and bool(torch.isnan(m.skew[2])) and bool(torch.isnan(m.kurt[2]))
    keep = [a for a in range(9) if a != 2]
    np.testing.assert_allclose(m.kurt.cpu().numpy()[keep], np.asarray(want["kurt"], np.float64)[keep],
                               rtol=4 * MOMENT_DEVIATION * 10)  # (relative to kurt + 3 <= 10 |kurt| on these columns)
    f = pf.fit_mvt(torch.from_numpy(x).cuda(), 9)              # ... and a singular scatter ends the fit
    assert not f.converged and np.isnan(f.df) and bool(torch.isnan(f.loc).all())
    x[3, 7, 1, 1, 1] = np.nan                                  # a NaN anywhere: every output NaN
    m = pf.moments(torch.from_numpy(x).cuda(), 9)
    assert all(bool(torch.isnan(t).all()) for t in m[1:10])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MVT_CASES)
def test_mvt_kernels_against_the_restatement(name):
    from bnn_priors_amd import prior_fit as pf
    S, shape, P, event_dim, permute = CASES[name][:5]
    kw = MVT_ARGS.get(name, {})
    w = _device_stack(name)
    f = pf.fit_mvt(w, P, event_dim, permute, **kw)
    want, wide = _mvt_ref(name, False), _mvt_ref(name, True)
    dev = _mvt_deviation(_fit_dict(f), wide)
    print(name, "iterations", f.iterations, want["iterations"], "df", f.df, "deviation", dev)
    assert (f.iterations, f.converged, f.df_at_bound) == (want["iterations"], want["converged"], want["df_at_bound"])
    assert len(f.trace) == f.iterations
    assert dev <= 4 * MVT_DEVIATION
    tr = np.append(f.trace.numpy(), f.loglik)
    assert np.diff(tr).min() >= -4 * MVT_DEVIATION * abs(f.loglik)                       # never decreases
    if CASES[name][6] == 2.5:
        assert f.loglik > tr[0] + 1.0                                                    # strictly above its start
    if name == "gauss":
        assert f.df_at_bound and f.df == 25.0
    for every in (1, 64):                                      # the same bits however the iterations are batched
        g = pf.fit_mvt(w, P, event_dim, permute, check_every=every, **kw)
        assert (g.iterations, g.converged, g.df, g.loglik) == (f.iterations, f.converged, f.df, f.loglik)
        assert torch.equal(g.loc, f.loc) and torch.equal(g.scale_tril, f.scale_tril) and torch.equal(g.trace, f.trace)
    if event_dim is not None:
        pr = f.prior(shape)
        spec = pr.fused_mvt_spec()
        assert spec is not None and spec["P"] == P and spec["df"] == pytest.approx(f.df)


@pytest.mark.gpu
def test_mvt_prior_of_an_unpermuted_fit_is_in_the_hook():
    from bnn_priors_amd import prior_fit as pf
    f = pf.fit_mvt(_device_stack("p9_1100"), 9)
    assert f.event_dim == 2 and f.permute == (0, 1, 2, 3)
    spec = f.prior((20, 5, 3, 3)).fused_mvt_spec()
    assert spec is not None and spec["ev_size"] == 9


@pytest.mark.gpu
def test_mvt_kernels_special_inputs():
    from bnn_priors_amd import prior_fit as pf
    x = np.array(_stack("p9_257"))
    x[0, 100, 0, 1, 2] = np.nan
    f = pf.fit_mvt(torch.from_numpy(x).cuda(), 9)
    assert not f.converged and f.iterations == 0 and np.isnan(f.df) and np.isnan(f.loglik)
    assert bool(torch.isnan(f.loc).all()) and bool(torch.isnan(f.scale_tril).all())
    f = pf.fit_mvt(_device_stack("p9_one"), 9)                 # one event: no scatter to start from
    assert not f.converged and np.isnan(f.df)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MARGINAL_DATA))
def test_marginal_fits_against_the_restatement(name):
    from bnn_priors_amd import prior_fit as pf
    x, loc = _marginal_data(name)
    w = torch.from_numpy(x.reshape(3, 1000).copy()).cuda()
    for beta in (1.0, 0.7, 2.5):
        n, zeros, sums = pf.abs_stats(w, loc, beta)
        _, mags = _sum_deviation(x, loc, beta)
        wide = ref.abs_stats_reference(x, loc, beta, LD)
        assert (n, zeros) == (wide[0], wide[1]) and isinstance(zeros, int)
        dev = float(np.max(np.abs(sums.numpy() - wide[2]) / mags))
        print(name, beta, "sum deviation", dev)
        assert dev <= 4 * SUM_DEVIATION
    fams = tuple(f for f in pf.FAMILIES if not (f == "t" and name == "gauss"))
    got = pf.fit_marginal(w, fams, loc=loc)
    wide = _marginal_ref(name, True)
    for fam in fams:
        want = np.asarray(wide[fam][0], np.float64)
        np.testing.assert_allclose(got[fam][0], want, rtol=4 * PARAM_DEVIATION, atol=4 * PARAM_DEVIATION * float(want[-1]),
                                   err_msg=fam)
        assert got[fam][1] == pytest.approx(float(wide[fam][1]), rel=4 * PARAM_DEVIATION, abs=4 * PARAM_DEVIATION)


@pytest.mark.gpu
def test_zeros_are_counted_and_refused_by_dgamma_only():
    from bnn_priors_amd import prior_fit as pf
    x = np.array(_marginal_data("t3")[0])
    x[[5, 700, 2999]] = 0.0
    w = torch.from_numpy(x).cuda().to(torch.float32)
    n, zeros, _ = pf.abs_stats(w, 0.0, 1.0)
    assert (n, zeros) == (3000, 3)
    with pytest.raises(ValueError, match="3 of the 3000 elements equal loc"):
        pf.fit_marginal(w, ("dgamma",))
    got = pf.fit_marginal(w, ("laplace", "gennorm"))
    want = ref.fit_marginal_reference(w.cpu().numpy(), ("laplace", "gennorm"), 0.0, LD)
    for fam in got:
        np.testing.assert_allclose(got[fam][0], np.asarray(want[fam][0], np.float64), rtol=4 * PARAM_DEVIATION)


def _conv_stacks(rng):
    "stacks drawn for the three modules of the data-driven convnet at width 8: heavy-tailed, correlated filters"
    S, width = 6, 8
    shapes = {"net.module.1.weight_prior.p": (width, 1, 3, 3), "net.module.1.bias_prior.p": (width,),
              "net.module.4.weight_prior.p": (width, width, 3, 3), "net.module.4.bias_prior.p": (width,),
              "net.module.8.weight_prior.p": (10, width * 49), "net.module.8.bias_prior.p": (10,)}
    out = {}
    for key, shape in shapes.items():
        n = S * int(np.prod(shape))
        x = _t_vectors(rng, n // 9, 9, 5) if len(shape) == 4 else _t_vectors(rng, n, 1, 5, loc_scale=0.0)
        out[key] = x.reshape((S,) + shape).astype(np.float32)
    return out


def _net_outputs(name, prior_data):
    from bnn_priors_amd import models
    torch.manual_seed(0)
    x, y = torch.rand(4, 784), torch.arange(4) % 10
    net = models.get_model(x, y, name, width=8, depth=3, prior_data=prior_data).double()
    rng = np.random.default_rng(5)
    with torch.no_grad():
        for _, p in net.named_parameters():
            p.copy_(torch.from_numpy(rng.standard_normal(p.shape) * 0.05))
    lp = net.log_prior()
    lp.backward()
    return float(lp.detach()), torch.cat([p.grad.reshape(-1) for _, p in net.named_parameters()]).numpy()


@pytest.mark.gpu
def test_fit_prior_data_round_trip_builds_the_data_driven_nets():
    from bnn_priors_amd import prior_fit as pf
    from bnn_priors_amd.models import data_driven
    stacks = _conv_stacks(np.random.default_rng(11))
    got = pf.fit_prior_data({k: torch.from_numpy(v).cuda() for k, v in stacks.items()})
    tables = [ref.fit_prior_data_reference(stacks, data_driven.MEAN_COVS_FILE, data_driven.FITS_FILE, dt)
              for dt in (np.float64, LD)]
    assert set(got) == {data_driven.MEAN_COVS_FILE, data_driven.FITS_FILE}
    mc = got[data_driven.MEAN_COVS_FILE]
    assert mc["net.module.4.weight_prior.p"][0].dtype == np.float32 and mc["net.module.4.weight_prior.p"][0].shape == (9,)
    assert mc["net.module.4.weight_prior.p"][1].dtype == np.float64 and mc["net.module.4.weight_prior.p"][1].shape == (9, 9)
    for name in ("datadrivengaussconv", "datadrivendoublegammaconv"):
        lp, grad = _net_outputs(name, got)
        (lp64, g64), (lp80, g80) = (_net_outputs(name, t) for t in tables)
        measured = max(abs(lp64 - lp80) / abs(lp80), float(np.abs(g64 - g80).max() / np.abs(g80).max()))
        print(name, "fp64 vs 80-bit tables", measured)
        assert measured <= NET_DEVIATION
        assert abs(lp - lp80) <= 4 * NET_DEVIATION * abs(lp80)
        assert np.abs(grad - g80).max() <= 4 * NET_DEVIATION * np.abs(g80).max()
    f = pf.fit_mvt(torch.from_numpy(stacks["net.module.4.weight_prior.p"]).cuda(), 9, event_dim=3, permute=(1, 0, 2, 3))
    assert f.prior((8, 8, 3, 3)).fused_mvt_spec() is not None
