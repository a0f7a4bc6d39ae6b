"""The fused prior kernels of csrc/sgmcmc_hip.hip ("fused priors") against the plain float64 reference of
tests/prior_reference.py, at every route, chunk geometry, item raggedness and edge value -- with per-family bounds derived
from the arithmetic the kernel documents instead of an rtol.

CPU: the reference itself against torch.distributions and against the values captured from the original project
(tests/golden/priors.npz, priors_remaining.npz), and the bounds against numpy emulations of deliberately wrong kernels.
GPU: tables built from raw specs through ``Engine`` + ``set_priors`` (no Prior module between the test and the kernel),
the two whitened kinds (FILTER_WHITENED, MULTIVARIATE_T) included, against ``prior_reference.whitened``.

Every GPU test prints one line ``prior-ratios {...}`` with its worst error / bound per family (docs/lab_notes.md)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import prior_reference as R
from bnn_priors_amd import _hip

GPU = pytest.mark.gpu
INVALID_VALUE = 1           # hipErrorInvalidValue
NAMES = {R.NORMAL: "normal", R.LAPLACE: "laplace", R.STUDENT_T: "student-t", R.CAUCHY: "cauchy", R.GENNORM: "gennorm",
         R.GAMMA_SOFTPLUS: "gamma", R.UNIFORM_CDF: "uniform-cdf", R.HALFCAUCHY_SOFTPLUS: "half-cauchy",
         R.IMPROPER_SOFTPLUS: "improper"}
# (loc, scale, df, N): an ordinary setting, small N, a tiny scale with df < 1, a huge scale with df = 1e6, irrational scale;
# GENNORM takes beta from BETAS in place of df
SETTINGS = [(0.1, 0.7, 3.0, 123.0), (-0.2, 1.3, 1.0, 7.0), (0.25, 1e-3, 0.5, 1.0), (0.0, 1e3, 1e6, 6e4),
            (1.7, 2 ** .5, 2.5, 5e4)]
BETAS = [0.5, 1.0, 1.7, 2.0, 8.0]
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 6]
CHUNKS = [_hip.CHUNK, _hip.CHUNK_SMALL]
DTYPES = ["float32", "float64"]


# ===================================================================================================== CPU: the reference
def _torch_dist(kind, loc, scale, df):
    t = lambda v: torch.tensor(v, dtype=torch.float64)         # noqa: E731
    D = torch.distributions
    return {R.NORMAL: lambda: D.Normal(t(loc), t(scale)), R.LAPLACE: lambda: D.Laplace(t(loc), t(scale)),
            R.STUDENT_T: lambda: D.StudentT(t(df), t(loc), t(scale)), R.CAUCHY: lambda: D.Cauchy(t(loc), t(scale))}[kind]()


@pytest.mark.parametrize("kind", [R.NORMAL, R.LAPLACE, R.STUDENT_T, R.CAUCHY])
def test_reference_reproduces_torch_distributions(kind):
    rng = np.random.default_rng(kind)
    for loc, scale, df, N in SETTINGS:
        if df > 1e3:
            continue        # (torch's own lgamma(df/2 + 1/2) - lgamma(df/2) has lost 7 digits there; see lgamma_half_step)
        theta = loc + scale * rng.standard_normal(500) * rng.choice([0.01, 1.0, 30.0], 500)
        g = rng.standard_normal(500)
        ref = R.elementwise(kind, loc, scale, df, N, theta, g, R.U64)
        th = torch.from_numpy(theta).requires_grad_(True)
        lp = _torch_dist(kind, loc, scale, df).log_prob(th).sum()
        lp.backward()
        np.testing.assert_allclose(ref["g"], g - th.grad.numpy() / N, rtol=1e-12, atol=1e-14)
        assert ref["logp"] == pytest.approx(float(lp.detach()), rel=1e-12)
        # d/dscale of the summed log-density, the chain-rule input of a linked segment
        sc = torch.tensor(scale, dtype=torch.float64, requires_grad=True)
        D = torch.distributions
        dist = {R.NORMAL: lambda: D.Normal(loc, sc), R.LAPLACE: lambda: D.Laplace(loc, sc),
                R.STUDENT_T: lambda: D.StudentT(df, loc, sc), R.CAUCHY: lambda: D.Cauchy(loc, sc)}[kind]()
        dist.log_prob(torch.from_numpy(theta)).sum().backward()
        assert ref["dls"] == pytest.approx(float(sc.grad), rel=1e-11, abs=1e-9 * ref["dls_abs"])


def test_lgamma_half_step_is_the_difference_it_names():
    for a in (0.25, 0.5, 1.0, 1.25, 7.3, 31.9):
        assert R.lgamma_half_step(a) == math.lgamma(a + 0.5) - math.lgamma(a)
    for a in (32.0, 40.5, 100.0):           # the two statements agree where both are accurate (|lgamma| < 400)
        assert R.lgamma_half_step(a) == pytest.approx(math.lgamma(a + 0.5) - math.lgamma(a), abs=2e-13)
    # two half steps are one whole step: lgamma(a + 1) - lgamma(a) = log(a), at sizes where math.lgamma has lost it
    for a in (32.0, 1e3, 5e5, 3e9):
        assert R.lgamma_half_step(a) + R.lgamma_half_step(a + 0.5) == pytest.approx(math.log(a), rel=1e-15)
    assert math.lgamma(5e5 + 0.5) - math.lgamma(5e5) != pytest.approx(R.lgamma_half_step(5e5), rel=1e-11)


def _spec_of_fixture(name, extra, loc, scale):
    "the raw table rows of a case of tests/golden/make_prior_goldens.py: (weight spec, hyper spec or None)"
    kw = {}
    for item in filter(None, extra.split("_")):
        for field in ("hyperscale", "rate", "beta", "df"):
            if item.startswith(field):
                kw[field] = float(item[len(field):])
    base, _, hyper = name.partition("_")
    if name == "horseshoe":
        base, hyper = "gaussian", "halfcauchy"
    kind = {"gaussian": R.NORMAL, "laplace": R.LAPLACE, "student-t": R.STUDENT_T, "cauchy": R.CAUCHY,
            "gennorm": R.GENNORM, "improper": R.NONE}[base]
    shape = {R.STUDENT_T: kw.get("df", 2.0 if hyper else 3.0), R.GENNORM: kw.get("beta", 0.0)}.get(kind, 0.0)
    hyper_spec = {"": None, "gamma": (R.GAMMA_SOFTPLUS, scale, kw.get("rate", 1.0)),         # hierarchical.py
                  "uniform": (R.UNIFORM_CDF, 0.0, 2.0 * scale),
                  "halfcauchy": (R.HALFCAUCHY_SOFTPLUS, scale, kw.get("hyperscale", 1.0)),
                  "empirical": (R.IMPROPER_SOFTPLUS, 0.0, 1.0)}[hyper]
    return (kind, loc, scale, shape), hyper_spec


def _reference_of_fixture(weight, hyper, theta, s, u):
    "-> (log p weight, d log p / d theta, x, log p hyper, d(log p weight + log p hyper) / ds) from the reference, N = 1"
    kind, loc, scale, shape = weight
    if kind == R.NONE:
        return 0.0, np.zeros(theta.size), None, None, None
    g0 = np.zeros(theta.size)
    if hyper is None:
        ref = R.elementwise(kind, loc, scale, shape, 1.0, theta, g0, u)
        return ref["logp"], -ref["g"], None, None, None
    x = R.hyper_value(*hyper, s)[0]
    ref = R.elementwise(kind, loc, x, shape, 1.0, theta, g0, u)
    h = R.hyper_segment(*hyper, s, 1.0, 0.0, u, chains=[ref])
    return ref["logp"], -ref["g"], h["x"], h["logp"], -h["g"]


def test_reference_reproduces_the_original_projects_values(golden_dir):
    """all 96 cases of priors.npz and the 16 ``gaussian_empirical`` / ``laplace_empirical`` cases of priors_remaining.npz
    (the ``*_empirical`` names the hook takes): log-density, gradient, hyper value, hyper log-density and the
    hyper-parameter's gradient, at the tolerances test_priors.py holds the modules to"""
    z = np.load(os.path.join(golden_dir, "priors.npz"))
    keys = sorted({k.rsplit("|", 1)[0] for k in z.files})
    assert len(keys) == 96
    linked = 0
    for key in keys:
        name, extra, _, loc, scale, dt = key.split("|")
        tol = dict(rel=2e-5, abs=2e-5) if dt == "float32" else dict(rel=1e-11, abs=1e-11)
        weight, hyper = _spec_of_fixture(name, extra, float(loc), float(scale))
        s = float(z[key + "|hyper_p"]) if hyper is not None else None
        lp, grad, x, lp_h, grad_h = _reference_of_fixture(weight, hyper, z[key + "|theta"].astype(np.float64).reshape(-1),
                                                          s, R.unit_roundoff(dt))
        assert lp == pytest.approx(float(z[key + "|log_prob"]), **tol), key
        np.testing.assert_allclose(grad, z[key + "|grad_theta"].astype(np.float64).reshape(-1), rtol=tol["rel"] * 5,
                                   atol=tol["abs"], err_msg=key)
        if hyper is not None:
            linked += 1
            assert x == pytest.approx(float(z[key + "|hyper_value"]), **tol), key
            assert lp_h == pytest.approx(float(z[key + "|hyper_log_prob"]), **tol), key
            assert grad_h == pytest.approx(float(z[key + "|grad_hyper"]), rel=tol["rel"] * 20, abs=tol["abs"] * 20), key
    assert linked == 48
    z = np.load(os.path.join(golden_dir, "priors_remaining.npz"))
    keys = sorted({k.rsplit("|", 1)[0] for k in z.files if k.split("|")[0] in ("gaussian_empirical", "laplace_empirical")})
    assert len(keys) == 16
    for key in keys:
        name, loc, scale, _, _, dt = key.split("|")
        tol = dict(rel=3e-5, abs=3e-5) if dt == "float32" else dict(rel=1e-10, abs=1e-10)
        weight, hyper = _spec_of_fixture(name, "", float(loc), float(scale))
        lp, grad, x, lp_h, grad_h = _reference_of_fixture(weight, hyper, z[key + "|param:p"].astype(np.float64).reshape(-1),
                                                          float(z[key + "|param:scale.p"]), R.unit_roundoff(dt))
        assert lp + lp_h == pytest.approx(float(z[key + "|log_prior"]), **tol), key
        np.testing.assert_allclose(grad, z[key + "|grad:p"].astype(np.float64).reshape(-1), rtol=tol["rel"] * 10,
                                   atol=tol["abs"] * 10, err_msg=key)
        assert grad_h == pytest.approx(float(z[key + "|grad:scale.p"]), rel=tol["rel"] * 10, abs=tol["abs"] * 10), key


def test_emulated_fp32_arithmetic_stays_inside_the_bounds():
    "the budgets on a numpy restatement of the kernel's fp32 arithmetic, edge values included: worst error / bound <= 1"
    rng = np.random.default_rng(11)
    worst = {}
    for si, (loc, scale, df, N) in enumerate(SETTINGS):
        for kind in (R.NORMAL, R.STUDENT_T, R.CAUCHY):
            theta = _theta(rng, 20000, loc, kind, "float32", wide=True)
            g = _g(rng, 20000, "float32")
            ref = R.elementwise(kind, loc, scale, df, N, theta, g, R.U32)
            ratio, _ = R.check_gradient(R.emulate_fp32(kind, loc, scale, df, N, theta, g), ref, R.U32, f"{NAMES[kind]} {si}")
            worst[NAMES[kind]] = max(worst.get(NAMES[kind], 0.0), ratio)
    print("prior-ratios", json.dumps({"test": "emulation", "worst": worst}))
    assert all(0.05 < w <= 1.0 for w in worst.values()), worst       # (a bound 20x too wide would be no test either)


OLD = dict(rtol=1e-4, atol=2e-6)      # test_fused_prior_hook_matches_reference_fixtures, float32


def _passes_old(got, want):
    return bool(np.all(np.abs(np.asarray(got, np.float64) - want) <= OLD["atol"] + OLD["rtol"] * np.abs(want)))


def test_wrong_kernels_pass_the_old_tolerances_and_fail_the_bounds():
    """the gap this file closes, stated on numpy emulations of five deliberately wrong kernels: each one is accepted by
    rtol = 1e-4, atol = 2e-6 (log-prior: rel = 1e-5), the tolerances the fixtures are held to, and rejected by the bound"""
    rng = np.random.default_rng(5)
    loc, scale, df, N = SETTINGS[4]
    n = 4097                                                     # a ragged last item
    theta = (loc + scale * rng.standard_normal(n)).astype(np.float32)
    g = _g(rng, n, "float32")
    ref = R.elementwise(R.NORMAL, loc, scale, df, N, theta, g, R.U32)
    R.check_gradient(R.emulate_fp32(R.NORMAL, loc, scale, df, N, theta, g), ref, R.U32, "the right kernel")

    # 1. the coefficient off by 3e-5 relative (Student-t at N = 123: the prior term is a visible part of g')
    loc1, scale1, df1, N1 = SETTINGS[0]
    theta1 = (loc1 + scale1 * rng.standard_normal(n)).astype(np.float32)
    ref1 = R.elementwise(R.STUDENT_T, loc1, scale1, df1, N1, theta1, g, R.U32)
    R.check_gradient(R.emulate_fp32(R.STUDENT_T, loc1, scale1, df1, N1, theta1, g), ref1, R.U32, "the right kernel")
    for kind, rf, args in ((R.NORMAL, R.elementwise(R.NORMAL, loc1, scale1, df1, N1, theta1, g, R.U32), (loc1, scale1, df1, N1)),
                           (R.STUDENT_T, ref1, (loc1, scale1, df1, N1))):
        wrong = R.emulate_fp32(kind, *args, theta1, g, coefficient_error=3e-5)
        assert _passes_old(wrong, rf["g"])
        with pytest.raises(AssertionError, match="outside"):
            R.check_gradient(wrong, rf, R.U32, "coefficient")

    # 2. the last element of the ragged item left unchanged
    wrong = R.emulate_fp32(R.NORMAL, loc, scale, df, N, theta, g)
    wrong[-1] = g[-1]
    assert _passes_old(wrong, ref["g"]) and wrong[-1] != np.float32(ref["g"][-1])
    with pytest.raises(AssertionError, match=f"element {n - 1}.*1 of {n} outside"):
        R.check_gradient(wrong, ref, R.U32, "ragged")

    # 3. the log-density accumulated in fp32 (serially, as one thread would)
    with np.errstate(all="ignore"):
        z = (theta.astype(np.float64) - loc) / scale
    acc = np.float32(0)
    for t in (-0.5 * z * z).astype(np.float32):
        acc = np.float32(acc + t)
    wrong_lp = float(acc) + n * ref["log_norm"]
    assert wrong_lp == pytest.approx(ref["logp"], rel=1e-5)
    with pytest.raises(AssertionError, match="bound"):
        R.check_logp(wrong_lp, ref["logp"], R.logp_bound(ref), "fp32 accumulation")
    R.check_logp(float(np.sum(-0.5 * z * z)) + n * ref["log_norm"], ref["logp"], R.logp_bound(ref), "fp64 accumulation")

    # 4. the log-normaliser counted for numel - 1 elements (a segment large enough for rel = 1e-5 to lose one element)
    big = 1 << 19
    theta4 = (loc + scale * rng.standard_normal(big)).astype(np.float32)
    ref4 = R.elementwise(R.NORMAL, loc, scale, df, N, theta4, np.ones(big), R.U32)
    wrong_lp = ref4["logp"] - ref4["log_norm"]
    assert wrong_lp == pytest.approx(ref4["logp"], rel=1e-5)
    with pytest.raises(AssertionError, match="bound"):
        R.check_logp(wrong_lp, ref4["logp"], R.logp_bound(ref4), "normaliser")

    # 5. the chain-rule sum of a 39-chunk segment missing one chunk
    _, _, _, N5 = SETTINGS[3]
    s, hyper = 1.0, (R.GAMMA_SOFTPLUS, 1.3, 2.5)
    x, _, rel = R.hyper_value(*hyper, s)
    theta5 = (loc + x * rng.standard_normal(39200)).astype(np.float32)
    w = R.elementwise(R.NORMAL, loc, x, 0.0, N5, theta5, np.ones(39200), R.U32, scale_rel=rel)
    h = R.hyper_segment(*hyper, s, N5, 10.0, R.U32, chains=[w])
    dropped = R.elementwise(R.NORMAL, loc, x, 0.0, N5, theta5[38 * 1024:], np.ones(39200 - 38 * 1024), R.U32)["dls"]
    wrong_gh = float(np.float32(h["g"] + dropped * h["dxds"] / N5))
    assert abs(dropped) > 1.0 and _passes_old(wrong_gh, h["g"])
    assert abs(float(np.float32(h["g"])) - h["g"]) <= h["bound"] < abs(wrong_gh - h["g"])


# ===================================================================================================== inputs
def _np_dtype(dtype):
    return np.float32 if dtype == "float32" else np.float64


def _g(rng, n, dtype):
    "standard normal in the working precision, no zeros of either sign"
    g = rng.standard_normal(n).astype(_np_dtype(dtype))
    g[g == 0] = 1
    return g


def _theta(rng, n, loc, kind, dtype, wide, plant_at=None, huge=True):
    """a mixture of scales 1e-3, 1, 30, 1e6 around loc (``wide``; else 1e-3 and 1 only, so that a sum over the segment is
    not a sum of its largest element alone), with theta = loc, loc +- 1 ulp and (``wide``) +-1e19, +-3e30 / +-1e160 planted;
    a segment too short for all of them takes the one named by ``plant_at``.  LAPLACE / GENNORM with a loc that is no number
    of the working precision: no element closer to loc than 2^-22 |loc| (the sign of theta - loc is then the exact one)."""
    npdt = _np_dtype(dtype)
    scales = np.array([1e-3, 1.0, 30.0, 1e6] if wide else [1e-3, 1.0])
    theta = (loc + rng.standard_normal(n) * rng.choice(scales, n)).astype(npdt)
    loc_t = npdt(loc)
    plants = [loc_t, np.nextafter(loc_t, npdt(np.inf)), np.nextafter(loc_t, npdt(-np.inf))]
    if wide and huge:
        plants += [npdt(v) for v in ((1e19, -1e19, 3e30, -3e30) if dtype == "float32" else (1e19, -1e19, 1e160, -1e160))]
    if n >= 4 * len(plants):
        where = rng.choice(n - 2, len(plants) - 2, replace=False) + 1
        theta[where] = plants[2:]
        theta[0], theta[-1] = plants[0], plants[1]           # the first element and the last (ragged) one are edge values
    else:
        theta[(plant_at or 0) % n] = plants[(plant_at or 0) % len(plants)]
    if kind in (R.LAPLACE, R.GENNORM) and float(loc_t) != loc:
        near = np.abs(theta.astype(np.float64) - loc) <= 2.0 ** -22 * abs(loc)
        theta[near] = npdt(loc * (1 + 2.0 ** -18))
    return theta


class Arena:
    """segments as 16-byte-aligned views into NaN-filled parameter and gradient buffers, one Engine over them.
    ``gradless``: indices of segments whose ``.grad`` stays None."""

    def __init__(self, sizes, dtype, chunk, gradless=()):
        self.dtype, self.sizes, self.gradless = dtype, list(sizes), set(gradless)
        tdt = torch.float32 if dtype == "float32" else torch.float64
        off, self.offsets = 8, []
        for n in sizes:
            self.offsets.append(off)
            off = -(-(off + n) // 4) * 4 + 4               # the next multiple of 4 elements, then 4 more of padding
        self.total = off + 4
        self.theta_buf = torch.full((self.total,), float("nan"), dtype=tdt, device="cuda")
        self.g_buf = torch.full((self.total,), float("nan"), dtype=tdt, device="cuda")
        self.params = [self.theta_buf[o:o + n] for o, n in zip(self.offsets, sizes)]
        assert all(p.data_ptr() % 16 == 0 for p in self.params)
        self.inside = np.zeros(self.total, dtype=bool)
        for o, n in zip(self.offsets, sizes):
            self.inside[o:o + n] = True
        from bnn_priors_amd.mcmc.engine import Engine
        self.engine = Engine([{"params": self.params}], seed=7, chunk_elems=chunk)
        assert not self.engine._unaligned

    def load(self, thetas, gs):
        "write the segments' values (numpy arrays of the working precision) and bind the gradients"
        th, g = np.full(self.total, np.nan, dtype=_np_dtype(self.dtype)), np.full(self.total, np.nan, dtype=_np_dtype(self.dtype))
        for o, n, a, b in zip(self.offsets, self.sizes, thetas, gs):
            th[o:o + n], g[o:o + n] = a, b
        self.theta_buf.copy_(torch.from_numpy(th))
        self.g_buf.copy_(torch.from_numpy(g))
        for i, (p, o, n) in enumerate(zip(self.params, self.offsets, self.sizes)):
            p.grad = None if i in self.gradless else self.g_buf[o:o + n]
        self.theta0, self.g0 = th, g

    def table(self, specs, links=None, filters=None):
        self.engine.set_priors(specs, links, filters)
        self.engine.refresh([1.0] * len(self.params), raise_on_no_grad=False)
        assert not self.engine._unaligned

    def read(self):
        torch.cuda.synchronize()
        return self.theta_buf.cpu().numpy(), self.g_buf.cpu().numpy()

    def seg(self, flat, i):
        return flat[self.offsets[i]:self.offsets[i] + self.sizes[i]]

    def log_priors(self):
        "(per-segment log-prior, total, per-chunk partials [n_chunks, 8])"
        eng = self.engine
        eng._touch()
        return (eng.fetch_state()[:, _hip.SEG_STATE_FIELDS.index("aux")].copy(), float(eng.log_prior_total().item()),
                eng.partials.cpu().numpy().reshape(-1, _hip.PSTRIDE))

    def chunks_of(self, i):
        first = int(self.engine.seg_host["first_chunk"][i])
        return range(first, first + max(1, -(-self.sizes[i] // self.engine.chunk)))


def same_number(a, b):
    "equal, or both NaN"
    return a == b or (math.isnan(a) and math.isnan(b))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} elements differ, first at " \
                                                        f"{np.flatnonzero(a != b)[:8]}"


class Worst:
    "the worst error / bound per key, with the case that produced it"

    def __init__(self, test):
        self.test, self.worst = test, {}

    def add(self, key, ratio, case):
        if ratio >= self.worst.get(key, (-1.0, None))[0]:
            self.worst[key] = (round(ratio, 4), case)

    def report(self):
        print("prior-ratios", json.dumps({"test": self.test, "worst": self.worst}))


# the table of the family tests: SIZES with a PRIOR_NONE segment and a segment without gradient in between
I_NONE, I_GRADLESS = 3, 9
FAMILY_SIZES = SIZES[:I_NONE] + [11] + SIZES[I_NONE:I_GRADLESS - 1] + [9] + SIZES[I_GRADLESS - 1:]
assert len(FAMILY_SIZES) == len(SIZES) + 2 and FAMILY_SIZES[I_NONE] == 11 and FAMILY_SIZES[I_GRADLESS] == 9
I_EXTRA = len(FAMILY_SIZES)             # the appended 6-element GENNORM segment that forces the full kernel


def _family_inputs(rng, sizes, kinds, loc, dtype, wide):
    thetas = [_theta(rng, n, loc, k, dtype, wide=wide if isinstance(wide, bool) else wide[i], plant_at=i)
              for i, (n, k) in enumerate(zip(sizes, kinds))]
    return thetas, [_g(rng, n, dtype) for n in sizes]


def _kinds_of(rot, families, n_seg):
    kinds = [families[(i + rot) % len(families)] for i in range(n_seg)]
    kinds[I_NONE] = R.NONE
    return kinds


def _specs(kinds, loc, scale, df, beta):
    return [None if k == R.NONE else (k, loc, scale, beta if k == R.GENNORM else df) for k in kinds]


def _check_untouched(arena, th, g, kinds, what):
    "theta entirely, the padding of g, and g of the PRIOR_NONE and grad-less segments: the bits they had"
    assert_same_bits(th, arena.theta0, f"{what}: theta")
    assert_same_bits(g[~arena.inside], arena.g0[~arena.inside], f"{what}: padding of g")
    for i, k in enumerate(kinds):
        if k == R.NONE or i in arena.gradless:
            assert_same_bits(arena.seg(g, i), arena.seg(arena.g0, i), f"{what}: g of segment {i}")


# ===================================================================================================== GPU: families
@GPU
@pytest.mark.parametrize("route", ["lean", "full"])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_scale_kinds_match_the_reference(dtype, chunk, route):
    """kinds 1-5 at constant scale, every family at every segment size under every setting: each element's gradient within
    its family's bound, each segment's log-prior and the total within numel * 2^-50 of the reference.  ``lean``:
    prior_kernel<T, false> (kinds 1-4); ``full``: prior_kernel<T, true>, forced by one GENNORM segment appended to the
    table (kinds 1-5)."""
    u = R.unit_roundoff(dtype)
    full = route == "full"
    sizes = FAMILY_SIZES + ([6] if full else [])
    families = [R.NORMAL, R.LAPLACE, R.STUDENT_T, R.CAUCHY] + ([R.GENNORM] if full else [])
    arena = Arena(sizes, dtype, chunk, gradless=[I_GRADLESS])
    rng = np.random.default_rng(100 + 2 * DTYPES.index(dtype) + full)
    worst = Worst(f"constant-scale {dtype} chunk {chunk} {route}")
    for si, (loc, scale, df, N) in enumerate(SETTINGS):
        for rot in range(len(families)):
            kinds = _kinds_of(rot, families, len(sizes))
            if full:
                kinds[I_EXTRA] = R.GENNORM
            beta = BETAS[(si + rot) % len(BETAS)]
            # segments alternate between the wide mixture (with the huge values) and the narrow one, both for every family
            wide = [((i + rot // 2 + si) % 2 == 0) for i in range(len(sizes))]
            thetas, gs = _family_inputs(rng, sizes, kinds, loc, dtype, wide)
            arena.load(thetas, gs)
            arena.table(_specs(kinds, loc, scale, df, beta))
            assert bool(arena.engine.prior_flags() & _hip.PRIOR_FULL) == full
            arena.engine.prior_grad(N, True)
            th, g = arena.read()
            what = f"setting {si} rotation {rot}"
            _check_untouched(arena, th, g, kinds, what)
            per_seg, total, partials = arena.log_priors()
            assert per_seg[I_NONE] == 0.0
            assert all(partials[c, 6] == 0.0 for c in arena.chunks_of(I_GRADLESS)), what
            want_total, n_total, own_total = [], 0, 0.0
            for i, k in enumerate(kinds):
                if k == R.NONE:
                    continue
                if i == I_GRADLESS:
                    # (no gradient: no element is evaluated; the kernel reports the normaliser alone, which this file
                    # does not pin -- it enters the expected total as reported)
                    want_total.append(per_seg[i])
                    continue
                ref = R.elementwise(k, loc, scale, beta if k == R.GENNORM else df, N, thetas[i], gs[i], u)
                case = f"{what} segment {i} ({sizes[i]} elements, {'wide' if wide[i] else 'narrow'})"
                ratio, idx = R.check_gradient(arena.seg(g, i), ref, u, f"{NAMES[k]} {case}")
                worst.add(NAMES[k], ratio, f"{case} element {idx}" + (f" beta {beta}" if k == R.GENNORM else ""))
                ratio = R.check_logp(float(per_seg[i]), ref["logp"], R.logp_bound(ref), f"log-prior of {NAMES[k]} {case}")
                worst.add("log-prior " + NAMES[k], ratio, case)
                want_total.append(ref["logp"])
                n_total += sizes[i]
                own_total += ref["logp_own"]
            want = math.fsum(want_total) if np.isfinite(want_total).all() else float(np.sum(want_total))
            worst.add("log-prior total", R.check_logp(total, want, n_total * R.LOGP_REL_PER_ELEMENT * abs(want) + own_total,
                                                      f"total log-prior, {what}"), what)
    worst.report()


@GPU
@pytest.mark.parametrize("dtype", DTYPES)
def test_gennorm_at_its_location_has_the_closed_forms_nan_pattern(dtype):
    "theta == loc: sign(0) * 0^(beta - 1) is 0 * inf = NaN for beta < 1, 0 * 1 = 0 at beta = 1, 0 beyond"
    u, loc, scale, N = R.unit_roundoff(dtype), 0.25, 0.7, 123.0
    arena = Arena([7] * len(BETAS), dtype, _hip.CHUNK_SMALL)
    rng = np.random.default_rng(3)
    thetas = [_theta(rng, 7, loc, R.GENNORM, dtype, wide=False) for _ in BETAS]
    for t in thetas:
        t[[0, 3, 6]] = loc
    gs = [_g(rng, 7, dtype) for _ in BETAS]
    arena.load(thetas, gs)
    arena.table([(R.GENNORM, loc, scale, b) for b in BETAS])
    arena.engine.prior_grad(N, True)
    th, g = arena.read()
    for i, b in enumerate(BETAS):
        ref = R.elementwise(R.GENNORM, loc, scale, b, N, thetas[i], gs[i], u)
        assert np.isnan(ref["g"][[0, 3, 6]]).all() == (b < 1) and np.isnan(ref["g"]).sum() == (3 if b < 1 else 0)
        R.check_gradient(arena.seg(g, i), ref, u, f"beta {b}")
        if b >= 1:
            assert_same_bits(arena.seg(g, i)[[0, 3, 6]], gs[i][[0, 3, 6]], f"beta {b}: g at theta == loc")


# ===================================================================================================== GPU: hierarchical
S_VALUES = [-20.0, -5.0, -1.0, 0.0, 1.0, 5.0, 20.0, 29.5, 30.5, 40.0]
HYPER_ROWS = {R.GAMMA_SOFTPLUS: (1.3, 2.5), R.UNIFORM_CDF: (0.05, 2.5), R.HALFCAUCHY_SOFTPLUS: (0.7, 1.0),
              R.IMPROPER_SOFTPLUS: (0.0, 1.0)}
# the weight kinds each hyper kind occurs with in the original table (gaussian_gamma, laplace_gamma, student-t_gamma,
# *_uniform, horseshoe, gaussian_empirical, laplace_empirical)
PAIRS = {R.GAMMA_SOFTPLUS: [R.NORMAL, R.LAPLACE, R.STUDENT_T], R.UNIFORM_CDF: [R.NORMAL, R.LAPLACE, R.STUDENT_T],
         R.HALFCAUCHY_SOFTPLUS: [R.NORMAL], R.IMPROPER_SOFTPLUS: [R.NORMAL, R.LAPLACE]}
N_WEIGHT = 784 * 50


def _linked_layout(hyper_first):
    "(sizes, index of: big weight, its hyper, small weight, its hyper): one hyper before, the other after its weights"
    if hyper_first:
        return [1, N_WEIGHT, 7, 1], (1, 0, 2, 3)
    return [N_WEIGHT, 1, 1, 7], (0, 1, 3, 2)


@GPU
@pytest.mark.parametrize("hyper_kind", sorted(PAIRS), ids=lambda k: NAMES[k])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hierarchical_scales_match_the_reference(dtype, hyper_kind):
    """a 784 x 50 weight segment (39 / 10 chunks) and a 7-element one, each linked to a one-element hyper segment of
    ``hyper_kind``: weight gradient, hyper gradient (own density + the chain-rule sum over all chunks, onto a nonzero g_h),
    the value-dependent normaliser and both log-densities, at both chunk sizes -- whose hyper gradients must agree within
    the chain-rule budget"""
    u, npdt = R.unit_roundoff(dtype), _np_dtype(dtype)
    h_loc, h_scale = HYPER_ROWS[hyper_kind]
    rng = np.random.default_rng(200 + hyper_kind)
    worst = Worst(f"hierarchical {dtype} {NAMES[hyper_kind]}")
    arenas = {(c, first): Arena(_linked_layout(first)[0], dtype, c) for c in CHUNKS for first in (True, False)}
    for wi, kind in enumerate(PAIRS[hyper_kind]):
        loc, _, df, N = SETTINGS[(wi + hyper_kind) % len(SETTINGS)]
        theta_big = _theta(rng, N_WEIGHT, loc, kind, dtype, wide=True, huge=False)
        theta_small = _theta(rng, 7, loc, kind, dtype, wide=False, plant_at=wi)
        g_big, g_small = _g(rng, N_WEIGHT, dtype), _g(rng, 7, dtype)
        for k, s in enumerate(S_VALUES):
            first = (k + wi) % 2 == 0
            sizes, (iw, ih, jw, jh) = _linked_layout(first)
            s_small = S_VALUES[(k + 3) % len(S_VALUES)]
            gh0 = {ih: npdt(0.75), jh: npdt(-1.25)}
            thetas, gs = [None] * 4, [None] * 4
            thetas[iw], thetas[jw], thetas[ih], thetas[jh] = theta_big, theta_small, np.array([s], npdt), np.array([s_small], npdt)
            gs[iw], gs[jw], gs[ih], gs[jh] = g_big, g_small, np.array([gh0[ih]]), np.array([gh0[jh]])
            specs, links = [None] * 4, [None] * 4
            specs[iw] = specs[jw] = (kind, loc, float("nan"), df)
            specs[ih] = specs[jh] = (hyper_kind, h_loc, h_scale, 0.0)
            links[iw], links[jw] = ih, jh
            refs = {}
            for w, h, sv in ((iw, ih, s), (jw, jh, s_small)):
                x, _, rel = R.hyper_value(hyper_kind, h_loc, h_scale, sv)
                refs[w] = R.elementwise(kind, loc, x, df, N, thetas[w], gs[w], u, scale_rel=rel)
                refs[h] = R.hyper_segment(hyper_kind, h_loc, h_scale, sv, N, float(gh0[h]), u, chains=[refs[w]])
            gh_by_chunk = {}
            for chunk in CHUNKS:
                arena = arenas[chunk, first]
                arena.load(thetas, gs)
                arena.table(specs, links)
                assert arena.engine.prior_flags() & _hip.PRIOR_HAS_LINKS
                arena.engine.prior_grad(N, True)
                th, g = arena.read()
                what = f"{NAMES[kind]} s = {s} / {s_small} chunk {chunk} hyper {'before' if first else 'after'}"
                _check_untouched(arena, th, g, [kind] * 4, what)
                per_seg, total, _ = arena.log_priors()
                for w, h in ((iw, ih), (jw, jh)):
                    ratio, idx = R.check_gradient(arena.seg(g, w), refs[w], u, f"weights ({sizes[w]}) {what}")
                    worst.add("weights " + NAMES[kind], ratio, f"{what} ({sizes[w]} elements) element {idx}")
                    got_h = float(arena.seg(g, h)[0])
                    err, bound = abs(got_h - refs[h]["g"]), refs[h]["bound"]
                    assert err <= bound, f"hyper gradient ({sizes[w]} weights) {what}: got {got_h!r}, want " \
                                         f"{refs[h]['g']!r}, |error| {err:.3e} > bound {bound:.3e}"
                    worst.add("hyper gradient " + NAMES[kind], err / bound, f"{what} ({sizes[w]} weights)")
                    worst.add("log-prior weights " + NAMES[kind],
                              R.check_logp(float(per_seg[w]), refs[w]["logp"], R.linked_logp_bound(refs[w]),
                                           f"weights' log-prior ({sizes[w]}) {what}"), what)
                    R.check_logp(float(per_seg[h]), refs[h]["logp"], refs[h]["logp_bound"], f"hyper log-prior {what}")
                want = math.fsum(r["logp"] for r in refs.values())
                R.check_logp(total, want, sum(R.linked_logp_bound(refs[w]) for w in (iw, jw))
                             + sum(refs[h]["logp_bound"] for h in (ih, jh)), f"total log-prior {what}")
                gh_by_chunk[chunk] = float(arena.seg(g, ih)[0])
                if k == 4:       # the same table once more: the same bits, log-prior included
                    arena.load(thetas, gs)
                    arena.engine.prior_grad(N, True)
                    _, g2 = arena.read()
                    assert_same_bits(g2, g, f"second run, {what}")
                    per_seg2, total2, _ = arena.log_priors()
                    assert_same_bits(per_seg2, per_seg, f"second run's log-priors, {what}")
                    assert total2 == total
            # two tables that differ only in the chunk size sum 39 / 10 partials: their hyper gradients differ by no more
            # than the two accumulations' budget plus one rounding of the result each
            w = refs[iw]
            budget = 2 * R.SAFETY * w["numel"] * R.U64 * w["dls_abs"] * abs(refs[ih]["dxds"]) / N + 2 * u * abs(refs[ih]["g"])
            assert abs(gh_by_chunk[CHUNKS[0]] - gh_by_chunk[CHUNKS[1]]) <= budget, (NAMES[kind], s, gh_by_chunk, budget)
    worst.report()


# ===================================================================================================== GPU: routes
ROUTES = ["lean", "full", "inline", "reduce", "reduce-indirect"]
A_MOM, LR = 0.9, 1e-3


def _scalars(kind, phase, N):
    "the transition's scalars as the samplers form them (SURVEY.md Appendix A), a = 0.9, T = 1"
    base = dict(num_data=N, b2h2=LR / N, bh=math.sqrt(LR / N), bhn=math.sqrt(LR * N), rmsprop_alpha=0.99)
    if kind == _hip.VERLET:
        row = {"initial": (A_MOM ** .5, 1.0, (1 - A_MOM) ** .5), "step": (A_MOM, 1 + A_MOM, (1 - A_MOM ** 2) ** .5),
               "final": (A_MOM ** .5, A_MOM ** .5, (1 - A_MOM) ** .5)}[phase]
    elif kind == _hip.HMC:
        row = (1.0, 1.0 if phase == "step" else 0.5, 0.0)
    else:
        row = (A_MOM, 1.0, (2 * (1 - A_MOM)) ** .5)
    return dict(base, mom_decay=row[0], grad_v=row[1], noise_std=row[2])


PHASES = [("initial", _hip.INITIAL | _hip.SAVE_STATE, True), ("step", 0, False), ("final", _hip.FINAL, True)]


def _run_route(route, chunk, kind, kinds, setting, inputs, clamp):
    """three transitions (initial with SAVE_STATE and metrics, plain, final with metrics) of one route on its own arena;
    -> per phase: dict of g, theta, m, v (and prev_*), per-segment log-priors and their total"""
    loc, scale, df, N = setting
    thetas, g_steps, m0, v0 = inputs
    sizes = FAMILY_SIZES + [6]
    arena = Arena(sizes, "float32", chunk, gradless=[I_GRADLESS])
    eng = arena.engine
    kinds = list(kinds)
    kinds[I_EXTRA] = R.GENNORM if route == "full" else R.NONE
    specs = _specs(kinds, loc, scale, df, 1.7)
    eng.m.copy_(torch.from_numpy(m0))
    eng.v.copy_(torch.from_numpy(v0))
    eng.momentum_ready = True
    out = []
    for step, ((phase, flags, metrics), gs) in enumerate(zip(PHASES, g_steps)):
        sc = _scalars(kind, phase, N)
        if step == 0:
            arena.load(thetas, gs)
        else:       # theta has moved: only the likelihood gradient is new
            flat = arena.g0.copy()
            for o, n, b in zip(arena.offsets, arena.sizes, gs):
                flat[o:o + n] = b
            arena.g_buf.copy_(torch.from_numpy(flat))
            arena.g0 = flat
        arena.table(specs)
        full_flags = flags | (_hip.CALC_METRICS if metrics else 0)
        if route in ("lean", "full"):
            assert bool(eng.prior_flags()) == (route == "full")
            eng.prior_grad(N, metrics)
            eng.step(0, kind, full_flags, step, grad_clamp=clamp, **sc)
        elif route == "inline":
            eng.ensure_prev()
            A = eng.make_args(0, kind, full_flags | _hip.INLINE_PRIOR | (_hip.WITH_LOG_PRIOR if metrics else 0), step,
                              grad_clamp=clamp, **sc)
            assert A.flags & _hip.SMALL_FINALIZE
            A_dev = torch.frombuffer(bytearray(bytes(A)), dtype=torch.uint8).cuda()
            eng.step_indirect(A, A_dev.data_ptr())
        else:
            # the dense path: the likelihood gradient arrives as ONE slice of partials laid out at noise_base; p.grad is
            # written, not read
            base = eng.seg_host["noise_base"]
            stride = int(base[-1]) + -(-sizes[-1] // 4) * 4
            part = np.full(stride, np.nan, dtype=np.float32)
            for i, (n, b) in enumerate(zip(sizes, gs)):
                part[int(base[i]):int(base[i]) + n] = b
            gpart = torch.from_numpy(part).cuda()
            keep = arena.g_buf.clone()
            arena.g_buf.fill_(float("nan"))
            o, n = arena.offsets[I_GRADLESS], sizes[I_GRADLESS]
            arena.g_buf[o:o + n] = keep[o:o + n]
            ones = torch.ones(1, device="cuda")
            indirect = route == "reduce-indirect"
            eng.ensure_prev()
            A = eng.make_args(0, kind, full_flags | (_hip.WITH_LOG_PRIOR if metrics and indirect else 0), step,
                              grad_clamp=clamp, **sc)
            A_dev = torch.frombuffer(bytearray(bytes(A)), dtype=torch.uint8).cuda()
            _hip.check(eng.lib.sgmcmc_grad_reduce_prior(ctypes.byref(eng.layout), gpart.data_ptr(), 1, stride, ones.data_ptr(),
                                                        ones.data_ptr(), 1, N, _hip.CALC_METRICS if metrics else 0,
                                                        A_dev.data_ptr() if indirect else None, eng.stream()),
                       "sgmcmc_grad_reduce_prior")
            _hip.check(eng.lib.sgmcmc_step(ctypes.byref(eng.layout), ctypes.byref(A), eng.stream()), "sgmcmc_step")
            eng._touch()
        th, g = arena.read()
        assert_same_bits(th[~arena.inside], arena.theta0[~arena.inside], f"{route}, transition {step}: padding of theta")
        assert_same_bits(g[~arena.inside], arena.g0[~arena.inside], f"{route}, transition {step}: padding of g")
        res = dict(theta=th, g=g, m=eng.m.cpu().numpy(), v=eng.v.cpu().numpy())
        if phase == "initial":
            res.update(prev_theta=eng.prev_theta.cpu().numpy(), prev_g=eng.prev_g.cpu().numpy(), prev_m=eng.prev_m.cpu().numpy())
        if metrics:
            res["per_seg"], res["total"], _ = arena.log_priors()
        out.append(res)
    return arena, out


def _route_inputs(rng, kinds, loc, chunk):
    sizes = FAMILY_SIZES + [6]
    wide = [i % 2 == 0 for i in range(len(sizes))]
    thetas, _ = _family_inputs(rng, sizes, kinds, loc, "float32", wide)
    g_steps = [[_g(rng, n, "float32") for n in sizes] for _ in PHASES]
    n_arena = sum(max(1, -(-n // chunk)) for n in sizes) * chunk
    return thetas, g_steps, rng.standard_normal(n_arena).astype(np.float32), \
        (0.5 + rng.random(n_arena)).astype(np.float32)


def _compare_routes(arena, a, b, what):
    "everything the transitions wrote, bit for bit, outside the appended segment (GENNORM in the full route's table)"
    keep = np.ones(arena.total, dtype=bool)
    keep[arena.offsets[I_EXTRA]:arena.offsets[I_EXTRA] + 6] = False
    chunk = arena.engine.chunk
    arena_keep = np.ones(a[0]["m"].size, dtype=bool)
    arena_keep[int(arena.engine.seg_host["first_chunk"][I_EXTRA]) * chunk:] = False
    for step, (ra, rb) in enumerate(zip(a, b)):
        for name in ("theta", "g"):
            assert_same_bits(ra[name][keep], rb[name][keep], f"{what}, transition {step}: {name}")
        for name in ("m", "v", "prev_theta", "prev_g", "prev_m"):
            if name in ra:
                assert_same_bits(ra[name][arena_keep], rb[name][arena_keep], f"{what}, transition {step}: {name}")
        if "per_seg" in ra:
            pa, pb = np.delete(ra["per_seg"], I_EXTRA), np.delete(rb["per_seg"], I_EXTRA)
            assert np.array_equal(np.isfinite(pa), np.isfinite(pb)), what
            np.testing.assert_allclose(pb, pa, rtol=1e-14, atol=0, err_msg=f"{what}, transition {step}: per-segment log-prior")
            ta, tb = ra["total"] - ra["per_seg"][I_EXTRA], rb["total"] - rb["per_seg"][I_EXTRA]
            # (the appended segment's log-prior is exactly 0 unless it is the full route's GENNORM one, whose 6 elements
            # are of order 1 against a total of order 1e60: the subtraction is exact or far below 1e-14)
            assert (abs(tb - ta) <= 1e-14 * abs(ta) if math.isfinite(ta) else same_number(ta, tb)), \
                f"{what}, transition {step}: total log-prior {ta!r} / {tb!r}"


@GPU
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind,clamp", [(_hip.VERLET, 0.0), (_hip.HMC, 0.0), (_hip.SGLD, 0.0), (_hip.VERLET, 0.75)],
                         ids=["verlet", "hmc", "sgld", "verlet-clamped"])
def test_every_route_gives_the_same_bits(kind, clamp, chunk):
    """prior_kernel<float, false> + sgmcmc_step, prior_kernel<float, true> + sgmcmc_step, the in-flight prior of
    sgmcmc_step_indirect (SGMCMC_INLINE_PRIOR, log-prior finished by the small finalize) and sgmcmc_grad_reduce_prior
    (scalars by value and from device memory) + sgmcmc_step on clones of one input, kinds 1-4 in float32: p.grad, theta, m,
    v and the roll-back copies bit-identical after an initial (SAVE_STATE), a plain and a final transition; the log-priors
    to 1e-14 (the two finalize kernels sum a segment's chunks in different orders)"""
    families = [R.NORMAL, R.LAPLACE, R.STUDENT_T, R.CAUCHY]
    rng = np.random.default_rng(300 + kind)
    for si, setting in enumerate(SETTINGS):
        kinds = _kinds_of(si, families, len(FAMILY_SIZES) + 1)
        inputs = _route_inputs(rng, kinds, setting[0], chunk)
        arena, first = _run_route(ROUTES[0], chunk, kind, kinds, setting, inputs, clamp)
        if clamp:       # the clamp bites: some |g'| of the first transition are beyond it
            g = first[0]["g"][arena.inside]
            assert np.sum(np.abs(g) > clamp) > 1000
        for route in ROUTES[1:]:
            _, other = _run_route(route, chunk, kind, kinds, setting, inputs, clamp)
            _compare_routes(arena, first, other, f"{route} against {ROUTES[0]}, setting {si}")


@GPU
@pytest.mark.parametrize("route", ROUTES)
def test_every_route_is_reproducible(route):
    "two runs of a route on the same input: identical bits, log-prior included"
    families = [R.NORMAL, R.LAPLACE, R.STUDENT_T, R.CAUCHY]
    rng = np.random.default_rng(400)
    kinds = _kinds_of(1, families, len(FAMILY_SIZES) + 1)
    inputs = _route_inputs(rng, kinds, SETTINGS[0][0], _hip.CHUNK_SMALL)
    arena, a = _run_route(route, _hip.CHUNK_SMALL, _hip.VERLET, kinds, SETTINGS[0], inputs, 0.0)
    _, b = _run_route(route, _hip.CHUNK_SMALL, _hip.VERLET, kinds, SETTINGS[0], inputs, 0.0)
    for step, (ra, rb) in enumerate(zip(a, b)):
        for name in ra:
            if name == "total":
                assert same_number(ra[name], rb[name]), (step, ra[name], rb[name])
            else:
                assert_same_bits(ra[name], rb[name], f"{route}, transition {step}: {name}")


@GPU
def test_lean_only_entry_points_refuse_what_they_do_not_implement():
    """SGMCMC_INLINE_PRIOR on a float64 layout, SGMCMC_INLINE_PRIOR and sgmcmc_grad_reduce_prior on a table whose
    prior_flags are not 0: hipErrorInvalidValue, nothing launched"""
    for dtype, specs, case in (("float64", [(R.NORMAL, 0.1, 0.7, 0.0)] * 2, "float64 layout"),
                               ("float32", [(R.NORMAL, 0.1, 0.7, 0.0), (R.GENNORM, 0.1, 0.7, 1.7)], "PRIOR_FULL table")):
        arena = Arena([1030, 7], dtype, _hip.CHUNK_SMALL)
        rng = np.random.default_rng(1)
        arena.load([_theta(rng, n, 0.1, R.NORMAL, dtype, wide=False) for n in arena.sizes], [_g(rng, n, dtype) for n in arena.sizes])
        arena.table(specs)
        eng = arena.engine
        assert (eng.layout.prior_flags != 0) == (dtype == "float32")
        eng.ensure_prev()
        A = eng.make_args(0, _hip.VERLET, _hip.INLINE_PRIOR, 0, **_scalars(_hip.VERLET, "step", 123.0))
        A_dev = torch.frombuffer(bytearray(bytes(A)), dtype=torch.uint8).cuda()
        rc = eng.lib.sgmcmc_step_indirect(ctypes.byref(eng.layout), ctypes.byref(A), A_dev.data_ptr(), eng.stream())
        assert rc == INVALID_VALUE, case
        if dtype == "float32":
            gpart = torch.ones(2048, device="cuda")
            rc = eng.lib.sgmcmc_grad_reduce_prior(ctypes.byref(eng.layout), gpart.data_ptr(), 1, 2048, gpart.data_ptr(),
                                                  gpart.data_ptr(), 1, 123.0, 0, None, eng.stream())
            assert rc == INVALID_VALUE, case
        th, g = arena.read()
        assert_same_bits(th, arena.theta0, f"{case}: theta")
        assert_same_bits(g, arena.g0, f"{case}: g")
        assert_same_bits(eng.m.cpu().numpy(), np.zeros(eng.m.numel(), _np_dtype(dtype)), f"{case}: m")


@GPU
@pytest.mark.parametrize("route", ["lean", "full"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nonfinite_parameter_touches_no_other_element(dtype, route):
    """one NaN and one +inf planted in every segment: every other element's gradient has the bits of the run without them;
    the segment's and the total log-prior are non-finite exactly when the reference's are"""
    u, full = R.unit_roundoff(dtype), route == "full"
    loc, scale, df, N = SETTINGS[0]
    kinds = [R.NORMAL, R.LAPLACE, R.STUDENT_T, R.CAUCHY] + ([R.GENNORM] if full else [])
    sizes = [4097, 1025, 5, 2 * 4096 + 6] + ([1023] if full else [])
    arena = Arena(sizes, dtype, _hip.CHUNK_SMALL)
    rng = np.random.default_rng(9)
    thetas, gs = _family_inputs(rng, sizes, kinds, loc, dtype, False)
    arena.load(thetas, gs)
    arena.table(_specs(kinds, loc, scale, df, 1.7))
    arena.engine.prior_grad(N, True)
    _, clean = arena.read()
    for i in range(len(sizes)):
        assert not np.array_equal(arena.seg(clean, i), gs[i])
    clean_lp, clean_total, _ = arena.log_priors()
    assert np.isfinite(clean_lp).all() and math.isfinite(clean_total)
    planted, where = [t.copy() for t in thetas], []
    for t in planted:
        i, j = (1, 3) if t.size < 8 else (t.size // 3, t.size - 2)
        t[i], t[j] = np.nan, np.inf
        where.append([i, j])
    arena.load(planted, gs)
    arena.engine.prior_grad(N, True)
    th, g = arena.read()
    _check_untouched(arena, th, g, kinds, "planted")
    per_seg, total, _ = arena.log_priors()
    want = []
    for i, k in enumerate(kinds):
        others = np.ones(sizes[i], dtype=bool)
        others[where[i]] = False
        assert_same_bits(arena.seg(g, i)[others], arena.seg(clean, i)[others], f"{NAMES[k]}: the other elements")
        ref = R.elementwise(k, loc, scale, 1.7 if k == R.GENNORM else df, N, planted[i], gs[i], u)
        assert not math.isfinite(ref["logp"])
        assert math.isfinite(per_seg[i]) == math.isfinite(ref["logp"]) and math.isnan(per_seg[i]) == math.isnan(ref["logp"])
        want.append(ref["logp"])
    assert math.isnan(total) == math.isnan(float(np.sum(want))) and not math.isfinite(total)


# ===================================================================================================== GPU: whitened kinds
# kinds 10 and 11 (FILTER_WHITENED, MULTIVARIATE_T) from raw tables against ``R.whitened`` at the stored values, held to
# the bounds of test_filter_prior.py / test_multivariate_t.py: fp64 gradient rtol 1e-10, atol 1e-12; fp32 gradient one
# rounding of the result with a safety factor of 2 on top of that allowance; log-priors rel 1e-11, abs 1e-9.
N_WHITENED = 37.0
FILTER_P = [1, 3, 9, _hip.FILTER_MAX_P]
# (name, base, beta, base_scale): GENNORM with beta on both sides of 1 and of 2, DOUBLE_GAMMA with concentration 1 and not 1
FILTER_BASES = [("normal", R.BASE_NORMAL, 2.0, 1.0), ("gennorm 0.7", R.BASE_GENNORM, 0.7, 0.8),
                ("gennorm 1.3", R.BASE_GENNORM, 1.3, 0.8), ("gennorm 2.5", R.BASE_GENNORM, 2.5, 1.2),
                ("laplace", R.BASE_LAPLACE, 1.0, 0.7), ("double-gamma 1", R.BASE_DOUBLE_GAMMA, 1.0, 0.6),
                ("double-gamma 0.62", R.BASE_DOUBLE_GAMMA, 0.62, 0.9), ("double-gamma 2.5", R.BASE_DOUBLE_GAMMA, 2.5, 0.5)]
MVT_DF = [2.001, 3.0, 1e4]
GENNORM_ROW = (R.GENNORM, 0.1, 0.7, 1.7)
I_W_NONE, I_W_GENNORM = 1, 3            # where the PRIOR_NONE and the element-wise GENNORM segment sit among the whitened ones


def _whitening(rng, P):
    "(mu [P], A [P, P], W = A^-1): theta_f = z A + mu, A = 0.3 (I + E) with |E| about 1/2 (condition number below ~3)"
    A = 0.3 * (np.eye(P) + 0.25 * rng.standard_normal((P, P)) / math.sqrt(P))
    return 0.05 * rng.standard_normal(P), A, np.linalg.inv(A)


def _filter_table(rng, P, base):
    _, kind, beta, base_scale = base
    mu, A, W = _whitening(rng, P)
    return dict(kind=R.FILTER_WHITENED, P=P, base=kind, beta=beta, base_scale=base_scale, mu=mu, W=W, A=A,
                lognorm=-0.5 * P * math.log(2.0 * math.pi) - float(np.linalg.slogdet(A)[1]))


def _mvt_table(rng, P, df, ev_size, ev_div, ev_mod):
    mu, A, W = _whitening(rng, P)
    lognorm = (math.lgamma((ev_size + df) / 2.0) - math.lgamma(df / 2.0) - (ev_size / 2.0) * math.log(math.pi * (df - 2.0))
               - (ev_size / P) * float(np.linalg.slogdet(A)[1]))
    return dict(kind=R.MULTIVARIATE_T, P=P, mu=mu, W=W, A=A, df=df, ev_size=ev_size, ev_div=ev_div, ev_mod=ev_mod,
                lognorm=lognorm)


def _filter_sizes(P):
    """one filter; the largest whole number of filters below a chunk edge and one more (that filter straddles the edge
    unless P divides it), for both chunk sizes; two large chunks and three filters"""
    sizes = [P]
    for edge in (_hip.CHUNK_SMALL, _hip.CHUNK):
        below = (edge - 1) // P
        sizes += [below * P, (below + 1) * P]
    return sizes + [(2 * _hip.CHUNK // P + 3) * P]


def _mvt_rows(rng, df):
    """(numel, table): the whole tensor as one event (700 filters of 3: the lane loop of the event sums takes 11 trips);
    33 events of 130 one-position filters (a second trip of the event loop, per_run = 130); the permuted convolution
    geometry [65, 5, 3, 3] (65 filters per event, per_run = 1 with a stride); 45 events of 3 consecutive 25-position filters"""
    return [(2100, _mvt_table(rng, 3, df, 2100, 2100, 1)), (33 * 130, _mvt_table(rng, 1, df, 130, 130, 33)),
            (65 * 5 * 9, _mvt_table(rng, 9, df, 65 * 9, 9, 5)), (45 * 75, _mvt_table(rng, 25, df, 75, 75, 45))]


def _with_companions(rows, gradless):
    """the whitened rows [(numel, table)] with a PRIOR_NONE segment, an element-wise GENNORM segment (the ordinary branch of
    the same launch) and, last, the whitened segment ``gradless`` whose gradient stays None
    -> (rows [(numel, kind, table)], specs, filters)"""
    rows = [(n, t["kind"], t) for n, t in list(rows) + [gradless]]
    rows.insert(I_W_NONE, (11, R.NONE, None))
    rows.insert(I_W_GENNORM, (7, R.GENNORM, None))
    specs = [None if k == R.NONE else GENNORM_ROW if k == R.GENNORM else (k, 0.0, 1.0, 0.0) for _, k, _ in rows]
    return rows, specs, [t for _, _, t in rows]


def _whitened_inputs(rng, rows, dtype):
    "theta = z A + mu with every |z| >= 0.1 (clear of the bases' kink at z == 0; z == 0: test_filters_at_their_location)"
    thetas = []
    for n, kind, t in rows:
        if t is None:
            thetas.append(_theta(rng, n, GENNORM_ROW[1], kind, dtype, wide=False))
            continue
        z = rng.standard_normal((n // t["P"], t["P"]))
        z = np.sign(z) * (0.1 + np.abs(z))
        thetas.append((z @ t["A"] + t["mu"]).reshape(-1).astype(_np_dtype(dtype)))
    return thetas, [_g(rng, n, dtype) for n, _, _ in rows]


def _run_whitened(arena, rows, specs, filters, inputs):
    "-> theta, g, per-segment log-priors, their total, the partials and the event sums after one sgmcmc_prior_grad"
    arena.load(*inputs)
    arena.table(specs, filters=filters)
    flags = arena.engine.prior_flags()
    assert flags & _hip.PRIOR_FULL and bool(flags & _hip.PRIOR_EVENTS) == any(k == R.MULTIVARIATE_T for _, k, _ in rows)
    arena.engine.prior_grad(N_WHITENED, True)
    th, g = arena.read()
    sums = arena.engine._event_sums
    return (th, g) + arena.log_priors() + (None if sums is None else sums.cpu().numpy(),)


def _hold_whitened(arena, rows, inputs, run, dtype, worst, what, label):
    "every assertion on one launch; ``label(table)`` names the Worst key of a whitened segment"
    u = R.unit_roundoff(dtype)
    th, g, per_seg, total, partials, ev_sum = run
    thetas, gs = inputs
    last = len(rows) - 1
    _check_untouched(arena, th, g, [k for _, k, _ in rows], what)
    assert per_seg[I_W_NONE] == 0.0
    assert all(partials[c, 6] == 0.0 for c in arena.chunks_of(last)), what
    want_total, ev_base = [per_seg[last]], 0
    for i, (n, kind, t) in enumerate(rows[:last]):
        case = f"{what} segment {i} ({n} elements)"
        if kind == R.NONE:
            continue
        if kind == R.GENNORM:
            ref = R.elementwise(kind, *GENNORM_ROW[1:], N_WHITENED, thetas[i], gs[i], u)
            R.check_gradient(arena.seg(g, i), ref, u, f"element-wise gennorm, {case}")
            R.check_logp(float(per_seg[i]), ref["logp"], R.logp_bound(ref), f"log-prior of the element-wise gennorm, {case}")
            want_total.append(ref["logp"])
            continue
        lp, grad, M = R.whitened(t, thetas[i].astype(np.float64))
        want = gs[i].astype(np.float64) - grad / N_WHITENED
        bound = (2 * u if dtype == "float32" else 0.0) * np.abs(want) + (1e-10 * np.abs(want) + 1e-12)
        ratio = np.abs(arena.seg(g, i).astype(np.float64) - want) / bound
        idx = int(np.argmax(ratio))
        worst.add(label(t), float(ratio[idx]), f"{case} element {idx}")
        assert ratio[idx] <= 1.0, f"{case} element {idx}: {ratio[idx]:.3f} x bound; {int((ratio > 1).sum())} of {n} outside"
        lp_bound = 1e-11 * abs(lp) + 1e-9
        worst.add("log-prior " + label(t), R.check_logp(float(per_seg[i]), lp, lp_bound, f"log-prior, {case}"), case)
        want_total.append(lp)
        if M is not None:
            np.testing.assert_allclose(ev_sum[ev_base:ev_base + M.size], M, rtol=1e-11, atol=0, err_msg=f"event sums, {case}")
            ev_base += M.size
    want = math.fsum(want_total)
    worst.add("log-prior total", R.check_logp(total, want, 1e-11 * abs(want) + 1e-9, f"total log-prior, {what}"), what)


def _filter_cases(P, seed):
    "one table per base: the six sizes of ``_filter_sizes`` and the companions"
    rng = np.random.default_rng(seed)
    for base in FILTER_BASES:
        rows = [(n, _filter_table(rng, P, base)) for n in _filter_sizes(P)]
        yield base[0], rng, _with_companions(rows, (3 * P, _filter_table(rng, P, base)))


def _mvt_cases(seed):
    rng = np.random.default_rng(seed)
    for df in MVT_DF:
        yield f"df {df:g}", rng, _with_companions(_mvt_rows(rng, df), (8 * 6, _mvt_table(rng, 3, df, 6, 6, 8)))


def _filter_label(t):
    return "filter " + next(b[0] for b in FILTER_BASES if b[1:] == (t["base"], t["beta"], t["base_scale"]))


@GPU
@pytest.mark.parametrize("P", FILTER_P)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_whitened_filters_match_the_reference(dtype, chunk, P):
    """FILTER_WHITENED from raw tables: P = 1, 3, 9 and SGMCMC_FILTER_MAX_P positions, segments that end just below and
    just beyond the first boundary of either chunk size, every base, next to a PRIOR_NONE, an element-wise GENNORM and a
    grad-less whitened segment in NaN-padded buffers"""
    worst = Worst(f"whitened filters {dtype} chunk {chunk} P {P}")
    arena = None
    for name, rng, (rows, specs, filters) in _filter_cases(P, 500 + P):
        arena = arena or Arena([n for n, _, _ in rows], dtype, chunk, gradless=[len(rows) - 1])
        assert sum(arena.sizes) < 25000
        inputs = _whitened_inputs(rng, rows, dtype)
        run = _run_whitened(arena, rows, specs, filters, inputs)
        assert run[-1] is None
        _hold_whitened(arena, rows, inputs, run, dtype, worst, f"P {P} base {name}", _filter_label)
    worst.report()


@GPU
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_multivariate_t_matches_the_reference(dtype, chunk):
    """MULTIVARIATE_T from raw tables: the four event geometries of ``_mvt_rows`` at df just above 2, 3 and 1e4 -- the
    per-event sums, the gradient and the log-priors"""
    worst = Worst(f"multivariate-t {dtype} chunk {chunk}")
    arena = None
    for name, rng, (rows, specs, filters) in _mvt_cases(600):
        arena = arena or Arena([n for n, _, _ in rows], dtype, chunk, gradless=[len(rows) - 1])
        assert sum(arena.sizes) < 25000
        inputs = _whitened_inputs(rng, rows, dtype)
        run = _run_whitened(arena, rows, specs, filters, inputs)
        _hold_whitened(arena, rows, inputs, run, dtype, worst, name, lambda t: f"mvt df {t['df']:g}")
    worst.report()


@GPU
@pytest.mark.parametrize("dtype", DTYPES)
def test_whitened_bits_do_not_depend_on_the_chunk_size(dtype):
    """an element's value depends on its index in the segment only, and an event's sum on the segment alone: g of every
    whitened segment and ev_sum have the same bits at CHUNK and CHUNK_SMALL, and ev_sum again on a second call"""
    cases = [c for P in FILTER_P for c in _filter_cases(P, 500 + P)] + list(_mvt_cases(600))
    for name, rng, (rows, specs, filters) in cases:
        inputs = _whitened_inputs(rng, rows, dtype)
        runs = []
        for chunk in CHUNKS:
            arena = Arena([n for n, _, _ in rows], dtype, chunk, gradless=[len(rows) - 1])
            runs.append(_run_whitened(arena, rows, specs, filters, inputs))
            if runs[-1][-1] is not None:
                again = _run_whitened(arena, rows, specs, filters, inputs)
                assert_same_bits(again[-1], runs[-1][-1], f"{name}: ev_sum of a second call, chunk {chunk}")
        for i, (n, kind, t) in enumerate(rows):
            if t is not None:
                assert_same_bits(arena.seg(runs[0][1], i), arena.seg(runs[1][1], i), f"{name}: g of segment {i} (P {t['P']})")
        if runs[0][-1] is not None:
            assert_same_bits(runs[0][-1], runs[1][-1], f"{name}: ev_sum at the two chunk sizes")


@GPU
def test_prior_grad_refuses_a_filter_table_it_cannot_evaluate():
    """a layout with a filter table but without SGMCMC_PRIOR_FULL in its prior_flags, and SGMCMC_PRIOR_EVENTS without a
    filter table: hipErrorInvalidValue, nothing launched"""
    rng = np.random.default_rng(2)
    rows, specs, filters = _with_companions([(n, _filter_table(rng, 3, FILTER_BASES[0])) for n in (3, 1026)],
                                            (9, _filter_table(rng, 3, FILTER_BASES[0])))
    for case in ("filters without PRIOR_FULL", "PRIOR_EVENTS without filters"):
        arena = Arena([n for n, _, _ in rows], "float32", _hip.CHUNK_SMALL, gradless=[len(rows) - 1])
        arena.load(*_whitened_inputs(rng, rows, "float32"))
        eng = arena.engine
        if case.startswith("filters"):
            arena.table(specs, filters=filters)
            assert eng.layout.filters and eng.layout.prior_flags & _hip.PRIOR_FULL
            eng.layout.prior_flags = 0
            flags = _hip.PRIOR_FULL               # (the caller's flags do not stand in for the layout's)
        else:
            arena.table([None if s is None else GENNORM_ROW for s in specs])
            assert not eng.layout.filters
            flags = _hip.PRIOR_FULL | _hip.PRIOR_EVENTS
        rc = eng.lib.sgmcmc_prior_grad(ctypes.byref(eng.layout), N_WHITENED, 1, flags, eng.stream())
        assert rc == INVALID_VALUE, case
        th, g = arena.read()
        assert_same_bits(th, arena.theta0, f"{case}: theta")
        assert_same_bits(g, arena.g0, f"{case}: g")
