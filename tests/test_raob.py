"""The Rao-Blackwellised regression model (bnn_priors_amd/raob.py, csrc/raob_hip.inc, models.RaoBRegressionModel) against
tests/raob_reference.py and the reference's own numbers (tests/golden/raob.npz, written by golden/make_raob_goldens.py).

THE TOLERANCE RULE of the value tests.  Per case the float64 restatement (numpy, the same formulas) is a distance ``dist``
from the longdouble value -- for the log likelihood the longdouble DIRECT N x N Gaussian where N <= 65, the longdouble
closed form beyond (O(N^3) is out of reach at N = 16451; the two agree below 1e-9 relative at every small case, see
``test_closed_form_is_the_direct_gaussian``).  A kernel result may differ from the longdouble value by at most
4 dist + 4 ulp of the result: the kernels add in another, tiled order than numpy does, which is worth a small factor and
no more.  For arrays both distances are max-norms and the ulp is that of the largest entry (raob_reference.bound).

Measured ``dist`` per case (N, F, v), s2 = 2 / F, inputs of raob_reference.case_inputs (feature 1 dead where F >= 3):

      N   F       v   log p     d/df      d/dv      w_mean    w_root    mean      var
      1   1    0.64   3.8e-17   0         3.1e-17   0         5.4e-20   0         2.7e-15
      1   1    1e-4   4.8e-15   0         9.8e-12   0         0         0         1.6e-15
      5   3    0.64   1.6e-15   6.5e-16   3.3e-15   2.1e-16   7.2e-17   2.1e-16   6.4e-17
      5   3    1e-4   1.5e-11   1.7e-12   1.1e-07   3.1e-17   7.8e-19   5.8e-17   2.0e-18
      1  17    0.64   2.0e-16   8.3e-17   1.4e-15   1.0e-16   3.1e-16   6.7e-17   2.3e-16
      1  17    1e-4   8.4e-13   4.1e-13   4.9e-09   7.3e-13   5.1e-13   5.1e-13   2.1e-13
     64  16    0.64   1.6e-14   2.4e-15   9.0e-15   9.5e-16   1.1e-16   4.7e-16   4.6e-17
     64  16    1e-4   9.9e-10   1.9e-11   5.7e-07   9.7e-16   2.2e-18   8.3e-16   4.3e-17
     65  17    0.64   6.3e-14   3.6e-15   7.0e-14   1.0e-15   1.2e-16   9.0e-16   1.3e-16
     65  17    1e-4   2.9e-10   2.9e-11   3.0e-06   2.2e-15   2.7e-18   1.7e-15   9.8e-17
     10  40    0.64   3.8e-15   8.1e-16   7.3e-15   7.0e-16   3.6e-16   6.2e-16   1.8e-16
     10  40    1e-4   3.9e-10   5.9e-11   3.9e-06   1.3e-11   4.5e-13   6.7e-12   1.2e-13
     65  50    0.64   2.6e-15   2.8e-15   1.0e-13   1.9e-15   4.8e-16   1.2e-15   3.4e-16
     65  50    1e-4   8.1e-10   2.8e-10   7.1e-06   4.1e-14   2.0e-16   1.1e-14   4.8e-18
     64  64    0.64   1.4e-14   1.6e-15   5.1e-14   1.7e-15   3.1e-16   1.2e-15   2.0e-16
     64  64    1e-4   3.1e-09   2.9e-09   3.2e-05   3.4e-12   1.6e-14   1.4e-12   1.4e-15
  16451  50    0.64   4.6e-12   7.5e-15   9.4e-12   2.9e-15   2.6e-17   1.2e-15   4.8e-17
  16451  50    1e-4   1.6e-08   5.0e-11   8.9e-05   3.0e-15   3.2e-19   1.3e-15   6.1e-18

(v = 1e-4 makes the terms of log p and of d/dv some 1e4 .. 1e8 times the v = 0.64 ones, and A's condition number 1e4 times
larger; (10, 40) is N < F: a Gram matrix of rank 10.)  The tests print their own figures before they assert.
"""
import functools
import os

import numpy as np
import pytest
import torch

import raob_reference as R
from helpers import default_dtype

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raob.npz")
TILE = 64                                    # SGMCMC_RAOB_TILE_ROWS
TWO_TILES = 256 * TILE + TILE + 3            # workgroups 0 and 1 take two tiles, the last tile has 3 rows
ROWS = (1, 5, TILE, TILE + 1, TWO_TILES)
FEATURES = (1, 3, 16, 17, 50, 64)
CASES = ((1, 1), (5, 3), (1, 17), (64, 16), (65, 17), (10, 40), (65, 50), (64, 64), (TWO_TILES, 50))
NOISE = (0.64, 1e-4)
FIELDS = ("ll", "df", "dv", "w_mean", "w_root")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def reference(N, F, v):
    "inputs, the float64 restatement, the longdouble values and the exact log likelihood of one case; computed once"
    f, y = R.case_inputs(N, F, dead_column=1 if F >= 3 else None)
    f_star = R.case_inputs(7, F, seed=1)[0]
    s2 = 2.0 / F
    m64, mld = R.marginal(f, y, v, s2), R.marginal(f, y, v, s2, np.longdouble)
    exact_ll = R.direct_gaussian(f, y, v, s2) if N <= 65 else mld.ll
    p64, pld = R.predictive(m64, f_star, v, s2), R.predictive(mld, f_star, v, s2, np.longdouble)
    for a in (f, y, f_star):
        a.setflags(write=False)
    return f, y, f_star, s2, m64, mld, exact_ll, p64, pld


def dense_features(g, tag, x, dtype=np.float64):
    "net(x) of the golden's RaoBDenseNet (two ReLU layers) or RaoBLinearRegression (the identity) in numpy"
    h = np.asarray(x, dtype=dtype)
    for i in (0, 2):
        key = f"{tag}.state.net.{i}.weight_prior.p"
        if key not in g:
            return h
        h = np.maximum(h @ g[key].astype(dtype).T + g[f"{tag}.state.net.{i}.bias_prior.p"].astype(dtype), 0)
    return h


GOLDEN_CASES = {"dense": (0.8 ** 2, 2.0 / 40), "linear": (0.5 ** 2, 2.0 / 3)}        # noise_std^2, last_layer_std^2


# ---- host ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_restatement_reproduces_the_reference(case):
    """the numpy formulas against what the reference's code computed in float64: two float64 evaluations of the same
    quantities by different routes (the reference whitens by v before it factors), so they agree to the conditioning of
    A (below 1e3 here: 10 rows of features of size 1, v >= 0.25) times a few hundred roundings: 1e-11 relative."""
    g, tag = golden(), f"{case}.float64"
    v, s2 = GOLDEN_CASES[case]
    x, y = g[f"{tag}.state.x_train"], g[f"{tag}.state.y_train"]
    m = R.marginal(dense_features(g, tag, x), y, v, s2)
    mean, var = R.predictive(m, dense_features(g, tag, g[f"{tag}.x_test"]), v, s2)
    for name, ours, ref in (("ll", m.ll, g[f"{tag}.ll"]), ("w_mean", m.w_mean, g[f"{tag}.w_mean"][:, 0]),
                            ("w_root", m.w_root, g[f"{tag}.w_root"]), ("mean", mean, g[f"{tag}.pred_mean"][:, 0]),
                            ("scale", np.sqrt(var), g[f"{tag}.pred_scale"][:, 0])):
        err = np.max(np.abs(ours - ref)) / np.max(np.abs(ref))
        print(case, name, err)
        assert err < 1e-11, (name, err)
    assert float(R.direct_gaussian(dense_features(g, tag, x), y, v, s2) - g[f"{tag}.ll"]) == pytest.approx(0, abs=1e-11)


@pytest.mark.parametrize("N,F", [c for c in CASES if c[0] <= 65])
@pytest.mark.parametrize("v", NOISE)
def test_closed_form_is_the_direct_gaussian(N, F, v):
    "Woodbury's form and the N x N Gaussian, both in longdouble (eps 1.1e-19, A's condition number up to 1e7)"
    *_, mld, exact_ll, _, _ = reference(N, F, v)
    assert abs(float(mld.ll - exact_ll)) <= 1e-9 * abs(float(exact_ll))
    # ... and the closed-form gradient in v is the derivative of that Gaussian (central difference in longdouble)
    f, y, _, s2 = reference(N, F, v)[:4]
    h = np.longdouble(v) * np.longdouble(1e-6)
    fd = (R.direct_gaussian(f, y, np.longdouble(v) + h, s2) - R.direct_gaussian(f, y, np.longdouble(v) - h, s2)) / (2 * h)
    assert abs(float(fd - mld.dv)) <= 1e-6 * abs(float(mld.dv)) + 1e-9


def test_argument_refusals():
    from bnn_priors_amd import models, raob
    f, y = torch.zeros(4, 3), torch.zeros(4, 1)
    bad = [
        (dict(f=f.long()), "float32 or float64"), (dict(f=f[0]), r"\[N, F\]"), (dict(f=torch.zeros(4, 65)), "65 features"),
        (dict(f=torch.zeros(0, 3), y=torch.zeros(0, 1)), "0 rows"), (dict(y=torch.zeros(4)), r"\[N, 1\]"),
        (dict(y=torch.zeros(4, 2)), r"\[N, 1\]"), (dict(y=y.double()), "must agree"), (dict(noise_var=0.0), "noise_var"),
        (dict(noise_var=float("nan")), "noise_var"), (dict(last_layer_var=-1.0), "last_layer_var"),
        (dict(noise_var=torch.zeros(2)), "0-dim"), (dict(), "CUDA tensor"),
    ]
    for change, message in bad:
        args = dict(f=f, y=y, noise_var=0.5, last_layer_var=1.0)
        args.update(change)
        with pytest.raises(ValueError, match=message):
            raob.marginal_log_likelihood(**args)
        if "noise_var" not in change and "last_layer_var" not in change:
            with pytest.raises(ValueError, match=message):
                raob.gram(args["f"], args["y"])
        with pytest.raises(ValueError, match=message):
            raob.posterior(**args)
    with pytest.raises(ValueError, match="RaoBPosterior"):
        raob.predictive(None, f)
    # there is no CPU path behind the model either: a missing kernel route is an error, not eager torch
    model = models.RaoBLinearRegression(torch.randn(4, 3), torch.randn(4, 1))
    with pytest.raises(ValueError, match="CUDA tensor"):
        model.log_likelihood(None, None, 4)
    with pytest.raises(AssertionError):
        model.log_likelihood(torch.randn(4, 3), None, 4)
    with pytest.raises(ValueError, match="outside the accelerated path"):
        models.get_model(torch.randn(4, 3), torch.randn(4, 1), "no_such_model")


def test_bindings_and_limits():
    from bnn_priors_amd import _hip, raob
    assert raob.MAX_FEATURES == _hip.RAOB_MAX_F == 64 and _hip.RAOB_TILE_ROWS == TILE
    lib = _hip.lib()
    part = lambda F: (F + 1) * (F + 2) // 2                                          # noqa: E731
    assert lib.sgmcmc_raob_workspace_doubles(1, 1) == part(1)
    assert lib.sgmcmc_raob_workspace_doubles(TILE + 1, 50) == 2 * part(50)
    assert lib.sgmcmc_raob_workspace_doubles(2 ** 31 - 1, 64) == _hip.RAOB_MAX_BLOCKS * part(64)
    for N, F in ((0, 3), (2 ** 31, 3), (5, 0), (5, 65)):
        assert lib.sgmcmc_raob_workspace_doubles(N, F) == -1


# ---- device -------------------------------------------------------------------------------------------------------------

def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("F", FEATURES)
def test_gram_is_exact_on_integers(F, dtype):
    "integer-valued f and y with |.| <= 8: every product and sum is exact in fp64, so G, c, yy equal int64 arithmetic"
    from bnn_priors_amd import raob
    gen = torch.Generator().manual_seed(F)
    for N in ROWS:
        f = torch.randint(-8, 9, (N, F), generator=gen)
        y = torch.randint(-8, 9, (N, 1), generator=gen)
        G, c, yy = raob.gram(f.to(dtype).to(DEV), y.to(dtype).to(DEV))
        assert G.dtype == torch.float64 and G.shape == (F, F) and c.shape == (F,) and yy.dim() == 0
        assert torch.equal(G.cpu(), (f.t() @ f).double()), (N, F)
        assert torch.equal(c.cpu(), (f.t() @ y)[:, 0].double()), (N, F)
        assert yy.item() == float((y * y).sum()), (N, F)


def _kernel_results(f, y, f_star, v, s2, dtype=torch.float64):
    from bnn_priors_amd import raob
    fd, yd = _dev(f, dtype).requires_grad_(), _dev(y, dtype)
    vd = torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True)
    ll = raob.marginal_log_likelihood(fd, yd, vd, s2)
    df, dv = torch.autograd.grad(ll, [fd, vd])
    post = raob.posterior(fd.detach(), yd, v, s2)
    mean, var = raob.predictive(post, _dev(f_star, dtype))
    out = dict(ll=ll.detach(), df=df, dv=dv, w_mean=post.b * s2 ** 0.5, w_root=post.Linv * post.noise_var.sqrt(),
               mean=mean, var=var)
    return {k: t.cpu().numpy() for k, t in out.items()}, post


@pytest.mark.gpu
@pytest.mark.parametrize("v", NOISE)
@pytest.mark.parametrize("N,F", CASES)
def test_values_and_gradients(N, F, v):
    "likelihood, both gradients, posterior_w and the predictive under THE TOLERANCE RULE (module docstring)"
    f, y, f_star, s2, m64, mld, exact_ll, p64, pld = reference(N, F, v)
    got, post = _kernel_results(f, y, f_star, v, s2)
    pairs = {"ll": (m64.ll, exact_ll), "df": (m64.df, mld.df), "dv": (m64.dv, mld.dv), "w_mean": (m64.w_mean, mld.w_mean),
             "w_root": (m64.w_root, mld.w_root), "mean": (p64[0], pld[0]), "var": (p64[1], pld[1])}
    failures = []
    for name, (restated, exact) in pairs.items():
        allowed, dist = R.bound(restated, exact)
        err = R.distance(got[name], exact)
        print(f"N={N} F={F} v={v} {name}: restatement {dist:.3e} kernel {err:.3e} allowed {allowed:.3e}")
        if not err <= allowed:
            failures.append((name, err, allowed))
    assert not failures, failures
    assert (got["var"] >= v).all()                                      # the variance never goes below the noise
    assert torch.equal(post.Ainv, post.Ainv.t()) and torch.equal(post.G, post.G.t())
    assert torch.equal(post.Linv, post.Linv.tril()) and torch.equal(post.L, post.L.tril())


@pytest.mark.gpu
def test_float32_inputs_are_widened_not_rounded():
    "fp32 f and y give the fp64 results of the widened values; only the stored gradient and the returned value are fp32"
    f, y, f_star, s2 = reference(65, 50, 0.64)[:4]
    f32, y32, fs32 = (np.float32(a) for a in (f, y, f_star))
    wide, _ = _kernel_results(f32.astype(np.float64), y32.astype(np.float64), fs32.astype(np.float64), 0.64, s2)
    got, _ = _kernel_results(f32, y32, fs32, 0.64, s2, torch.float32)
    for name in ("w_mean", "w_root", "mean", "var", "dv"):
        assert np.array_equal(got[name], wide[name]), name
    assert got["ll"].dtype == np.float32 and got["ll"] == np.float32(wide["ll"])
    assert got["df"].dtype == np.float32 and np.array_equal(got["df"], wide["df"].astype(np.float32))


@pytest.mark.gpu
def test_gradcheck():
    from bnn_priors_amd import raob
    f, y = R.case_inputs(7, 5, seed=3)
    fd, yd = _dev(f + 0.1).requires_grad_(), _dev(y)            # (off the ReLU's kink: the function of f itself is smooth)
    vd = torch.tensor(0.64, dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: raob.marginal_log_likelihood(a, yd, b, 0.4), (fd, vd))
    assert torch.autograd.gradcheck(lambda a: 3.0 * raob.marginal_log_likelihood(a, yd, 0.64, 0.4), (fd,))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_two_calls_give_identical_bits(dtype):
    f, y, f_star, s2 = reference(TWO_TILES, 50, 0.64)[:4]
    a, pa = _kernel_results(f, y, f_star, 0.64, s2, dtype)
    b, pb = _kernel_results(f, y, f_star, 0.64, s2, dtype)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert torch.equal(pa.state, pb.state)


@pytest.mark.gpu
def test_an_overflowed_gram_matrix_gives_nan_everywhere_and_nothing_else_happens():
    "f at 1e200: A overflows, the first pivot is not finite; every output is NaN, and the next call is unharmed"
    f, y, f_star, s2 = reference(65, 17, 0.64)[:4]
    got, post = _kernel_results(f * 1e200 + 1e200, y, f_star, 0.64, s2)
    for name, value in got.items():
        assert np.isnan(value).all(), name
    for field in ("log_likelihood", "dnoise_var", "b", "Linv", "Ainv", "L"):
        assert torch.isnan(getattr(post, field)).all(), field
    again, _ = _kernel_results(f, y, f_star, 0.64, s2)
    assert np.isfinite(again["ll"]) and np.isfinite(again["df"]).all()


def _golden_model(case, dtype):
    from bnn_priors_amd import models
    g, tag = golden(), f"{case}.{str(dtype).split('.')[1]}"
    state = {k[len(tag) + 7:]: torch.from_numpy(a) for k, a in g.items() if k.startswith(tag + ".state.")}
    with default_dtype(dtype):
        if case == "dense":
            model = models.RaoBDenseNet(state["x_train"], state["y_train"], 40, noise_std=0.8)
        else:
            model = models.RaoBLinearRegression(state["x_train"], state["y_train"], noise_std=0.5)
        assert sorted(model.state_dict()) == sorted(state)
        model.load_state_dict(state)
    return model.to(DEV), g, tag


def _model_outputs(model, x_test):
    ll = model.log_likelihood(model.x_train, model.y_train, 10)
    params = dict(model.named_parameters())
    grads = torch.autograd.grad(ll, list(params.values())) if params else ()
    with torch.no_grad():
        mean, root = model.posterior_w()
        pred = model(x_test)
        white, L_w = model._posterior_w(model.x_train, model.y_train)
    out = {"ll": ll.detach(), "w_mean": mean, "w_root": root, "pred_mean": pred.mean, "pred_scale": pred.scale}
    out.update({f"grad.{k}": g for k, g in zip(params, grads)})
    # the unaccelerated autograd route (a gradient is required: the parameters') must say the same
    mean_a, root_a = model.posterior_w()
    pred_a = model(x_test)
    white_a, L_wa = model._posterior_w(model.x_train, model.y_train)
    for a, b in ((mean_a, mean), (root_a, root), (pred_a.mean, pred.mean), (pred_a.scale, pred.scale), (white_a, white),
                 (L_wa, L_w)):
        if params:
            assert a.requires_grad
        assert torch.allclose(a.detach().double(), b.double(), rtol=1e-5 if ll.dtype == torch.float32 else 1e-9,
                              atol=1e-6 if ll.dtype == torch.float32 else 1e-11)
    return {k: t.detach().cpu().numpy() for k, t in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_golden_model_float64(case):
    """the model on the device against the longdouble values of the golden's weights under THE TOLERANCE RULE, where
    ``dist`` is the distance of the REFERENCE's float64 numbers (the golden) from them; the parameter gradients -- the
    same linear backward map applied to d/df in both -- against the golden's at 4 times the relative distance of the
    golden's log likelihood, posterior mean and root from longdouble, plus 64 eps for 40-term dot products in another
    order"""
    model, g, tag = _golden_model(case, torch.float64)
    v, s2 = GOLDEN_CASES[case]
    x, y, x_test = g[f"{tag}.state.x_train"], g[f"{tag}.state.y_train"], g[f"{tag}.x_test"]
    ld = np.longdouble
    mld = R.marginal(dense_features(g, tag, x, ld), y, v, s2, ld)
    mean, var = R.predictive(mld, dense_features(g, tag, x_test, ld), v, s2, ld)
    exact = {"ll": R.direct_gaussian(dense_features(g, tag, x, ld), y, v, s2), "w_mean": mld.w_mean[:, None],
             "w_root": mld.w_root, "pred_mean": mean[:, None], "pred_scale": np.sqrt(var)[:, None]}
    got = _model_outputs(model, _dev(x_test))
    failures, rel = [], 0.0
    for name, value in exact.items():
        allowed, dist = R.bound(g[f"{tag}.{name}"], value)
        err = R.distance(got[name], value)
        rel = max(rel, dist / float(np.max(np.abs(value))))
        print(f"{case} {name}: golden {dist:.3e} model {err:.3e} allowed {allowed:.3e}")
        if not err <= allowed:
            failures.append((name, err, allowed))
    for name in (k for k in got if k.startswith("grad.")):
        ref = g[f"{tag}.{name}"]
        err = np.max(np.abs(got[name] - ref)) / np.max(np.abs(ref))
        allowed = 4 * rel + 64 * 2.0 ** -52
        print(f"{case} {name}: relative {err:.3e} allowed {allowed:.3e}")
        if not err <= allowed:
            failures.append((name, err, allowed))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_golden_model_float32(case):
    """fp32 against the reference's fp32 numbers, per quantity at 4 times the relative (max-norm) distance between the
    golden's own fp32 and fp64 numbers: what fp32 features, a fp32 Gram matrix and fp32 storage cost the reference"""
    model, g, tag = _golden_model(case, torch.float32)
    tag64 = tag.replace("float32", "float64")
    got = _model_outputs(model, _dev(g[f"{tag}.x_test"], torch.float32))
    failures = []
    for name, value in got.items():
        ref32, ref64 = g[f"{tag}.{name}"], g[f"{tag64}.{name}"]
        assert value.dtype == ref32.dtype and value.shape == ref32.shape, name
        scale = np.max(np.abs(ref64))
        allowed = 4 * np.max(np.abs(ref32 - ref64)) / scale
        err = np.max(np.abs(value.astype(np.float64) - ref32)) / scale
        print(f"{case} {name}: relative {err:.3e} allowed {allowed:.3e}")
        if not err <= allowed:
            failures.append((name, err, allowed))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["raobdensenet", "raob_linear"])
def test_get_model_builds_the_reference_names(name):
    from bnn_priors_amd import models
    x, y = torch.randn(12, 3, device=DEV), torch.randn(12, 1, device=DEV)
    model = models.get_model(x, y, name, width=50)
    assert isinstance(model, models.RaoBRegressionModel)
    assert sorted(model.state_dict()) == list(golden()[f"keys.{name}"])
    assert all(t.device.type == "cuda" for t in model.state_dict().values())
    value = model.potential(x, y, 12.)                      # the tensors it was built with: no comparison on the device
    assert torch.isfinite(value)
    params = list(model.parameters())
    assert len(params) == (5 if name == "raobdensenet" else 0)          # raob_linear has nothing left to sample
    if params:
        value.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)


def _snapshot(opt):
    return ([p.detach().clone() for p in opt.state], [st['momentum_buffer'].detach().clone() for st in opt.state.values()])


def _close(xs, ys):
    return [torch.allclose(a, b) for a, b in zip(xs, ys)]


@pytest.mark.gpu
def test_hmc_reversible():
    """test_hip_reference_tests.test_hmc_reversible on RaoBDenseNet in float64: the closure is over the marginal
    likelihood (``potential``), num_data = 1; forward three leapfrog steps, negate the momenta, back.  lr is small enough
    that the energy H = U + m.m / 2, with U from the numpy restatement, changes by less than 0.1 over the three steps."""
    from bnn_priors_amd import mcmc, models
    with default_dtype(torch.float64):
        torch.manual_seed(3)
        x = torch.randn(10, 3, device=DEV)
        y = x[:, :1].sin() + 0.1 * torch.randn(10, 1, device=DEV)
        model = models.RaoBDenseNet(x, y, 10, noise_std=0.5).to(DEV)

        def loss():
            model.zero_grad()
            v = model.potential(None, None, 1.)
            v.backward()
            return v

        def energy(momenta):
            with torch.no_grad():
                f, log_prior = model.net(model.x_train).cpu().numpy(), float(model.log_prior())
            U = -(float(R.marginal(f, y.cpu().numpy(), 0.25, model.last_layer_std ** 2).ll) + log_prior)
            return U + 0.5 * sum(float((m.double() ** 2).sum()) for m in momenta)

        hmc = mcmc.HMC(model.parameters(), lr=1e-3, num_data=1, raise_on_nan=True, raise_on_no_grad=True)
        for _, st in hmc.state.items():
            st['preconditioner'] = torch.rand(()).item() + 0.2
        hmc.sample_momentum()
        p0, m0 = _snapshot(hmc)
        e0 = energy(m0)
        hmc.initial_step(loss)
        p1, m_half = _snapshot(hmc)
        hmc.step(loss)
        p2, m_3half = _snapshot(hmc)
        hmc.final_step(loss)
        p2_alt, m2 = _snapshot(hmc)
        delta = energy(m2) - e0
        print("energy change over the three steps:", delta)
        assert abs(delta) < 0.1
        assert not any(_close(p0, p1)) and not any(_close(p1, p2)) and all(_close(p2, p2_alt))
        assert not any(_close(m0, m_half)) and not any(_close(m_half, m_3half)) and not any(_close(m_3half, m2))
        for _, st in hmc.state.items():
            st['momentum_buffer'].neg_()
        hmc.initial_step(loss)
        p1_alt, m_3half_neg = _snapshot(hmc)
        assert all(_close(p1, p1_alt)) and all(_close(m_3half, [-m for m in m_3half_neg]))
        hmc.step(loss)
        p0_alt, m_half_neg = _snapshot(hmc)
        assert all(_close(p0, p0_alt)) and all(_close(m_half, [-m for m in m_half_neg]))
        hmc.final_step(loss)
        p0_alt2, m0_neg = _snapshot(hmc)
        assert all(_close(p0, p0_alt2)) and all(_close(m0, [-m for m in m0_neg]))
