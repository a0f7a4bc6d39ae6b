"""Effective dimensionality (bnn_priors_amd/eff_dim.py, csrc/lanczos_hip.inc): the autograd helpers, the Lanczos step, the
tridiagonal eigensolver, the Ritz vectors, the "positive" rule and N_eff.  The five properties that the reference's
``testing/test_eff_dim.py`` asks of the module its tree lacks (dense Hessian, Hessian-vector product in ``p.grad``,
``unflatten_like``, eigenvalues by Lanczos of a matrix and of a Hessian) are tested here afresh.

Tolerances are measured, not guessed: ``eff_dim_reference`` evaluates the GPU tests' own inputs in float64 and in longdouble,
the largest deviation per quantity is recorded below with its scale, and the GPU tolerance is 4 x that against the
longdouble values (the factor allows for the kernels' other summation order and the matrix pipe's internal order).
``test_the_recorded_deviations_are_the_measured_ones`` re-measures them.  For the invariants (orthogonality, residuals) the
recorded figure is what the float64 restatement itself leaves, evaluated in longdouble.  After a breakdown the continuation
depends on rounding, so whole runs are compared by invariants only, and where restarts occur a Ritz value is held to
max(4 x measured, breakdown_rtol): a beta <= rtol * scale was set to zero, which moves an eigenvalue by at most that."""
import functools
import zlib

import numpy as np
import pytest
import torch

import eff_dim_reference as ref

# single step, relative to |w| (c, alpha, beta) and to max |v| (the next row)
C_DEVIATION = 6.0e-17
ALPHA_DEVIATION = 4.2e-17
BETA_DEVIATION = 4.3e-16
V_DEVIATION = 8.4e-16
# tridiagonal eigensolver, relative to max |theta|: theta, max |T Y - Y theta|, max |Y^T Y - I|
THETA_DEVIATION = 9.0e-16
TY_DEVIATION = 5.1e-16
YY_DEVIATION = 3.9e-15
# whole runs with m = D: max |V V^T - I|; Ritz values against eigvalsh and max |A U - U theta|, relative to |A|_2
VV_DEVIATION = 5.3e-16
RITZ_DEVIATION = 2.9e-14
AU_DEVIATION = 1.4e-14
# the residual estimate against the true residual norm |A u - theta u|, relative to |A|_2 (m = 20, 40 at D = 130)
RESIDUAL_DEVIATION = 2.9e-17
NEFF_DEVIATION = 1.6e-16            # N_eff, relative to the number of eigenvalues

CHUNK, ROWS, MAX_M, MAX_SPLITS, WIDTH = 256, 16, 512, 512, 514
LD = np.longdouble
EPS = 2.0 ** -52


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------------------------------------- step inputs

STEP_CASES = {f"rows{r}": (r, CHUNK + 1, None) for r in (1, 2, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 3)}
STEP_CASES.update({f"D{D}": (1, D, None) for D in (1, 2, CHUNK - 1, CHUNK)})
STEP_CASES["D2_rows2"] = (2, 2, None)                                             # nothing is left of w: a breakdown
STEP_CASES["default_workspace"] = (ROWS + 1, (2 * MAX_SPLITS + 1) * CHUNK - 57, None)
STEP_CASES["three_splits"] = (ROWS + 1, 7 * CHUNK - 57, 3 * WIDTH * 8)
BREAKDOWNS = ("D1", "D2_rows2")


@functools.lru_cache(maxsize=None)
def _step_inputs(name):
    rows, D, _ = STEP_CASES[name]
    rng = _rng(name)
    V = np.linalg.qr(rng.standard_normal((D, rows)))[0].T.copy()
    w = rng.standard_normal(D) * 3.0
    return V, w


@functools.lru_cache(maxsize=None)
def _step_ref(name, wide):
    V, w = _step_inputs(name)
    return ref.step(V, w, 0.0, ref.default_rtol(V.shape[1]), wide)


def _step_deviations(got, wide, w):
    n = float(np.sqrt(np.sum(w.astype(LD) ** 2)))
    out = dict(c=max(np.max(np.abs(got[k] - wide[k])) for k in ("c1", "c2")) / n, alpha=abs(got["alpha"] - wide["alpha"]) / n,
               beta=abs(got["norm"] - wide["norm"]) / n, v=0.0)
    if wide["ok"]:
        out["v"] = np.max(np.abs(got["v_next"] - wide["v_next"])) / np.max(np.abs(wide["v_next"]))
    return {k: float(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------- tridiagonal inputs

def _toeplitz(m):
    return np.full(m, 2.0), np.full(m, -1.0)


def _wilkinson(n=21):
    return np.abs(np.arange(n) - (n - 1) / 2.0), np.ones(n)


TRIDIAG_CASES = {f"toeplitz{m}": _toeplitz(m) for m in (1, 2, 3, 63, 64, 65, 130, 512)}
TRIDIAG_CASES["wilkinson21"] = _wilkinson()
TRIDIAG_CASES["graded"] = (10.0 ** -np.arange(16), 10.0 ** -(np.arange(16) + 1.0))
TRIDIAG_CASES["diagonal"] = (np.array([3.0, -1.0, 2.0, 2.0, 0.0, 7.5, -4.0]), np.zeros(7))
TRIDIAG_CASES["identity"] = (np.ones(9), np.zeros(9))


@functools.lru_cache(maxsize=None)
def _tridiag_ref(name, wide):
    "(the longdouble run without its vectors: only its eigenvalues are compared)"
    return ref.tridiag_eig(*TRIDIAG_CASES[name], wide=wide, vectors=not wide)


def _dense_T(a, b):
    m = len(a)
    return np.diag(np.asarray(a, LD)) + np.diag(np.asarray(b, LD)[:m - 1], 1) + np.diag(np.asarray(b, LD)[:m - 1], -1)


def _tridiag_deviations(name, theta, Y):
    "theta against the longdouble restatement; the invariants of (theta, Y) evaluated in longdouble"
    a, b = TRIDIAG_CASES[name]
    wide = _tridiag_ref(name, True)[0]
    top = float(np.max(np.abs(wide)))
    T, theta, Y = _dense_T(a, b), np.asarray(theta, LD), np.asarray(Y, LD)
    return dict(theta=float(np.max(np.abs(theta - wide))) / top, TY=float(np.max(np.abs(T @ Y - Y * theta[None, :]))) / top,
                YY=float(np.max(np.abs(Y.T @ Y - np.eye(len(a))))))


# --------------------------------------------------------------------------------------------------------- whole-run inputs

def _psd(D, rng):
    B = rng.standard_normal((D, D + 3))
    return B @ B.T / D


@functools.lru_cache(maxsize=None)
def _matrix(name):
    "-> (A, v0 or None, the least number of restarts: 0 means none at all, None no statement)"
    rng = _rng(name)
    if name.startswith("psd"):
        return _psd(int(name[3:]), rng), None, 0
    Q = lambda D: np.linalg.qr(rng.standard_normal((D, D)))[0]                # noqa: E731
    if name == "fivefold":                                                        # indefinite, one eigenvalue five times
        q, lam = Q(40), np.concatenate([np.full(5, 1.5), np.linspace(-2.0, 3.0, 35)])
        return (q * lam) @ q.T, None, 4
    if name == "wide_spectrum":
        q = Q(60)
        return (q * np.logspace(-12, 3, 60)) @ q.T, None, None                  # (eigenvalues below rtol |A| count as zero)
    if name == "identity":
        return np.eye(20), None, 19
    if name == "zero":
        return np.zeros((20, 20)), None, 19
    if name == "rank3":
        B = rng.standard_normal((50, 3))
        return B @ B.T, None, 46
    if name == "invariant_start":                                                 # v0 inside a 3-dimensional invariant subspace
        q, lam = Q(30), np.linspace(0.5, 4.0, 30)
        return (q * lam) @ q.T, q[:, [2, 11, 17]] @ np.array([1.0, -2.0, 0.5]), 1
    raise KeyError(name)


MATRICES = tuple(f"psd{D}" for D in (1, 2, 8, 63, 64, 65, 130)) + ("fivefold", "wide_spectrum", "identity", "zero", "rank3",
                                                                   "invariant_start")


def _sym(A):
    return (A + A.T) / 2


def _run_invariants(A, V, theta, U, restarts):
    "of a run with m = D, evaluated in longdouble: orthogonality, Ritz values against eigvalsh, residual of the Ritz pairs"
    A = _sym(np.asarray(A, np.float64))
    norm = max(float(np.max(np.abs(np.linalg.eigvalsh(A)))), np.finfo(float).tiny)
    V, U, theta = np.asarray(V, LD), np.asarray(U, LD), np.asarray(theta, LD)
    return dict(VV=float(np.max(np.abs(V @ V.T - np.eye(V.shape[0])))),
                ritz=float(np.max(np.abs(theta - np.linalg.eigvalsh(A)))) / norm,
                AU=float(np.max(np.abs(A.astype(LD) @ U - U * theta[None, :]))) / norm)


@functools.lru_cache(maxsize=None)
def _run_ref(name):
    A, v0, _ = _matrix(name)
    A = _sym(A)
    run = ref.lanczos(A, A.shape[0], v0=v0, seed=1)
    theta, Y, _, failed = ref.tridiag_eig(run["alpha"], run["beta"])
    assert not failed
    U = ref.ritz(run["V"], Y, np.arange(run["m"]))
    return dict(run, theta=theta, Y=Y, U=U, **_run_invariants(A, run["V"], theta, U, run["restarts"]))


@functools.lru_cache(maxsize=None)
def _residual_ref(m):
    A = _sym(_matrix("psd130")[0])
    run = ref.lanczos(A, m, seed=2)
    theta, Y, _, _ = ref.tridiag_eig(run["alpha"], run["beta"])
    return _residual_deviation(A, run["V"], theta, Y, run["beta"])


def _residual_deviation(A, V, theta, Y, beta):
    m = len(theta)
    U = np.asarray(V, LD).T @ np.asarray(Y, LD)
    true = np.sqrt(np.sum((A.astype(LD) @ U - U * np.asarray(theta, LD)[None, :]) ** 2, axis=0))
    est = np.abs(np.asarray(beta, LD)[m - 1] * np.asarray(Y, LD)[m - 1])
    return float(np.max(np.abs(est - true))) / float(np.max(np.abs(np.linalg.eigvalsh(A))))


NEFF_ALPHAS = (0.01, 1.0, 37.5)


@functools.lru_cache(maxsize=None)
def _neff_inputs():
    e = _rng("neff").standard_normal((5, 300)) * np.logspace(-6, 4, 300)[None, :]
    e[1, 7], e[3, 11], e[3, 12], e[4, :] = 0.0, np.nan, np.inf, -np.abs(e[4, :])
    return e


def _measure():
    out = dict(c=0.0, alpha=0.0, beta=0.0, v=0.0, theta=0.0, TY=0.0, YY=0.0, VV=0.0, ritz=0.0, AU=0.0)
    for name in STEP_CASES:
        d = _step_deviations(_step_ref(name, False), _step_ref(name, True), _step_inputs(name)[1])
        for k, v in d.items():
            out[k] = max(out[k], v)
    for name in TRIDIAG_CASES:
        theta, Y, _, failed = _tridiag_ref(name, False)
        assert not failed
        for k, v in _tridiag_deviations(name, theta, Y).items():
            out[k] = max(out[k], v)
    for name in MATRICES:
        r = _run_ref(name)
        for k in ("VV", "ritz", "AU"):
            out[k] = max(out[k], r[k])
    out["residual"] = max(_residual_ref(20), _residual_ref(40))
    e = _neff_inputs()
    out["neff"] = float(np.max(np.abs(ref.eff_dim(e, NEFF_ALPHAS)[0] - ref.eff_dim(e, NEFF_ALPHAS, wide=True)[0]))) / e.shape[1]
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU

def test_module_constants_are_the_ones_the_shapes_are_built_on():
    from bnn_priors_amd import _hip, eff_dim
    assert (eff_dim.CHUNK, eff_dim.ROWS, eff_dim.MAX_M, eff_dim.MAX_SPLITS) == (CHUNK, ROWS, MAX_M, MAX_SPLITS)
    assert ref.CHUNK == CHUNK and _hip.LANCZOS_WIDTH == WIDTH and _hip.TRIDIAG_MAX_SWEEPS == ref.MAX_SWEEPS
    assert eff_dim.MAX_BATCH == 65535 and _hip.ABI_VERSION >= 27
    lib = _hip.lib()
    for D in (1, CHUNK, CHUNK + 1, 7 * CHUNK - 57, (2 * MAX_SPLITS + 1) * CHUNK - 57, 10 ** 6):
        for ws in (0, WIDTH * 8 - 1, WIDTH * 8, 3 * WIDTH * 8, 256 << 20):
            assert eff_dim.splits(D, ws) == lib.sgmcmc_lanczos_splits(D, ws)
            assert eff_dim.splits(D, ws) * WIDTH * 8 == lib.sgmcmc_lanczos_workspace_bytes(D, ws)
    assert eff_dim.splits(STEP_CASES["default_workspace"][1]) == MAX_SPLITS and eff_dim.splits(7 * CHUNK - 57, 3 * WIDTH * 8) == 3
    assert lib.sgmcmc_lanczos_splits(0, 1 << 20) == -1 and lib.sgmcmc_lanczos_splits(2 ** 31, 1 << 20) == -1


@pytest.mark.parametrize("name", MATRICES)
def test_restatement_of_a_whole_run_against_eigvalsh(name):
    A, _, least = _matrix(name)
    r = _run_ref(name)
    D = A.shape[0]
    print(name, r["restarts"], r["VV"], r["ritz"], r["AU"])
    assert least is None or (r["restarts"] >= least and (least > 0 or r["restarts"] == 0))
    if name in ("identity", "zero"):
        assert r["restarts"] == D - 1
    if name == "rank3":
        assert D - 4 <= r["restarts"] <= D - 3
    assert r["VV"] <= 1e-14
    assert r["ritz"] <= (1e-14 if r["restarts"] == 0 else max(1e-14, ref.default_rtol(D)))
    assert r["AU"] <= (1e-13 if r["restarts"] == 0 else max(1e-13, 4 * ref.default_rtol(D)))


@pytest.mark.parametrize("m", (1, 2, 3, 63, 64, 65, 130))
def test_ql_restatement_against_the_closed_form_of_the_toeplitz_matrix(m):
    theta, Y, sweeps, failed = _tridiag_ref(f"toeplitz{m}", False)
    k = np.arange(1, m + 1)
    exact = 2.0 - 2.0 * np.cos(k * np.pi / (m + 1))
    assert not failed and np.max(np.abs(theta - exact)) <= 8 * EPS * 4.0
    vec = np.sin(np.outer(k, k) * np.pi / (m + 1)) * np.sqrt(2.0 / (m + 1))      # column p: the vector of lambda_p
    assert np.max(np.abs(np.abs(np.sum(vec * Y, axis=0)) - 1.0)) <= 64 * m * EPS


@pytest.mark.parametrize("name", ("wilkinson21", "graded", "diagonal", "identity"))
def test_ql_restatement_against_eigvalsh(name):
    a, b = TRIDIAG_CASES[name]
    theta, Y, sweeps, failed = _tridiag_ref(name, False)
    lam = np.linalg.eigvalsh(_dense_T(a, b).astype(np.float64))
    d = _tridiag_deviations(name, theta, Y)
    print(name, sweeps, d)
    assert not failed and np.max(np.abs(theta - lam)) <= 8 * EPS * np.max(np.abs(lam))
    assert d["TY"] <= 16 * EPS and d["YY"] <= 16 * EPS and np.all(np.diff(theta) >= 0)
    if name == "graded":                                # the small eigenvalues keep their RELATIVE accuracy from this end
        assert np.max(np.abs(theta - lam) / lam) <= 1e-12
    if name in ("diagonal", "identity"):
        assert sweeps == 0 and np.array_equal(theta, np.sort(a)) and np.array_equal(np.abs(Y).sum(axis=0), np.ones(len(a)))
    if name == "diagonal":                              # ties keep their original order: d[2] = d[3] = 2
        assert Y[2, 3] == 1 and Y[3, 4] == 1


def test_ql_restatement_flags_a_nan_and_stops():
    a, b = (x.copy() for x in TRIDIAG_CASES["toeplitz65"])
    a[17] = np.nan
    theta, Y, sweeps, failed = ref.tridiag_eig(a, b)
    assert failed and np.isnan(theta).all() and np.isnan(Y).all() and sweeps <= ref.MAX_SWEEPS * 65


def test_n_eff_restatement_against_a_three_line_sum():
    e = _neff_inputs()
    got, nonpos, nonfin = ref.eff_dim(e, NEFF_ALPHAS)
    for b in range(e.shape[0]):
        lam = e[b][np.isfinite(e[b]) & (e[b] > 0)]
        for i, al in enumerate(NEFF_ALPHAS):
            assert got[b, i] == pytest.approx(float(np.sum(lam / (lam + al))), rel=1e-13, abs=1e-300)
    assert nonfin.tolist() == [0, 0, 0, 2, 0] and nonpos[4] == 300 and nonpos[1] >= 1 and got[4].tolist() == [0, 0, 0]
    vals, small = ref.positive(np.array([-3.0, 0.0, 1e-17, 1e-3, 2.0]))
    assert vals.tolist() == [1.0, 1.0, 1.0, 1e-3, 2.0] and small.tolist() == [True, True, True, False, False]


def _quadratic():
    torch.manual_seed(0)
    P, Q = torch.randn(3, 3, dtype=torch.float64), torch.randn(4, 4, dtype=torch.float64)
    a = torch.randn(3, dtype=torch.float64, requires_grad=True)
    b = torch.randn(2, 2, dtype=torch.float64, requires_grad=True)
    fn = lambda s: s * (a @ P @ a) + 0.5 * s * (b.reshape(-1) @ Q @ b.reshape(-1))      # noqa: E731
    return a, b, P, Q, fn


def test_hessian_of_quadratics_in_two_parameter_tensors():
    from bnn_priors_amd import eff_dim
    a, b, P, Q, fn = _quadratic()
    loader = [(torch.tensor(1.0),), (torch.tensor(2.5),)]                         # the batches are SUMMED: 3.5 times
    H = eff_dim.hessian([a, b], fn, loader)
    assert H.shape == (7, 7) and H.dtype == torch.float64
    assert torch.allclose(H[:3, :3], 3.5 * (P + P.T), rtol=1e-14, atol=0) and torch.allclose(H[3:, 3:], 3.5 * 0.5 * (Q + Q.T), rtol=1e-14, atol=0)
    assert (H[:3, 3:] == 0).all() and (H[3:, :3] == 0).all()
    with pytest.raises(ValueError, match="4096"):
        eff_dim.hessian([torch.zeros(4097, requires_grad=True)], fn, loader)


def _mlp(device="cpu"):
    torch.manual_seed(1)
    W1 = torch.randn(3, 4, dtype=torch.float64, device=device, requires_grad=True)
    b1 = torch.randn(3, dtype=torch.float64, device=device, requires_grad=True)
    W2 = torch.randn(2, 3, dtype=torch.float64, device=device, requires_grad=True)
    x, y = torch.randn(10, 4, dtype=torch.float64, device=device), torch.randn(10, 2, dtype=torch.float64, device=device)
    fn = lambda xb, yb: 0.5 * ((torch.tanh(xb @ W1.T + b1) @ W2.T - yb) ** 2).sum()      # noqa: E731
    return [W1, b1, W2], fn, [(x[:6], y[:6]), (x[6:], y[6:])]


def test_hess_vec_prod_against_the_dense_hessian_and_unflatten_like():
    from bnn_priors_amd import eff_dim
    params, fn, loader = _mlp()
    H = eff_dim.hessian(params, fn, loader)
    assert H.shape == (21, 21) and torch.allclose(H, H.T, rtol=0, atol=1e-13) and torch.linalg.eigvalsh(H)[0] < 0
    v = torch.randn(21, dtype=torch.float64)
    views = eff_dim.unflatten_like(v, params)
    assert [u.shape for u in views] == [p.shape for p in params] and all(u.data_ptr() >= v.data_ptr() for u in views)
    assert torch.equal(torch.cat([u.reshape(-1) for u in views]), v) and views[1].data_ptr() == v[12:].data_ptr()
    hv = eff_dim.hess_vec_prod(v, params, fn, loader)
    assert hv.dtype == torch.float64 and torch.allclose(hv, H @ v, rtol=0, atol=1e-13 * float(H.abs().max() * v.abs().max()) * 21)
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in params]), hv)       # the reference's contract: in p.grad
    assert torch.equal(eff_dim.hess_vec_prod(views, params, fn, loader), hv)
    with pytest.raises(ValueError):
        eff_dim.unflatten_like(v[:-1], params)


def _dense_model(device="cpu"):
    from bnn_priors_amd import models
    torch.manual_seed(2)
    model = models.ClassificationDenseNet(4, 3, 5, 2).double().to(device)
    x = torch.randn(12, 4, dtype=torch.float64, device=device)
    y = torch.randint(0, 3, (12,), device=device)
    return model, x, y


def test_model_hvp_against_the_dense_hessian_of_the_potential():
    from bnn_priors_amd import eff_dim
    model, x, y = _dense_model()
    params = [p for _, p in model.named_parameters()]
    D = sum(p.numel() for p in params)
    assert D == 43
    flags, mode = [p.requires_grad for p in params], model.training
    for what, fn in (("potential", lambda a, b: model.potential(a, b, len(a))),
                     ("likelihood", lambda a, b: -model.log_likelihood(a, b, len(a)))):
        H = eff_dim.hessian(params, fn, [(x, y)])
        full, batched = eff_dim.model_hvp(model, x, y, what), eff_dim.model_hvp(model, x, y, what, batch_size=5)
        scale = float(H.abs().max())
        for seed in range(3):
            v = torch.randn(D, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
            assert torch.allclose(full(v), H @ v, rtol=0, atol=1e-13 * scale * D)
            assert torch.allclose(batched(v), full(v), rtol=0, atol=1e-13 * scale * D)
    assert [p.requires_grad for p in params] == flags and model.training == mode
    with pytest.raises(ValueError, match="what"):
        eff_dim.model_hvp(model, x, y, "prior")
    with pytest.raises(ValueError, match="batch_size"):
        eff_dim.model_hvp(model, x, y, batch_size=0)
    with pytest.raises(ValueError):
        eff_dim.model_hvp(model, x, y[:-1])
    with pytest.raises(ValueError):
        eff_dim.model_hvp(model, x, y)(torch.zeros(D - 1, dtype=torch.float64))


def test_argument_checks():
    from bnn_priors_amd import eff_dim
    A = torch.eye(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="CUDA"):
        eff_dim.lanczos(A, 4)
    with pytest.raises(ValueError, match="CUDA"):
        eff_dim.symeig_positive_lanczos(A)
    with pytest.raises(ValueError, match="CUDA"):
        eff_dim.effective_dimensionality(torch.ones(3, dtype=torch.float64), 1.0)
    with pytest.raises(ValueError, match="CUDA"):
        eff_dim.tridiag_eig(torch.ones(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA"):
        eff_dim.hessian_eigs_positive_lanczos(*_mlp())
    for bad in (torch.eye(4, dtype=torch.float16), torch.ones(4, 5), torch.ones(4), "A"):
        with pytest.raises(ValueError):
            eff_dim.lanczos(bad, 4)
    with pytest.raises(ValueError, match="v0"):
        eff_dim.lanczos(lambda v: v, 4)
    with pytest.raises(ValueError, match=str(MAX_M)):
        eff_dim.symeig_positive_lanczos(torch.zeros(MAX_M + 1, MAX_M + 1))
    with pytest.raises(ValueError):
        eff_dim.effective_dimensionality(torch.ones(3, dtype=torch.int64), 1.0)
    with pytest.raises(ValueError):
        eff_dim.effective_dimensionality(torch.ones(0), 1.0)
    with pytest.raises(ValueError):
        eff_dim.tridiag_eig(torch.ones(3), torch.ones(3))


class _FakeCuda(torch.Tensor):
    "a CPU tensor that claims to be on the device: reaches the checks behind the device check without a GPU"
    is_cuda = True


def _fake(t):
    return t.as_subclass(_FakeCuda)


def test_argument_checks_behind_the_device_check():
    from bnn_priors_amd import eff_dim
    A = _fake(torch.eye(4, dtype=torch.float64))
    for kw in (dict(n_steps=0), dict(n_steps=MAX_M + 1), dict(n_steps=True), dict(n_steps=2, seed=-1),
               dict(n_steps=2, workspace_bytes=WIDTH * 8 - 1), dict(n_steps=2, breakdown_rtol=1.0),
               dict(n_steps=2, v0=torch.ones(4, dtype=torch.float64)), dict(n_steps=2, v0=_fake(torch.ones(5, dtype=torch.float64)))):
        with pytest.raises(ValueError):
            eff_dim.lanczos(A, **kw)
    with pytest.raises(ValueError, match="n_eigs"):
        eff_dim.symeig_positive_lanczos(A, 5)
    with pytest.raises(ValueError, match="n_steps"):
        eff_dim.symeig_positive_lanczos(A, 2, n_steps=1)
    e = _fake(torch.ones(3, dtype=torch.float64))
    for alpha in (0.0, -1.0, float("nan"), float("inf"), []):
        with pytest.raises(ValueError, match="alpha"):
            eff_dim.effective_dimensionality(e, alpha)
    with pytest.raises(ValueError):
        eff_dim.tridiag_eig(_fake(torch.ones(2, 3, dtype=torch.float64)), _fake(torch.ones(2, 4, dtype=torch.float64)))
    with pytest.raises(ValueError):
        eff_dim.tridiag_eig(_fake(torch.ones(1, MAX_M + 1, dtype=torch.float64)), _fake(torch.ones(1, MAX_M + 1, dtype=torch.float64)))


def test_the_recorded_deviations_are_the_measured_ones():
    got = _measure()
    print(got)
    for key, recorded in (("c", C_DEVIATION), ("alpha", ALPHA_DEVIATION), ("beta", BETA_DEVIATION), ("v", V_DEVIATION),
                          ("theta", THETA_DEVIATION), ("TY", TY_DEVIATION), ("YY", YY_DEVIATION), ("VV", VV_DEVIATION),
                          ("ritz", RITZ_DEVIATION), ("AU", AU_DEVIATION), ("residual", RESIDUAL_DEVIATION),
                          ("neff", NEFF_DEVIATION)):
        assert got[key] <= recorded <= max(2 * got[key], EPS * 1.01), (key, got[key], recorded)
    for name in STEP_CASES:                             # the breakdown decisions do not depend on the precision, with a margin
        a, b = _step_ref(name, False), _step_ref(name, True)
        assert a["ok"] == b["ok"] == (name not in BREAKDOWNS), name
        rtol = ref.default_rtol(STEP_CASES[name][1])
        assert (b["norm"] > 100 * rtol * b["scale"]) if b["ok"] else (b["norm"] < 0.01 * rtol * b["scale"]), name


# ------------------------------------------------------------------------------------------------------------------ GPU

def _bound(recorded):
    return 4 * max(recorded, 2.0 ** -53)        # a measured 0 leaves 4 roundings of the quantity: 2^-51


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _gpu_step(V, w, workspace_bytes=None, buffer=None):
    "one step of the kernels on the rows V and w -> what ``ref.step`` returns, and the tensors"
    from bnn_priors_amd import eff_dim
    rows, D = V.shape
    buf = torch.zeros((rows + 1, D), dtype=torch.float64, device="cuda") if buffer is None else buffer
    buf[:rows] = V
    st = eff_dim._Step(buf, eff_dim.WORKSPACE_BYTES if workspace_bytes is None else workspace_bytes)
    w = w.clone()
    st.run(rows - 1, w)
    state = st.state.tolist()
    tensors = (st.coef[:, :rows].clone(), st.alpha[rows - 1].clone(), st.beta[rows - 1].clone(), buf[rows].clone(), w, st.state)
    return dict(c1=st.coef[0, :rows].cpu().numpy(), c2=st.coef[1, :rows].cpu().numpy(), alpha=float(st.alpha[rows - 1]),
                beta=float(st.beta[rows - 1]), norm=state[2], scale=state[0], ok=state[3] == 0, v_next=buf[rows].cpu().numpy(),
                nonfinite=state[4], norm_before=state[5]), tensors


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_step_kernels_against_the_restatement(name):
    from bnn_priors_amd import eff_dim
    rows, D, ws = STEP_CASES[name]
    V, w = _step_inputs(name)
    assert eff_dim.splits(D, eff_dim.WORKSPACE_BYTES if ws is None else ws) == min(-(-D // CHUNK), 3 if ws else MAX_SPLITS)
    got, tensors = _gpu_step(_dev(V), _dev(w), ws)
    again, tensors2 = _gpu_step(_dev(V), _dev(w), ws)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(tensors, tensors2))
    wide = _step_ref(name, True)
    dev = _step_deviations(got, wide, w)
    print(name, dev)
    assert got["ok"] == wide["ok"] and got["nonfinite"] == 0
    assert (got["beta"] == got["norm"]) if got["ok"] else (got["beta"] == 0.0 and not got["v_next"].any())
    assert abs(got["norm_before"] - float(wide["norm_before"])) <= _bound(BETA_DEVIATION) * float(wide["norm_before"])
    assert dev["c"] <= _bound(C_DEVIATION) and dev["alpha"] <= _bound(ALPHA_DEVIATION)
    assert dev["beta"] <= _bound(BETA_DEVIATION) and dev["v"] <= _bound(V_DEVIATION)


@pytest.mark.gpu
def test_a_row_strided_view_gives_the_bits_of_its_contiguous_copy():
    V, w = (_dev(a) for a in _step_inputs("three_splits"))
    rows, D = V.shape
    _, plain = _gpu_step(V, w, 3 * WIDTH * 8)
    every_second = torch.zeros((2 * rows + 2, D), dtype=torch.float64, device="cuda")[::2]
    padded = torch.zeros((rows + 1, D + 37), dtype=torch.float64, device="cuda")[:, 5:D + 5]
    for buffer in (every_second, padded):
        assert not buffer.is_contiguous()
        _, strided = _gpu_step(V, w, 3 * WIDTH * 8, buffer=buffer)
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(plain, strided))
    _, default = _gpu_step(V, w)                        # another workspace is another order: the same to rounding only
    assert torch.allclose(default[0], plain[0], rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_a_restart_step_and_a_non_finite_element():
    from bnn_priors_amd import eff_dim
    V, w = (_dev(a) for a in _step_inputs("rows17"))
    rows, D = V.shape
    buf = torch.zeros((rows + 1, D), dtype=torch.float64, device="cuda")
    buf[:rows] = V
    st = eff_dim._Step(buf)
    st.run(rows - 1, w.clone(), restart=True)
    wide = ref.step(V.cpu().numpy(), w.cpu().numpy(), 0.0, ref.default_rtol(D), True, restart=True)
    state = st.state.tolist()
    assert state[0] == 0 and state[3] == 0 and float(st.alpha[rows - 1]) == 0 and float(st.beta[rows - 1]) == 0
    assert np.max(np.abs(buf[rows].cpu().numpy() - wide["v_next"])) <= _bound(V_DEVIATION) * np.max(np.abs(wide["v_next"]))
    st.run(rows - 1, (V[3] * 2.0).clone(), restart=True)                         # a candidate inside the span: refused
    assert st.state[3].item() == 1 and st.state[1].item() == 0
    w[5], w[77] = float("nan"), float("inf")
    st.run(rows - 1, w.clone())
    assert st.state[4].item() >= 2 and st.state[3].item() == 1
    res = eff_dim.lanczos(_dev(np.diag([1.0, np.nan, 3.0])), 3)                  # counted, NaN outputs, no hang
    assert res.nonfinite >= 1 and all(bool(torch.isnan(t).all()) for t in (res.alpha, res.beta, res.V, res.theta, res.Y))


def _gpu_tridiag(names):
    from bnn_priors_amd import eff_dim
    a = torch.stack([_dev(TRIDIAG_CASES[n][0]) for n in names])
    b = torch.stack([_dev(TRIDIAG_CASES[n][1]) for n in names])
    return eff_dim.tridiag_eig(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TRIDIAG_CASES))
def test_tridiag_eig_against_the_restatement(name):
    theta, Y, sweeps, failed = _gpu_tridiag([name])
    m = len(TRIDIAG_CASES[name][0])
    assert theta.shape == (1, m) and Y.shape == (1, m, m) and int(failed[0]) == 0
    d = _tridiag_deviations(name, theta[0].cpu().numpy(), Y[0].cpu().numpy())
    print(name, int(sweeps[0]), d)
    assert int(sweeps[0]) == _tridiag_ref(name, False)[2] or m > 3        # (the shifts are the restatement's for the tiny ones)
    assert bool((theta[0, 1:] >= theta[0, :-1]).all())
    assert d["theta"] <= _bound(THETA_DEVIATION) and d["TY"] <= _bound(TY_DEVIATION) and d["YY"] <= _bound(YY_DEVIATION)
    if name == "diagonal":
        assert Y[0, 2, 3] == 1 and Y[0, 3, 4] == 1 and int(sweeps[0]) == 0


@pytest.mark.gpu
def test_a_batched_tridiag_launch_gives_the_bits_of_the_single_launches():
    rng = _rng("batch")
    for m in (3, 65):
        a, b = _dev(rng.standard_normal((5, m))), _dev(rng.standard_normal((5, m)))
        a[0], b[0] = (_dev(x) for x in _toeplitz(m))
        from bnn_priors_amd import eff_dim
        batch = eff_dim.tridiag_eig(a, b)
        again = eff_dim.tridiag_eig(a, b)
        for i in range(5):
            single = eff_dim.tridiag_eig(a[i], b[i])
            assert all(torch.equal(_bits(p[i]), _bits(q)) and torch.equal(_bits(p[i]), _bits(r[i]))
                       for p, q, r in zip(batch, single, again))


@pytest.mark.gpu
def test_one_nan_in_a_tridiagonal_gives_a_flag_and_nan_outputs():
    from bnn_priors_amd import eff_dim
    a, b = (_dev(np.stack([x, x])) for x in TRIDIAG_CASES["toeplitz65"])
    a[1, 17] = float("nan")
    theta, Y, sweeps, failed = eff_dim.tridiag_eig(a, b)
    assert failed.tolist() == [0, 1] and bool(torch.isnan(theta[1]).all()) and bool(torch.isnan(Y[1]).all())
    assert bool(torch.isfinite(theta[0]).all()) and int(sweeps[1]) <= ref.MAX_SWEEPS * 65


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("float32", "float64"))
@pytest.mark.parametrize("name", MATRICES)
def test_whole_runs_by_their_invariants(name, dtype):
    from bnn_priors_amd import eff_dim
    A, v0, least = _matrix(name)
    A = _sym(A).astype(dtype)
    if dtype == "float32" and name in ("fivefold", "rank3", "invariant_start"):
        least = None                                    # rounded to float32 the matrix has lost the exact degeneracy
    D = A.shape[0]
    Ad = torch.from_numpy(A).cuda()
    res = eff_dim.lanczos(Ad, D, v0=None if v0 is None else _dev(v0), seed=1)
    U = eff_dim._ritz(res.V, res.theta, res.Y, D, False)
    inv = _run_invariants(A.astype(np.float64), res.V.cpu().numpy(), res.theta.cpu().numpy(), U.cpu().numpy(), res.restarts)
    print(name, dtype, res.restarts, _run_ref(name)["restarts"], inv)
    assert res.m == D and res.nonfinite == 0 and res.V.shape == (D, D) and res.Y.shape == (D, D)
    assert least is None or (res.restarts >= least and (least > 0 or res.restarts == 0))
    if name in ("identity", "zero"):
        assert res.restarts == D - 1 == _run_ref(name)["restarts"]
    rtol = ref.default_rtol(D) if res.restarts else 0.0
    assert inv["VV"] <= _bound(VV_DEVIATION)
    assert inv["ritz"] <= max(_bound(RITZ_DEVIATION), rtol)
    assert inv["AU"] <= max(_bound(AU_DEVIATION), 4 * rtol)
    assert bool((res.Y[0] * torch.sign(res.Y[0]) >= 0).all()) and torch.equal(res.residual, (res.beta[D - 1] * res.Y[D - 1]).abs())


@pytest.mark.gpu
@pytest.mark.parametrize("m", (20, 40))
def test_the_residual_estimate_against_the_true_residual(m):
    from bnn_priors_amd import eff_dim
    A = _sym(_matrix("psd130")[0])
    res = eff_dim.lanczos(_dev(A), m, seed=2)
    assert res.m == m and res.restarts == 0 and res.V.shape == (m, 130)
    got = _residual_deviation(A, res.V.cpu().numpy(), res.theta.cpu().numpy(), res.Y.cpu().numpy(), res.beta.cpu().numpy())
    print(m, got, _residual_ref(m))
    assert got <= _bound(RESIDUAL_DEVIATION)
    assert torch.equal(res.residual, (res.beta[m - 1] * res.Y[m - 1]).abs())
    top = np.linalg.eigvalsh(A)[-1]
    assert abs(float(res.theta[-1]) - top) <= max(float(res.residual[-1]), 1e-12 * top)      # the top pair has converged


@pytest.mark.gpu
def test_ritz_vectors_on_the_matrix_pipe_against_the_restatement():
    from bnn_priors_amd import eff_dim
    rng = _rng("ritz")
    for m, D, k in ((1, 1, 1), (3, 65, 2), (37, 200, 17), (130, 7 * 64 + 5, 33)):
        V, Y = rng.standard_normal((m, D)), rng.standard_normal((m, m))
        theta = np.sort(rng.standard_normal(m))
        if m > 2:                                       # an exact zero and a negative value among the k largest: both small
            theta = theta - theta[min(m - k + 1, m - 2)]
        cols = np.arange(m - k, m)
        for rule in (False, True):
            wide = ref.ritz(V, Y, cols, theta, rule, wide=True)
            plain = ref.ritz(V, Y, cols, theta, rule)
            padded = torch.zeros((m, D + 3), dtype=torch.float64, device="cuda")[:, :D]
            padded[:] = _dev(V)
            got = eff_dim._ritz(padded, _dev(theta), _dev(Y), k, rule)
            assert torch.equal(_bits(got), _bits(eff_dim._ritz(_dev(V), _dev(theta), _dev(Y), k, rule)))
            scale = float(np.max(np.sqrt(np.sum(V.astype(LD) ** 2, axis=0)))) * float(np.max(np.sqrt(np.sum(Y.astype(LD) ** 2, axis=0))))
            measured = float(np.max(np.abs(plain - wide))) / scale
            assert float(np.max(np.abs(got.cpu().numpy() - wide))) / scale <= 4 * max(measured, 2.0 ** -53)
            zero = ref.positive(theta)[1][cols] & rule
            assert not got.cpu().numpy()[:, zero].any() and (zero.any() or not rule or m <= 2)


@pytest.mark.gpu
def test_n_eff_against_the_restatement():
    from bnn_priors_amd import eff_dim
    e = _neff_inputs()
    wide, nonpos, nonfin = ref.eff_dim(e, NEFF_ALPHAS, wide=True)
    got, gp, gf = eff_dim.effective_dimensionality(_dev(e), list(NEFF_ALPHAS))
    assert got.shape == (5, 3) and gp.tolist() == nonpos.tolist() and gf.tolist() == nonfin.tolist()
    assert float(np.max(np.abs(got.cpu().numpy() - wide))) / e.shape[1] <= _bound(NEFF_DEVIATION)
    one, _, _ = eff_dim.effective_dimensionality(_dev(e)[2], 1.0)                 # a row and an alpha of the batch: its bits
    assert one.shape == (1,) and torch.equal(_bits(one), _bits(got[2, 1:2]))
    f32, _, _ = eff_dim.effective_dimensionality(_dev(e).float()[:3].reshape(3, 1, 300), torch.tensor(NEFF_ALPHAS))
    assert f32.shape == (3, 1, 3) and f32.dtype == torch.float64


@pytest.mark.gpu
def test_symeig_positive_lanczos_against_eigh():
    from bnn_priors_amd import eff_dim
    M = _psd(8, _rng("symeig"))
    lam, vec = np.linalg.eigh(M)
    vals, vecs = eff_dim.symeig_positive_lanczos(_dev(M), -1, vecs=True)
    assert vals.shape == (8,) and vecs.shape == (8, 8)
    assert np.max(np.abs(vals.cpu().numpy() - lam)) <= _bound(RITZ_DEVIATION) * lam[-1]
    overlap = np.abs(np.sum(vecs.cpu().numpy() * vec, axis=0))                   # the sign is free
    assert np.max(np.abs(overlap - 1.0)) <= 1e-10
    top, none = eff_dim.symeig_positive_lanczos(_dev(M), 3, n_steps=8)
    assert none is None and torch.equal(_bits(top), _bits(vals[5:]))
    with pytest.raises(ValueError, match=str(MAX_M)):
        eff_dim.symeig_positive_lanczos(torch.zeros(MAX_M + 1, MAX_M + 1, device="cuda"))


@pytest.mark.gpu
def test_hessian_eigs_positive_lanczos_on_the_tanh_mlp():
    from bnn_priors_amd import eff_dim
    params, fn, loader = _mlp("cuda")
    H = eff_dim.hessian(params, fn, loader).cpu().numpy()
    lam, vec = np.linalg.eigh(_sym(H))
    negative = int((lam < 0).sum())
    assert negative >= 1
    grads = [p.grad for p in params]
    vals, vecs = eff_dim.hessian_eigs_positive_lanczos(params, fn, loader, -1, vecs=True)
    vals, vecs = vals.cpu().numpy(), vecs.cpu().numpy()
    assert all(p.grad is g for p, g in zip(params, grads))
    assert (vals[:negative] == 1.0).all() and not vecs[:, :negative].any()
    keep = lam > 21 * EPS * np.max(np.abs(lam)) * 1e3                            # clear of the positive rule's threshold
    assert keep.sum() >= 21 - negative - 1
    assert np.max(np.abs(vals[keep] - lam[keep])) <= 1e-11 * np.max(np.abs(lam))
    assert np.max(np.abs(np.abs(np.sum(vecs[:, keep] * vec[:, keep], axis=0)) - 1.0)) <= 1e-8


def _loader(x, y, batch):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, y), batch_size=batch)


@pytest.mark.gpu
def test_evaluate_eff_dim_equals_the_dense_hessian_and_the_separate_calls():
    from bnn_priors_amd import eff_dim, evaluation
    model, x, y = _dense_model("cuda")
    params = [p for _, p in model.named_parameters()]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(5)
    samples = {k: (v.detach()[None] + 0.3 * torch.randn((3, *v.shape), dtype=v.dtype, generator=gen).cuda())
               for k, v in model.named_parameters()}
    alphas = [0.1, 1.0]
    out = evaluation.evaluate_eff_dim(model, _loader(x, y, 5), samples, n_eigs=-1, alpha=alphas, what="potential")
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert out["dimension"] == 43 and len(out["eigenvalues"]) == 3 and len(out["eigenvalues"][0]) == 43
    assert isinstance(out["negative"], int) and isinstance(out["restarts"], int) and isinstance(out["max_residual"], float)
    per = []
    for s in range(3):
        model.load_state_dict({k: v[s] for k, v in samples.items()}, strict=False)
        H = eff_dim.hessian(params, lambda a, b: model.potential(a, b, len(a)), [(x, y)]).cpu().numpy()
        lam = np.linalg.eigvalsh(_sym(H))
        assert np.max(np.abs(np.array(out["eigenvalues"][s]) - lam)) <= 1e-10 * np.max(np.abs(lam))
        pos = lam[lam > 0]
        per.append([float(np.sum(pos / (pos + a))) for a in alphas])
        hvp = eff_dim.model_hvp(model, x, y, "potential", batch_size=5)
        v0 = torch.randn(43, generator=torch.Generator(device="cuda").manual_seed(0), device="cuda", dtype=torch.float64)
        res = eff_dim.lanczos(hvp, 43, v0=v0)
        assert torch.equal(_bits(res.theta), _bits(torch.tensor(out["eigenvalues"][s], dtype=torch.float64).cuda()))
        sep = eff_dim.effective_dimensionality(res.theta, alphas)[0]
        assert sep.tolist() == out["eff_dim_per_sample"][s]
    model.load_state_dict(before)
    assert np.max(np.abs(np.array(out["eff_dim_per_sample"]) - np.array(per))) <= 1e-8
    assert np.max(np.abs(np.array(out["eff_dim"]) - np.mean(per, axis=0))) <= 1e-8


@pytest.mark.gpu
def test_evaluate_eff_dim_on_a_float32_convnet_runs_on_the_plain_layers():
    from bnn_priors_amd import bn, bnlink, conv, evaluation, models, pool, resblock
    torch.manual_seed(3)
    model = models.ClassificationConvNet(1, 4, 3, 4, 2).cuda()
    x, y = torch.randn(6, 1, 4, 4, device="cuda"), torch.randint(0, 3, (6,), device="cuda")
    switches = [m.ENABLED for m in (bn, bnlink, conv, pool, resblock)]
    samples = {k: v[None].clone() for k, v in model.state_dict().items()}
    out = evaluation.evaluate_eff_dim(model, _loader(x, y, 6), samples, n_eigs=2, n_steps=5)
    assert [m.ENABLED for m in (bn, bnlink, conv, pool, resblock)] == switches and all(switches)
    assert out["dimension"] == sum(p.numel() for p in model.parameters())
    assert np.isfinite(out["eff_dim"]).all() and np.isfinite(out["eigenvalues"]).all() and len(out["eigenvalues"][0]) == 2
    assert np.isfinite(out["max_residual"]) and 0 <= out["eff_dim"][0] <= 2
