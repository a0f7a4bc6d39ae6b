"""Kernel Stein discrepancy, its wild bootstrap test and Stein thinning on the device (bnn_priors_amd/stein.py,
csrc/stein_hip.inc; definitions in include/sgmcmc_hip.h, restated in tests/stein_reference.py).

On the CPU the restatement is held to independent code (torch.autograd on the base kernel, a quadrature of the Stein
identity, a brute-force thinning), ``scores`` to closed forms, the wrappers to their argument checks.  On the GPU the
kernels are held to the restatement.

Shapes.  The Gram pass forms TILE x TILE = 64 x 64 blocks of the 2S rows [X - x_0; G] from chunks of KC = CHUNK = 32
coordinates, ``splits(S, D, workspace_bytes)`` workgroups sharing the chunks of a block pair.  S in {2, 17, 32, 33, 64,
65}: the X / G boundary inside the first tile (2, 17), on its edge (32: exactly one tile), just past one tile (33), on the
edge of two (64), and three tile rows with a partial last (65); 17 and 65 are also the test of the fp64 MFMA's C/D lane map.
D in {1, 2, KC - 1, KC + 1}, and 2 splits + 1 chunks with a ragged tail at the default workspace (64 splits) and at one that
leaves 3.

Tolerances.  They are measured, not guessed: the restatement is evaluated on the GPU tests' own inputs in np.float64 (the
anchor / Gram form of the kernels) and in np.longdouble (the difference form), the largest deviation per quantity over all
cases is recorded, and the GPU tolerance is 4 x that against the longdouble values (the factor allows for the kernels'
other summation order and the MFMA's internal order).  Scales:

  K         relative to sqrt(K_ii K_jj)                          measured 6.90e-15 (K_DEVIATION = 7.0e-15)
  r2        relative to sqrt(s_i s_j), s_i = mean_j r2_ij, the mean squared distance of sample i from the others (r2 itself
            is 0 on the diagonal and arbitrarily small for near-duplicates)
                                                                 measured 2.87e-15 (R2_DEVIATION = 2.9e-15)
  v_stat    relative                                             measured 2.80e-15 (V_DEVIATION = 2.9e-15)
  u_stat    relative to v_stat                                   measured 3.36e-15 (U_DEVIATION = 3.4e-15)
  row_mean  relative to its largest element in magnitude (a single row mean may cross 0)
                                                                 measured 5.09e-15 (ROW_DEVIATION = 5.1e-15)
  ksd_path  relative, with equal indices                         measured 3.35e-14 (PATH_DEVIATION = 3.4e-14)
  null      the wild bootstrap's Q_r (S = 200, D = 5), relative to v_stat
                                                                 measured 9.30e-16 (NULL_DEVIATION = 9.4e-16)

The case S = 65, D = 1 sets the first six: with one coordinate r2 and t are differences of single products, and 65 draws on
a line come close to each other; the other cases stay below 3.4e-15.  The ``far`` cases (every coordinate 1e4 standard
deviations from 0) are among them: the anchor makes x - x_0 exact for fp32 input and, here, for fp64 input too.
``test_the_recorded_deviations_are_the_measured_ones`` re-measures them, and shows that the uncentred Gram form misses the
fp64 ``far`` case by more than 1e4 times R2_DEVIATION.
"""
import functools

import numpy as np
import pytest
import torch

import stein_reference as ref

K_DEVIATION = 7.0e-15
R2_DEVIATION = 2.9e-15
V_DEVIATION = 2.9e-15
U_DEVIATION = 3.4e-15
ROW_DEVIATION = 5.1e-15
PATH_DEVIATION = 3.4e-14
NULL_DEVIATION = 9.4e-16
BOOT_SEED = 3
USE_SEED = 0
BOOT_S, BOOT_D, BOOT_R = 200, 5, 199

LD = np.longdouble
KC, TILE = 32, 64                    # asserted against the module's constants below
SMALL = 3 * 8 * 130 * 130            # a workspace that leaves 3 splits at S = 65
QUANTITIES = ("K", "r2", "v_stat", "u_stat", "row_mean", "ksd_path")

# name: (S, D, dtype, beta, c, special, workspace_bytes or None)
#   special: "far" every coordinate of x offset by 1e4 standard deviations, "dup" rows 3 and 7 identical, "bad" one NaN in
#   x and one Inf in the score
CASES = {}
for _i, _S in enumerate((2, 17, 32, 33, 64, 65)):
    for _j, _D in enumerate((1, 2, KC - 1, KC + 1)):
        CASES[f"s{_S}_d{_D}"] = (_S, _D, ("float32", "float64")[(_i + _j) % 2], (-0.5, -0.3)[(_i + _j // 2) % 2], 1.0, "",
                                 None)
CASES.update({
    "s17_all_splits": (17, 128 * KC + 5, "float32", -0.5, 1.0, "", None),             # 129 chunks, 64 splits, ragged
    "s65_three_splits": (65, 7 * KC - 9, "float64", -0.3, 1.0, "", SMALL),            # 7 chunks, 3 splits, ragged
    "s65_three_splits_f32": (65, 7 * KC - 9, "float32", -0.5, 2.0, "", SMALL),
    "median": (33, KC + 1, "float32", -0.5, "median", "", None),
    "median_beta": (18, 3, "float64", -0.3, "median", "", None),
    "far": (20, 6, "float64", -0.5, 1.0, "far", None),
    "far_f32": (20, 6, "float32", -0.5, 1.0, "far", None),
    "duplicates": (12, 5, "float32", -0.5, 1.0, "dup", None),
    "nan_inf": (9, 4, "float32", -0.5, 1.0, "bad", None),
})


@functools.lru_cache(maxsize=None)
def _inputs(name):
    "(x [S, D], score [S, D]) of a case as read-only numpy arrays: draws of N(0.3, 1) with the score of a nearby target"
    S, D, dtype, _, _, special, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 200)
    z = rng.standard_normal((S, D))
    g = -(z * 1.1) + 0.2 * rng.standard_normal((S, D))
    x = z + 0.3
    if special == "far":
        x = x + 1e4
    if special == "dup":
        x[7], g[7] = x[3], g[3]
    x, g = x.astype(dtype), g.astype(dtype)
    if special == "bad":
        x[2, 1], g[5, 3] = np.nan, np.inf
    x.setflags(write=False), g.setflags(write=False)
    return x, g


def _picks(name):
    return CASES[name][0] // 2 + 1


@functools.lru_cache(maxsize=None)
def _ref(name, wide):
    "the restatement of a case: the Stein matrix, its statistics and a thinning of S / 2 + 1 picks"
    S, D, dtype, beta, c, special, _ = CASES[name]
    out = ref.stein_matrix(*_inputs(name), c=c, beta=beta, wide=wide)
    out.update(ref.ksd_stats(out["K"]))
    out["indices"], out["ksd_path"] = ref.thin(out["K"], _picks(name))
    return out


def _boot_inputs(shifted):
    "exact N(0, I) draws (or the same shifted by 0.5 in every coordinate) and the target's score -x at them"
    x = np.random.default_rng(BOOT_SEED).standard_normal((BOOT_S, BOOT_D)) + (0.5 if shifted else 0.0)
    return x, -x


@functools.lru_cache(maxsize=None)
def _boot_signs():
    return ref.sign_process(np.random.default_rng(BOOT_SEED + 1000).random((BOOT_R, BOOT_S)), 0.5)


@functools.lru_cache(maxsize=None)
def _boot_ref(shifted, wide):
    return ref.wild_bootstrap(ref.stein_matrix(*_boot_inputs(shifted), wide=wide)["K"], _boot_signs())


@functools.lru_cache(maxsize=None)
def _use_inputs():
    "S = 300 draws of N(0, I) in two dimensions of which every third is shifted by 2 in every coordinate"
    x = np.random.default_rng(USE_SEED).standard_normal((300, 2))
    x[::3] += 2.0
    return x, -x


def _deviations(got, wide):
    "largest deviation per quantity of a result (dict as ``_ref``'s) from the longdouble restatement"
    if wide["nonfinite"]:
        return dict.fromkeys(QUANTITIES, 0.0)
    dk = np.sqrt(np.diag(wide["K"]))
    s = wide["r2"].mean(axis=1)
    out = dict(K=np.max(np.abs(LD(1) * got["K"] - wide["K"]) / np.outer(dk, dk)),
               r2=np.max(np.abs(LD(1) * got["r2"] - wide["r2"]) / np.sqrt(np.outer(s, s))),
               v_stat=abs(LD(1) * got["v_stat"] - wide["v_stat"]) / abs(wide["v_stat"]),
               u_stat=abs(LD(1) * got["u_stat"] - wide["u_stat"]) / abs(wide["v_stat"]),
               row_mean=np.max(np.abs(LD(1) * got["row_mean"] - wide["row_mean"])) / np.max(np.abs(wide["row_mean"])),
               ksd_path=np.max(np.abs(LD(1) * got["ksd_path"] - wide["ksd_path"]) / wide["ksd_path"]))
    return {k: float(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _measure():
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for name in CASES:
        for k, v in _deviations(_ref(name, False), _ref(name, True)).items():
            worst[k] = max(worst[k], v)
    worst["null"] = 0.0
    for shifted in (False, True):
        a, b = _boot_ref(shifted, False), _boot_ref(shifted, True)
        worst["null"] = max(worst["null"], float(np.max(np.abs(LD(1) * a["null"] - b["null"])) / b["v_stat"]))
        worst["v_stat"] = max(worst["v_stat"], float(abs(LD(1) * a["v_stat"] - b["v_stat"]) / b["v_stat"]))
    return worst


# ------------------------------------------------------------------------------------------------------------------ CPU

def test_module_constants_are_the_ones_the_shapes_are_built_on():
    from bnn_priors_amd import _hip, stein
    assert (stein.CHUNK, stein.TILE, stein.MAX_S, stein.MAX_PICKS, stein.MAX_D) == (KC, TILE, 1024, 2 ** 20, 2 ** 31 - 1)
    assert stein.splits(17, 128 * KC + 5) == 64 and -(-(128 * KC + 5) // KC) == 2 * 64 + 1      # two each, one a third
    assert stein.splits(65, 7 * KC - 9, SMALL) == 3 and -(-(7 * KC - 9) // KC) == 2 * 3 + 1 and (7 * KC - 9) % KC
    assert stein.splits(65, 100, 8 * 130 * 130 - 1) == 0
    lib = _hip.lib()
    for S, D, ws in ((2, 1, 1 << 20), (32, 31, 1 << 28), (65, 215, SMALL), (17, 4101, 1 << 28), (1024, 10 ** 6, 1 << 28),
                     (1024, 2 ** 31 - 1, 1 << 26), (100, 79510, 1 << 28), (512, 272000, 1 << 28), (300, 77, 0)):
        assert stein.splits(S, D, ws) == lib.sgmcmc_stein_splits(S, D, ws), (S, D, ws)
    assert lib.sgmcmc_stein_splits(1025, 10, 1 << 20) == -1 and lib.sgmcmc_stein_splits(1, 10, 1 << 20) == -1
    assert lib.sgmcmc_stein_splits(4, 0, 1 << 20) == -1 and lib.sgmcmc_stein_splits(4, 2 ** 31, 1 << 20) == -1


@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("beta", (-0.5, -0.3))
def test_restatement_against_autograd_on_the_base_kernel(D, beta):
    """k_p(x, y) = tr(grad_x grad_y k) + grad_x k . s(y) + grad_y k . s(x) + k s(x) . s(y) of k = (c^2 + |x - y|^2)^beta,
    every derivative by torch.autograd in float64"""
    rng = np.random.default_rng(7 + D)
    S, c = 5, 1.3
    x, g = rng.standard_normal((S, D)), rng.standard_normal((S, D))
    want = np.zeros((S, S))
    for i in range(S):
        for j in range(S):
            a = torch.tensor(x[i], requires_grad=True)
            b = torch.tensor(x[j], requires_grad=True)
            k = (c * c + ((a - b) ** 2).sum()) ** beta
            ga, gb = torch.autograd.grad(k, (a, b), create_graph=True)
            trace = sum(torch.autograd.grad(ga[q], b, retain_graph=True)[0][q] for q in range(D))
            si, sj = torch.tensor(g[i]), torch.tensor(g[j])
            want[i, j] = float((trace + ga @ sj + gb @ si + k * (si @ sj)).detach())
    for wide in (False, True):
        got = ref.stein_matrix(x, g, c=c, beta=beta, wide=wide)
        assert got["d"] == D and got["nonfinite"] == 0 and got["K"].dtype == (LD if wide else np.float64)
        assert np.max(np.abs(got["K"] - want)) < 1e-13 * np.max(np.abs(want))
        assert np.array_equal(got["K"], got["K"].T) and (np.diag(got["r2"]) == 0).all()
    halves = ref.stein_matrix({"a": x[:, :1], "b": x}, {"a": g[:, :1], "b": g}, c=c, beta=beta, wide=True)
    whole = ref.stein_matrix(np.hstack([x[:, :1], x]), np.hstack([g[:, :1], g]), c=c, beta=beta, wide=True)
    assert halves["d"] == D + 1 and np.max(np.abs(halves["K"] - whole["K"])) < 1e-17 * np.max(np.abs(whole["K"]))


@pytest.mark.parametrize("beta", (-0.5, -0.3))
def test_stein_identity_for_a_standard_normal_by_quadrature(beta):
    """E_{x, y ~ p} k_p(x, y) = 0 for p = N(0, 1) with its own score -x: the trapezoid rule on [-12, 12]^2 (spectrally
    accurate for an analytic integrand that has decayed to e^-72 at the edge) at two step sizes; the difference of the two
    is the quadrature's own error, next to the rounding of the sum."""
    values = []
    for n in (241, 481):
        x = np.linspace(-12, 12, n).reshape(n, 1)
        K = ref.stein_matrix(x, -x, c=1.0, beta=beta, wide=True)["K"]
        w = np.exp(-(x[:, 0].astype(LD) ** 2) / 2) / np.sqrt(2 * LD(np.pi)) * (x[1, 0] - x[0, 0])
        values.append((w @ K @ w, np.abs(w) @ np.abs(K) @ np.abs(w)))
        assert abs(w.sum() - 1) < 1e-13
    (coarse, _), (fine, mass) = values
    print(float(coarse), float(fine), float(mass))
    assert mass > 0.5 and abs(fine) <= abs(fine - coarse) + 1e-17 * mass and abs(fine - coarse) < 1e-12
    # ... and it is not 0 for draws of another distribution: p = N(0.5, 1) with the score of N(0, 1)
    x = np.linspace(-12, 12, 241).reshape(241, 1)
    K = ref.stein_matrix(x, -x, wide=False)["K"]
    w = np.exp(-((x[:, 0] - 0.5) ** 2) / 2) / np.sqrt(2 * np.pi) * 0.1
    assert w @ K @ w > 0.05


def _brute_force_thinning(K, m):
    "the full objective K_jj / 2 + sum_{a < m} K(pi_a, j) recomputed at every pick, the double sum of every prefix too"
    picks, path = [], []
    for _ in range(m):
        obj = [K[j, j] / 2 + sum(K[p, j] for p in picks) for j in range(K.shape[0])]
        picks.append(min(range(K.shape[0]), key=lambda j: (obj[j], j)))
        path.append(np.sqrt(sum(K[p, q] for p in picks for q in picks)) / len(picks))
    return picks, path


def _integer_K(S, seed=0):
    "a symmetric matrix of small non-negative integers: many equal entries (ties at every pick), every sum positive"
    rng = np.random.default_rng(seed + S)
    B = rng.integers(0, 3, size=(S, S))
    K = (B + B.T).astype(np.float64)
    K[np.arange(S), np.arange(S)] = rng.integers(6, 9, size=S)
    return K


def test_thinning_restatement_against_a_brute_force():
    for S, m in ((2, 5), (9, 9), (30, 41)):
        K = _integer_K(S)
        idx, path = ref.thin(K, m)
        picks, want = _brute_force_thinning(K, m)
        assert idx.tolist() == picks and np.array_equal(path, np.array(want))          # integers: exact
    K = np.random.default_rng(3).standard_normal((12, 40))
    K = K @ K.T
    idx, path = ref.thin(K, 20)
    picks, want = _brute_force_thinning(K, 20)
    assert idx.tolist() == picks and np.max(np.abs(path - want) / want) < 1e-13
    assert len(set(picks)) < 20                                                         # picks repeat
    K = np.full((4, 4), 1.0) + 2 * np.eye(4)                                            # all equal: the first index
    assert ref.thin(K, 3)[0].tolist() == [0, 1, 2] and ref.thin(K, 6)[0].tolist() == [0, 1, 2, 3, 0, 1]
    assert ref.thin(np.full((3, 3), np.nan), 2)[0].tolist() == [0, 0]


def test_sign_process_and_p_value():
    u = np.array([[0.4, 0.6, 0.1, 0.9], [0.7, 0.2, 0.2, 0.8]])
    assert ref.sign_process(u, 0.5).tolist() == [[-1, -1, 1, 1], [1, -1, 1, 1]]
    assert ref.sign_process(u, 0.15).tolist() == [[-1, -1, 1, 1], [1, 1, 1, 1]]          # the first sign stays fair
    assert ref.p_value([1.0, 2.0, 3.0], 2.0) == 3 / 4 and ref.p_value([1.0], 5.0) == 1 / 2
    w = ref.sign_process(np.random.default_rng(0).random((2000, 50)), 0.1)
    assert abs(w[:, 0].mean()) < 0.1 and abs((w[:, 1:] != w[:, :-1]).mean() - 0.1) < 0.01


def test_scores_of_a_gaussian_model_in_closed_form():
    from bnn_priors_amd import stein
    from bnn_priors_amd.models import GaussianModel
    mean, std, T = 0.7, 1.5, 2.0
    model = GaussianModel(2, 3, mean, std)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    training = model.training
    samples = {"0.p": torch.randn(6, 3, generator=torch.Generator().manual_seed(1)),
               "1.p": torch.randn(6, 3, generator=torch.Generator().manual_seed(2))}
    got = stein.scores(model, samples, temperature=T)
    assert sorted(got) == ["0.p", "1.p"]
    for k in got:
        assert got[k].shape == (6, 3) and torch.allclose(got[k], -(samples[k] - mean) / std ** 2 / T, rtol=1e-5, atol=1e-6)
    assert model.training == training and all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    assert not any(p.grad is not None for p in model.parameters())
    only = stein.scores(model, {"1.p": samples["1.p"]})
    assert sorted(only) == ["1.p"] and torch.allclose(only["1.p"], got["1.p"] * T)
    with pytest.raises(ValueError, match="temperature"):
        stein.scores(model, samples, temperature=0.0)
    with pytest.raises(ValueError, match="does not"):
        stein.scores(model, {"0.p": samples["0.p"], "nope": samples["0.p"]})
    with pytest.raises(ValueError, match="together"):
        stein.scores(model, samples, x=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="batch_size"):
        stein.scores(model, samples, batch_size=0)


def test_scores_in_batches_equal_the_full_batch_call():
    from bnn_priors_amd import stein
    from bnn_priors_amd.models import ClassificationDenseNet
    torch.manual_seed(3)
    model = ClassificationDenseNet(4, 3, 5, 2).double()
    model.eval()
    x, y = torch.randn(12, 4, dtype=torch.float64), torch.randint(0, 3, (12,))
    samples = {k: torch.stack([v.detach() + 0.1 * i for i in range(3)]) for k, v in model.named_parameters()}
    full = stein.scores(model, samples, x, y)
    parts = stein.scores(model, samples, x, y, batch_size=5)
    assert not model.training
    for k in full:
        assert full[k].dtype == torch.float64 and full[k].shape == samples[k].shape
        assert float((full[k] - parts[k]).abs().max() / full[k].abs().max()) <= 1e-12
    # ... and it is the gradient of -potential: a central difference along one direction at sample 1
    k0 = "net.0.weight_prior.p"
    model.load_state_dict({k: v[1] for k, v in samples.items()}, strict=False)
    p = dict(model.named_parameters())[k0]
    direction = torch.randn(p.shape, dtype=torch.float64)
    with torch.no_grad():
        p += 1e-5 * direction
        up = model.potential(x, y, 12)
        p -= 2e-5 * direction
        down = model.potential(x, y, 12)
    assert abs(float(-(up - down) / 2e-5) - float((full[k0][1] * direction).sum())) < 1e-6 * float(full[k0][1].norm())


def test_argument_checks():
    from bnn_priors_amd import stein
    x = torch.zeros(6, 5)
    for bad, match in ((torch.zeros(6, 5, dtype=torch.int64), "float32 or float64"), (torch.zeros(7), r"\[S, D\]"),
                       (torch.zeros(6, 0), "empty"), ([[1.0]], "float32 or float64"), (torch.zeros(2, 3, 4), r"\[S, D\]")):
        with pytest.raises(ValueError, match=match):
            stein.kernel_matrix(bad, bad)
    with pytest.raises(ValueError, match="differ in shape or dtype"):
        stein.kernel_matrix(x, torch.zeros(6, 4))
    with pytest.raises(ValueError, match="differ in shape or dtype"):
        stein.kernel_matrix(x, x.double())
    with pytest.raises(ValueError, match="2 .. 1024"):
        stein.kernel_matrix(torch.zeros(1, 5), torch.zeros(1, 5))
    with pytest.raises(ValueError, match="2 .. 1024"):
        stein.kernel_matrix(torch.zeros(1025, 1), torch.zeros(1025, 1))
    with pytest.raises(ValueError, match="both be tensors or both be dicts"):
        stein.kernel_matrix({"a": x}, x)
    with pytest.raises(ValueError, match="same keys"):
        stein.kernel_matrix({"a": x}, {"b": x})
    with pytest.raises(ValueError, match="same keys"):
        stein.kernel_matrix({}, {})
    with pytest.raises(ValueError, match="holds 5 samples"):
        stein.kernel_matrix({"a": x, "b": torch.zeros(5, 2)}, {"a": x, "b": torch.zeros(5, 2)})
    for beta in (0.0, -1.0, 0.5, None, True):
        with pytest.raises(ValueError, match="beta"):
            stein.kernel_matrix(x, x, beta=beta)
    for c in (0.0, -1.0, "mean", None, float("inf"), True):
        with pytest.raises(ValueError, match="c = "):
            stein.kernel_matrix(x, x, c=c)
    with pytest.raises(ValueError, match="workspace_bytes = 1151"):
        stein.kernel_matrix(x, x, workspace_bytes=32 * 36 - 1)
    with pytest.raises(ValueError, match="workspace_bytes"):
        stein.kernel_matrix(x, x, workspace_bytes=-1)
    with pytest.raises(ValueError, match="no CPU path"):
        stein.kernel_matrix(x, x)
    with pytest.raises(ValueError, match="no CPU path"):
        stein.kernel_matrix({"a": x.reshape(6, 5, 1)}, {"a": x.reshape(6, 5, 1)}, c="median")
    K = torch.eye(4, dtype=torch.float64)
    for fn in (stein.ksd, lambda k: stein.thin(k, 2), lambda k: stein.quadratic_forms(k, torch.ones(4, dtype=torch.float64)),
               stein.wild_bootstrap_test):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(K)
        for bad in (torch.eye(4), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), None):
            with pytest.raises(ValueError, match=r"\[S, S\]"):
                fn(bad)
        with pytest.raises(ValueError, match="2 .. 1024"):
            fn(torch.zeros(1, 1, dtype=torch.float64))


def _fake_device_K(S=4):
    "a host tensor that says it is on the device: for the argument checks that come after the device check"
    class OnDevice(torch.Tensor):
        is_cuda = True
    return torch.eye(S, dtype=torch.float64).as_subclass(OnDevice)


def test_argument_checks_behind_the_device_check():
    from bnn_priors_amd import stein
    K = _fake_device_K()
    for m in (0, 2 ** 20 + 1, 2.0, None, True):
        with pytest.raises(ValueError, match="m = "):
            stein.thin(K, m)
    for W in (torch.ones(4), torch.ones(3, dtype=torch.float64), torch.ones(2, 2, 4, dtype=torch.float64),
              [1.0] * 4):
        with pytest.raises(ValueError, match=r"W must be a float64"):
            stein.quadratic_forms(K, W)
    with pytest.raises(ValueError, match="R = 0"):
        stein.quadratic_forms(K, torch.ones(0, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="no CPU path"):
        stein.quadratic_forms(K, torch.ones(4, dtype=torch.float64))
    for replicates in (0, 65536, 9.0):
        with pytest.raises(ValueError, match="replicates"):
            stein.wild_bootstrap_test(K, replicates=replicates)
    for flip_prob in (0.0, 1.5, None):
        with pytest.raises(ValueError, match="flip_prob"):
            stein.wild_bootstrap_test(K, flip_prob=flip_prob)
    with pytest.raises(ValueError, match="seed"):
        stein.wild_bootstrap_test(K, seed=0.5)
    for signs in (torch.ones(4, dtype=torch.float64), torch.ones(3, 4), torch.ones(3, 5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="signs must be"):
            stein.wild_bootstrap_test(K, signs=signs)


def test_the_wild_bootstrap_data_separate_the_exact_draws_from_the_shifted_ones():
    """BOOT_SEED = 3, by the restatement in both precisions: p = 0.51 on the exact N(0, I) draws and 0.005 = 1 / (R + 1) on
    the draws shifted by 0.5; the null value nearest to the observed one is 8.7e-4 of it away on the exact draws (and
    0.84 on the shifted ones): no rounding at 1e-9 can change a count.  (Of the seeds 0 .. 7, seed 0 gives p = 0.025 and
    seed 7 p = 0.095 on the exact draws, the other six 0.22 .. 1.)"""
    for wide in (False, True):
        exact, shifted = _boot_ref(False, wide), _boot_ref(True, wide)
        gaps = [float(np.min(np.abs(r["null"] - r["v_stat"])) / r["v_stat"]) for r in (exact, shifted)]
        print(exact["p"], shifted["p"], gaps)
        assert exact["p"] >= 0.2 and shifted["p"] <= 0.02 and min(gaps) > 1e-9
    assert _boot_ref(False, False)["p"] == _boot_ref(False, True)["p"]
    assert _boot_ref(True, False)["p"] == _boot_ref(True, True)["p"]
    signs = _boot_signs()
    assert signs.shape == (BOOT_R, BOOT_S) and (np.abs(signs) == 1).all() and abs(signs.mean()) < 0.02


def _use_margins():
    K = ref.stein_matrix(*_use_inputs(), wide=False)["K"]
    sub = lambda idx: float(ref.ksd_stats(K[np.ix_(idx, idx)])["ksd"])
    return float(ref.thin(K, 30)[1][-1]), sub(np.arange(30)), sub(np.arange(0, 300, 10))


def test_thinning_is_useful_by_the_restatement():
    "USE_SEED = 0: the KSD of the 30 thinned samples is 0.133, of the first 30 0.917 and of every tenth 0.774"
    thinned, first, tenth = _use_margins()
    print(thinned, first, tenth)
    assert thinned < 0.5 * first and thinned < 0.5 * tenth


def test_the_recorded_deviations_are_the_measured_ones():
    got = _measure()
    print(got)
    for key, recorded in (("K", K_DEVIATION), ("r2", R2_DEVIATION), ("v_stat", V_DEVIATION), ("u_stat", U_DEVIATION),
                          ("row_mean", ROW_DEVIATION), ("ksd_path", PATH_DEVIATION), ("null", NULL_DEVIATION)):
        assert got[key] <= recorded <= max(2 * got[key], 2.0 ** -52 * 1.01), (key, got[key], recorded)
    for name in CASES:                                             # the integer outcomes do not depend on the precision
        a, b = _ref(name, False), _ref(name, True)
        assert a["nonfinite"] == b["nonfinite"] == (2 if CASES[name][5] == "bad" else 0) and a["d"] == b["d"]
        assert np.array_equal(a["indices"], b["indices"]), name
    wide = _ref("duplicates", True)
    assert wide["r2"][3, 7] == 0 and wide["K"][3, 7] == wide["K"][3, 3]
    # what the anchor is for: the uncentred Gram form loses the far case by orders of magnitude
    x, g = (a.astype(np.float64) for a in _inputs("far"))
    A = x @ x.T
    r2 = np.diag(A)[:, None] + np.diag(A)[None, :] - 2 * A
    s = _ref("far", True)["r2"].mean(axis=1)
    assert np.max(np.abs(r2 - _ref("far", True)["r2"]) / np.sqrt(np.outer(s, s))) > 1e4 * R2_DEVIATION


# ------------------------------------------------------------------------------------------------------------------ GPU

def _bound(recorded):
    return 4 * max(recorded, 2.0 ** -53)        # a measured 0 leaves 4 roundings of the quantity: 2^-51


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _kwargs(name):
    _, _, _, beta, c, _, ws = CASES[name]
    return dict(c=c, beta=beta, **({} if ws is None else dict(workspace_bytes=ws)))


def _same_bits(a, b):
    return all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b) if isinstance(p, torch.Tensor))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_against_the_restatement(name):
    from bnn_priors_amd import stein
    assert (stein.TILE, stein.CHUNK) == (TILE, KC)
    S, D, dtype, beta, c, special, _ = CASES[name]
    x, g = (_dev(a) for a in _inputs(name))
    k = stein.kernel_matrix(x, g, **_kwargs(name))
    stats, thinned = stein.ksd(k), stein.thin(k, _picks(name))
    again = stein.kernel_matrix(x, g, **_kwargs(name))
    assert _same_bits(k, again) and _same_bits(stats, stein.ksd(again)) and _same_bits(thinned, stein.thin(again, _picks(name)))
    wide = _ref(name, True)
    assert k.K.shape == k.r2.shape == (S, S) and k.K.dtype == torch.float64 and (k.d, k.beta) == (D, beta) == (wide["d"], beta)
    assert int(k.nonfinite) == wide["nonfinite"] and stats.row_mean.shape == (S,) and thinned.indices.dtype == torch.int64
    got = dict(K=k.K.cpu().numpy(), r2=k.r2.cpu().numpy(), v_stat=float(stats.v_stat), u_stat=float(stats.u_stat),
               row_mean=stats.row_mean.cpu().numpy(), ksd_path=thinned.ksd_path.cpu().numpy())
    if wide["nonfinite"]:
        assert all(np.isnan(got[q]).all() for q in QUANTITIES) and np.isnan(float(stats.ksd))
        assert thinned.indices.tolist() == [0] * _picks(name)
        return
    assert np.array_equal(got["K"], got["K"].T) and np.array_equal(got["r2"], got["r2"].T) and (np.diag(got["r2"]) == 0).all()
    assert abs(float(stats.ksd) - np.sqrt(got["v_stat"])) <= 2.0 ** -52 * float(stats.ksd)
    assert np.array_equal(thinned.indices.cpu().numpy(), wide["indices"])
    if c == "median":
        assert float(k.c) ** 2 == pytest.approx(float(wide["c2"]), rel=1e-12)
        assert float(k.c) ** 2 == pytest.approx(float(np.sort(got["r2"][np.triu_indices(S, 1)])[(S * (S - 1) // 2 - 1) // 2]),
                                                rel=1e-15)
    else:
        assert k.c == c
    if special == "dup":
        assert got["r2"][3, 7] == 0 and got["r2"][3, 6] > 0
        scale = np.sqrt(got["K"][3, 3] * got["K"][7, 7])
        assert abs(got["K"][3, 7] - got["K"][3, 3]) <= _bound(K_DEVIATION) * scale
    dev = _deviations(got, wide)
    print(name, dev)
    assert dev["K"] <= _bound(K_DEVIATION) and dev["r2"] <= _bound(R2_DEVIATION)
    assert dev["v_stat"] <= _bound(V_DEVIATION) and dev["u_stat"] <= _bound(U_DEVIATION)
    assert dev["row_mean"] <= _bound(ROW_DEVIATION) and dev["ksd_path"] <= _bound(PATH_DEVIATION)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_a_row_strided_view_gives_the_bits_of_its_contiguous_copy(dtype):
    from bnn_priors_amd import stein
    rng = np.random.default_rng(31)
    S, D = 33, 2 * KC + 3
    longer = _dev(rng.standard_normal((2 * S, D + 9)).astype(dtype))
    scores = _dev(rng.standard_normal((2 * S, D + 9)).astype(dtype))
    x, g = longer[::2, 4:4 + D], scores[1::2, 2:2 + D]      # every second sample of a longer stack, a column slice of a wider
    assert not x.is_contiguous() and x.stride() == (2 * (D + 9), 1) and g.storage_offset() == D + 9 + 2
    a = stein.kernel_matrix(x, g, c="median", beta=-0.3)
    b = stein.kernel_matrix(x.contiguous(), g.contiguous(), c="median", beta=-0.3)
    assert _same_bits(a, b)
    wide = ref.stein_matrix(x.cpu().numpy(), g.cpu().numpy(), c="median", beta=-0.3, wide=True)
    dk = np.sqrt(np.diag(wide["K"]))
    assert np.max(np.abs(LD(1) * a.K.cpu().numpy() - wide["K"]) / np.outer(dk, dk)) <= _bound(K_DEVIATION)


@pytest.mark.gpu
def test_a_dict_of_three_tensors_gives_the_gram_calls_added_in_key_order():
    from bnn_priors_amd import stein
    rng = np.random.default_rng(32)
    S = 17
    shapes = {"b.weight": (6, 5), "a.bias": (7,), "c.filter": (2, 3, 3, 3)}
    x = {k: _dev(rng.standard_normal((S, *s)).astype(np.float32)) for k, s in shapes.items()}
    g = {k: _dev(rng.standard_normal((S, *s)).astype(np.float32)) for k, s in shapes.items()}
    x["c.filter"] = _dev(rng.standard_normal((2 * S, 2, 3, 3, 3)).astype(np.float32))[::2]        # a view stays a view
    k = stein.kernel_matrix(x, g, c=1.5, beta=-0.3)
    gram = bad = None
    for name in sorted(shapes):
        g1, b1 = stein._gram(x[name].reshape(S, -1), g[name].reshape(S, -1))
        gram, bad = (g1, b1) if gram is None else (gram + g1, bad + b1)
    d = sum(int(np.prod(s)) for s in shapes.values())
    K, r2 = stein._finish(gram, bad, d, 1.5 * 1.5, -0.3)
    assert k.d == d == 91 and torch.equal(_bits(k.K), _bits(K)) and torch.equal(_bits(k.r2), _bits(r2))
    to_np = lambda t: {n: v.cpu().numpy() for n, v in t.items()}
    wide = ref.stein_matrix(to_np(x), to_np(g), c=1.5, beta=-0.3, wide=True)
    dk = np.sqrt(np.diag(wide["K"]))
    assert np.max(np.abs(LD(1) * k.K.cpu().numpy() - wide["K"]) / np.outer(dk, dk)) <= _bound(K_DEVIATION)
    flat = stein.kernel_matrix(torch.cat([x[n].reshape(S, -1) for n in sorted(shapes)], 1),
                               torch.cat([g[n].reshape(S, -1) for n in sorted(shapes)], 1), c=1.5, beta=-0.3)
    assert np.max(np.abs(flat.K.cpu().numpy() - k.K.cpu().numpy()) / np.outer(dk, dk)) <= 2 * _bound(K_DEVIATION)


@pytest.mark.gpu
def test_a_batch_of_three_weight_vectors_gives_the_bits_of_three_single_calls():
    from bnn_priors_amd import stein
    name = "s65_three_splits"
    k = stein.kernel_matrix(*(_dev(a) for a in _inputs(name)), **_kwargs(name))
    S = CASES[name][0]
    W = _dev(np.random.default_rng(33).standard_normal((3, S)))
    batch = stein.quadratic_forms(k, W)
    singles = torch.stack([stein.quadratic_forms(k, W[r]) for r in range(3)])
    assert batch.shape == (3,) and torch.equal(_bits(batch), _bits(singles))
    assert torch.equal(_bits(stein.quadratic_forms(k.K, W[1:2])), _bits(batch[1:2]))        # a bare K
    want = ref.quadratic_forms(_ref(name, True)["K"], W.cpu().numpy())
    scale = (np.abs(W.cpu().numpy()) @ np.sqrt(np.diag(_ref(name, True)["K"]))) ** 2 / S ** 2
    assert np.max(np.abs(LD(1) * batch.cpu().numpy() - want) / scale) <= _bound(K_DEVIATION)
    ones = torch.ones(S, dtype=torch.float64, device="cuda")
    v = stein.ksd(k).v_stat
    assert torch.equal(_bits(stein.quadratic_forms(k, ones)), _bits(v))                       # W = 1 is v_stat, bit for bit
    assert torch.equal(_bits(stein.quadratic_forms(k, -ones.reshape(1, S))[0]), _bits(v))


@pytest.mark.gpu
@pytest.mark.parametrize("S", (2, 65, 300))
def test_thinning_of_an_integer_valued_matrix_is_exact(S):
    from bnn_priors_amd import stein
    K = _integer_K(S)
    for m in (S - 1 if S > 2 else 1, S, S + 7):
        want_idx, want_path = ref.thin(K, m)
        if S <= 65:
            picks, path = _brute_force_thinning(K, m)
            assert picks == want_idx.tolist() and np.array_equal(np.array(path), want_path)
        got = stein.thin(_dev(K), m)
        assert got.indices.tolist() == want_idx.tolist()
        path = got.ksd_path.cpu().numpy()
        assert np.max(np.abs(path - want_path) / want_path) <= 2.0 ** -51          # (a square root and a division)
        sums = np.cumsum([2 * K[want_idx[:a], p].sum() + K[p, p] for a, p in enumerate(want_idx)])   # integers
        assert np.array_equal(np.rint((path * np.arange(1, m + 1)) ** 2), sums)
    assert len(set(want_idx.tolist())) < m                       # m > S: picks repeat
    flat = np.full((S, S), 1.0) + 2 * np.eye(S)                  # all equal: the smaller index, round after round
    assert stein.thin(_dev(flat), S + 1).indices.tolist() == list(range(S)) + [0]


@pytest.mark.gpu
@pytest.mark.parametrize("shifted", (False, True))
def test_wild_bootstrap_with_given_signs_against_the_restatement(shifted):
    """The measured gaps between the observed statistic and the nearest null value are 8.7e-4 (exact draws) and 0.84
    (shifted) of the observed one, the bound on a null value 2.1e-15 of it: no rounding can change a count."""
    from bnn_priors_amd import stein
    x, g = (_dev(a) for a in _boot_inputs(shifted))
    k = stein.kernel_matrix(x, g)
    t = stein.wild_bootstrap_test(k, signs=_dev(_boot_signs()))
    wide = _boot_ref(shifted, True)
    assert t.null.shape == (BOOT_R,) and float(t.p) == wide["p"] and (wide["p"] >= 0.2, wide["p"] <= 0.02)[shifted]
    assert torch.equal(_bits(t.v_stat), _bits(stein.ksd(k).v_stat))
    assert abs(LD(1) * float(t.v_stat) - wide["v_stat"]) / wide["v_stat"] <= _bound(V_DEVIATION)
    assert np.max(np.abs(LD(1) * t.null.cpu().numpy() - wide["null"])) / wide["v_stat"] <= _bound(NULL_DEVIATION)
    assert float(np.min(np.abs(wide["null"] - wide["v_stat"])) / wide["v_stat"]) > 1e-9


@pytest.mark.gpu
def test_wild_bootstrap_by_seed():
    from bnn_priors_amd import stein
    k = stein.kernel_matrix(*(_dev(a) for a in _boot_inputs(False)))
    a = stein.wild_bootstrap_test(k, replicates=BOOT_R, seed=3)
    b = stein.wild_bootstrap_test(k, replicates=BOOT_R, seed=3)
    assert _same_bits(a, b) and a.null.shape == (BOOT_R,) and 0 < float(a.p) <= 1
    assert not torch.equal(_bits(a.null), _bits(stein.wild_bootstrap_test(k, replicates=BOOT_R, seed=4).null))
    # independent signs: E Q_r = trace(K) / S^2
    assert abs(float(a.null.mean()) / float(torch.diagonal(k.K).sum() / BOOT_S ** 2) - 1) < 0.2
    slow = stein.wild_bootstrap_test(k, replicates=BOOT_R, flip_prob=0.02, seed=3)           # long runs of equal signs
    assert torch.isfinite(slow.null).all() and not torch.equal(_bits(a.null), _bits(slow.null))
    shifted = stein.kernel_matrix(*(_dev(a) for a in _boot_inputs(True)))
    assert float(stein.wild_bootstrap_test(shifted, replicates=BOOT_R, seed=3).p) == 1 / (BOOT_R + 1)


@pytest.mark.gpu
def test_thinning_is_useful():
    """S = 300 draws of which a third are shifted (USE_SEED = 0): by the restatement the KSD of the 30 thinned samples is
    0.133, that of the first 30 is 0.917 and that of every tenth 0.774; it keeps none of the shifted third."""
    from bnn_priors_amd import stein
    k = stein.kernel_matrix(*(_dev(a) for a in _use_inputs()))
    thinned = stein.thin(k, 30)
    first = stein.ksd(k.K[:30, :30]).ksd
    tenth = stein.ksd(k.K[::10, ::10]).ksd
    want = _use_margins()
    print(float(thinned.ksd_path[-1]), float(first), float(tenth), want)
    assert float(thinned.ksd_path[-1]) < float(first) and float(thinned.ksd_path[-1]) < float(tenth)
    for got, ref_value in zip((thinned.ksd_path[-1], first, tenth), want):
        assert float(got) == pytest.approx(ref_value, rel=1e-9)
    kept = thinned.indices.cpu().numpy()
    assert (kept % 3 == 0).mean() < 0.2                          # it keeps few of the shifted third
    sub = stein.ksd(k.K[thinned.indices][:, thinned.indices]).ksd
    assert float(sub) == pytest.approx(float(thinned.ksd_path[-1]), rel=1e-12)


@pytest.mark.gpu
def test_evaluate_stein_equals_the_separate_calls():
    from bnn_priors_amd import evaluation, stein
    from bnn_priors_amd.models import GaussianModel
    model = GaussianModel(2, 3, 0.5, 1.5)
    gen = torch.Generator().manual_seed(5)
    samples = {"0.p": 0.5 + 1.5 * torch.randn(40, 3, generator=gen), "1.p": 0.5 + 1.5 * torch.randn(40, 3, generator=gen)}
    out = evaluation.evaluate_stein(model, samples, None, None, temperature=1.0, thin_to=7, c=2.0, beta=-0.3)
    score = stein.scores(model, samples)
    k = stein.kernel_matrix({n: v.cuda() for n, v in samples.items()}, {n: v.cuda() for n, v in score.items()}, c=2.0,
                            beta=-0.3)
    stats, thinned = stein.ksd(k), stein.thin(k, 7)
    assert out == {"ksd": float(stats.ksd), "v_stat": float(stats.v_stat), "u_stat": float(stats.u_stat), "dimension": 6,
                   "nonfinite": 0, "kept": thinned.indices.tolist(), "ksd_thinned": float(thinned.ksd_path[-1])}
    assert all(type(out[q]) is float for q in ("ksd", "v_stat", "u_stat", "ksd_thinned")) and len(out["kept"]) == 7
    plain = evaluation.evaluate_stein(model, samples, None, None)
    assert sorted(plain) == ["dimension", "ksd", "nonfinite", "u_stat", "v_stat"]
    # the samples are draws of the target: a run at the wrong scale is further from it
    # (by the restatement 0.679 against 0.457)
    wide_samples = {n: 0.5 + 2 * (v - 0.5) for n, v in samples.items()}
    wrong = evaluation.evaluate_stein(model, wide_samples, None, None)
    assert wrong["ksd"] > plain["ksd"]
    for got, smp in ((plain, samples), (wrong, wide_samples)):
        x = {n: v.numpy() for n, v in smp.items()}
        want = ref.ksd_stats(ref.stein_matrix(x, {n: v.numpy() for n, v in stein.scores(model, smp).items()}, wide=True)["K"])
        assert got["ksd"] == pytest.approx(float(want["ksd"]), rel=1e-9)


@pytest.mark.gpu
def test_the_gram_walk_reproduces_the_recorded_bits():
    """sha256 of K, r2 and nonfinite of ``kernel_matrix`` and of the thinning order of 5 picks, for every case of
    tests/golden/make_gram_bits.py, against tests/golden/gram_bits.json -- recorded with the library of the commit before
    the two Gram passes came to share csrc/gram_hip.inc.  The library is built with -ffp-contract=off: the same operations
    in the same order are the same bits."""
    import importlib.util
    import json
    import os
    spec = importlib.util.spec_from_file_location(
        "make_gram_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_gram_bits.py"))
    bits = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bits)
    with open(bits.PATH) as fh:
        recorded = json.load(fh)
    assert len(recorded["parent_commit"]) == 40 and len(recorded["library_sha"]) == 16
    want, got = recorded["stein"], bits.stein_digests()
    assert sorted(got) == sorted(want) == sorted(bits.stein_cases())
    for name in sorted(got):
        assert sorted(got[name]) == sorted(want[name]) == ["K", "nonfinite", "r2", "thin"]
        for array in got[name]:
            assert got[name][array] == want[name][array], (
                f"case {name}: {array} differs from the recording (recorded under {recorded['versions']}, running "
                f"{bits.versions()})")
