"""Calibration and out-of-distribution metrics on the device (bnn_priors_amd/calibration.py, csrc/calib_hip.inc;
reference: bnn_priors/third_party/calibration_error.py, exp_utils.py:323-327,343-380).

A numpy restatement of the kernels' arithmetic -- sorted columns, bins as contiguous ranges of them, integer counts --
(tests/calibration_reference.py) is pinned to the goldens the reference's own code produced
(tests/golden/make_calibration_goldens.py) and to its own statement in exact rationals on the CPU; the GPU tests hold
the kernels to the goldens and to the rationals at every geometry where a kernel takes another path (the grids below),
calling the C ABI directly with sentinel-filled, over-allocated outputs so that a skipped write or a write past the end
shows; and the model-level evaluation to the restatement applied to its own predictive tables."""
import math
import os
import re
import time
from fractions import Fraction

import numpy as np
import pytest
import torch

from bnn_priors_amd import _hip
from bnn_priors_amd import calibration as cal
from bnn_priors_amd import evaluation as ev
from calibration_reference import (EPS, exact_auroc_auprc, exact_gce, exact_metrics, mann_whitney_auroc,  # noqa: F401
                                   np_ensemble_probs, np_gce, np_metrics)     # (re-exported: test_uncertainty imports)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "calibration.npz")
HEADER = os.path.join(os.path.dirname(HERE), "include", "sgmcmc_hip.h")
INVALID_VALUE = 1           # hipErrorInvalidValue
TINY = np.finfo(np.float64).tiny


def _golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _cases(prefix):
    g = _golden()
    return sorted({k.split("__")[1] for k in g if k.startswith(prefix + "__")})


def _bins(g, case):
    "(num_bins, datapoints_per_bin) of a calibration golden: the reference's defaults where the case carries none"
    return int(g.get(f"cal__{case}__num_bins", 30)), int(g.get(f"cal__{case}__dpb", 100))


# ---- the grids (shared by the CPU checks of the references and the GPU tests) ------------------------------------------

# ensemble_kernel: 256 // C rows per block, four samples per rescale.  Every (C, N) below runs with two values of E;
# E walks its axis diagonally, so every E meets at least two C and two N, every C five or more E, every N position all E.
ENS_E = (1, 2, 3, 4, 5, 7, 8, 9)
ENS_C = (1, 2, 3, 7, 85, 86, 127, 128)          # 256, 128, 85, 36, 3, 2, 2, 2 rows per block


def _ens_rows(C):
    rows = 256 // C
    return [n for n in dict.fromkeys((1, rows - 1, rows, rows + 1, 2 * rows + 1)) if n >= 1]


ENS_GRID = [(ENS_E[(i + j + d) % len(ENS_E)], N, C)
            for i, C in enumerate(ENS_C) for j, N in enumerate(_ens_rows(C)) for d in (0, 3)]

ORDER_N = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049)      # the 256-key LDS tile, the 1024 keys of a block
ORDER_KINDS = ("continuous", "all_equal", "grid8", "sorted", "reversed", "zeros", "two_nans")

CALIB_N = (1, 2, 63, 64, 65, 257)                               # the 64 lanes of a bin's wave, a second pass over them
CALIB_BINS = (0, 1, 2, 3, 30, 255, 256, 257, 4096)              # 0: adaptive only; the 256 threads of the bound loop
CALIB_SCHEMES = (("even", False), ("adaptive", False), ("adaptive", True))      # (binning, l2)
CALIB_KINDS = ("continuous", "all_equal", "nonpositive", "one_positive", "on_bounds", "grid8")
CALIB_C = (2, 7, 128)

RANK_N = (2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4097)    # L = ceil(n / 1024) keys per thread: 1, 2, 3, 5
RANK_KINDS = ("continuous", "quantised", "all_equal", "mixed", "long_run", "separable_up", "separable_down", "zeros")


def _rank_P(n):
    return sorted({1, n - 1, n // 2})


def _order_keys(kind, n, rng):
    if kind == "continuous":
        return rng.normal(size=n)
    if kind == "all_equal":
        return np.full(n, 0.375)
    if kind == "grid8":
        return rng.integers(0, 9, n) / 8.0
    if kind == "sorted":
        return np.sort(rng.normal(size=n))
    if kind == "reversed":
        return np.sort(rng.normal(size=n))[::-1].copy()
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324, TINY / 3, TINY, -TINY, 1.0]), n)
    assert kind == "two_nans"
    a = rng.normal(size=n)
    a[rng.choice(n, min(2, n), replace=False)] = np.nan
    return a


def _calib_keys(kind, n, num_bins, rng):
    if kind == "continuous":
        return 1.0 - rng.random(n)                              # (0, 1]
    if kind == "all_equal":
        return np.full(n, 0.375)
    if kind in ("nonpositive", "one_positive"):
        a = rng.choice(np.array([0.0, -0.0, -0.25, -1.0]), n)
        if kind == "one_positive":
            a[rng.integers(n)] = 0.625
        return a
    if kind == "on_bounds":
        return rng.choice(np.histogram_bin_edges([], bins=num_bins or 30, range=(0.0, 1.0))[1:], n)
    assert kind == "grid8"
    return rng.integers(0, 9, n) / 8.0                          # 0 is filtered, 1 falls in the extra even bin


def _rank_scores(kind, n, P, rng):
    "n scores, the first P the positives"
    if kind in ("separable_up", "separable_down"):
        v = np.sort(rng.random(n))
        assert (np.diff(v) > 0).all()
        pos, neg = (v[n - P:], v[:n - P]) if kind == "separable_up" else (v[:P], v[P:])
        return np.concatenate([rng.permutation(pos), rng.permutation(neg)])
    if kind == "continuous":
        return rng.normal(size=n)
    if kind == "quantised":
        return np.round(rng.beta(3, 2, n) * 64) / 64
    if kind == "all_equal":
        return np.full(n, 0.5)
    if kind == "mixed":
        s = rng.random(n)
        s[n // 2:] = np.round(s[n // 2:] * 16) / 16
        return rng.permutation(s)
    if kind == "long_run":
        s = rng.random(n)
        s[:n // 2] = 0.5
        return rng.permutation(s)
    assert kind == "zeros"
    return rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324, TINY, -TINY, 1.0]), n)


def _bounds(scheme, num_bins):
    return np.histogram_bin_edges([], bins=num_bins, range=(0.0, 1.0))[1:] if scheme == "even" else None


# ---- CPU: the restatement against the reference's numbers, argument checks ------------------------------------------

@pytest.mark.parametrize("case", _cases("cal"))
def test_restatement_reproduces_the_reference_calibration_goldens(case):
    g = _golden()
    num_bins, dpb = _bins(g, case)
    got = np_metrics(g[f"cal__{case}__labels"], g[f"cal__{case}__probs"], num_bins, dpb)
    for k in ("ece", "ace", "rmsce"):
        assert abs(got[k] - float(g[f"cal__{case}__{k}"])) <= 1e-15, (k, got[k], float(g[f"cal__{case}__{k}"]))
    exact = exact_metrics(g[f"cal__{case}__labels"], g[f"cal__{case}__probs"], num_bins, dpb)
    assert abs(got["ece"] - float(exact["ece"])) <= 1e-13 and abs(got["ace"] - float(exact["ace"])) <= 1e-13
    assert abs(got["rmsce"] ** 2 - float(exact["rmsce2"])) <= 1e-13


@pytest.mark.parametrize("case", _cases("ood"))
def test_restatement_reproduces_the_reference_ood_goldens(case):
    g = _golden()
    s_in, s_out = g[f"ood__{case}__in"], g[f"ood__{case}__out"]
    auroc, ap = exact_auroc_auprc(s_in, s_out)
    assert abs(float(auroc) - float(g[f"ood__{case}__auroc"])) <= 1e-15
    assert abs(ap - float(g[f"ood__{case}__auprc"])) <= 1e-15
    assert mann_whitney_auroc(s_in, s_out) == auroc                 # two algorithms, one rational


@pytest.mark.parametrize("n", CALIB_N)
def test_exact_gce_and_np_gce_agree_on_the_grid(n):
    "the fp64 restatement is within 1e-13 of the rationals on every input of the device grid"
    rng = np.random.default_rng(100 + n)
    worst = 0.0
    for num_bins in CALIB_BINS:
        for scheme, l2 in CALIB_SCHEMES:
            if scheme == "even" and num_bins == 0:
                continue
            for kind in CALIB_KINDS:
                keys, hits = _calib_keys(kind, n, num_bins, rng), rng.integers(0, 2, n)
                args = dict(bounds=_bounds(scheme, num_bins), num_bins=num_bins, l2=l2)
                dev = abs(np_gce(keys, hits, **args) - float(exact_gce(keys, hits, **args)))
                assert dev <= 1e-13, (n, num_bins, scheme, l2, kind, dev)
                worst = max(worst, dev)
    print(f"np_gce against exact_gce at n = {n}: max deviation {worst:.3g}")


def test_exact_gce_is_the_definition_on_a_case_small_enough_to_do_by_hand():
    # keys 1/4, 1/2, 1/2, 3/4 (and a dropped 0), hits 0 1 0 1; two adaptive bins: step 2, bound = sorted[2] = 1/2,
    # np.digitize: [1/4] and [1/2, 1/2, 3/4] -> |0 - 1/4| / 4 + |2 - 7/4| / 4 = 1/8 up to the eps in the weights
    keys, hits = np.array([0.5, 0.0, 0.25, 0.75, 0.5]), np.array([1, 1, 0, 1, 0])
    got = exact_gce(keys, hits, num_bins=2)
    assert got == Fraction(1, 8) and abs(np_gce(keys, hits, num_bins=2) - 0.125) <= 1e-15
    assert exact_gce(keys, hits, num_bins=2, l2=True) == Fraction(1, 256) + Fraction(1, 256)
    # even bounds 1/2, 1: [1/4], [1/2, 1/2, 3/4], [] -> the same two bins
    assert exact_gce(keys, hits, bounds=np.array([0.5, 1.0])) == Fraction(1, 8)


def test_golden_cases_cover_the_corner_cases():
    g = _golden()
    assert len(g["cal__small80__labels"]) < 100                                   # rmsce: one bin
    p = g["cal__onehot__probs"]
    assert (p.max(1) == 1.0).all() and ((p == 0) | (p == 1)).all()                # `> 0` filter, bin 30
    on_bound = np.isin(g["cal__edges__probs"].max(1), np.histogram_bin_edges([], 30, (0, 1)))
    assert on_bound.all()
    assert g["cal__binary__probs"].shape[1] == 2
    assert len(np.unique(np.concatenate([g["ood__quantised__in"], g["ood__quantised__out"]]))) <= 65
    assert len(g["ood__single_pos__in"]) == 1
    assert os.path.getsize(GOLDEN) <= 600 * 1024
    # ---- the geometry cases: each reaches the edge it is named for
    shape = {c: g[f"cal__{c}__probs"].shape + _bins(g, c) for c in _cases("cal")}
    p = g["cal__few_rows__probs"]
    assert shape["few_rows"] == (15, 3, 30, 100) and (p > 0).all() and 15 / 30 == 0.5      # step 1/2 in every column,
    idx = np.rint(np.arange(1, 30) * 0.5)                                                   # half-integers to even,
    assert (idx[::2] != np.floor(0.5 + np.arange(1, 30) * 0.5)[::2]).any() and idx.max() == 14   # 14.5 -> 14 = m - 1
    assert shape["one_bin"] == (200, 10, 1, 100) and shape["two_bins"] == (200, 10, 2, 50)
    assert shape["max_bins"] == (333, 5, cal.MAX_BINS, 100)
    assert shape["dpb7"] == (1000, 3, 100, 7) and int(1000 / 7) == 142
    assert shape["wide"] == (64, cal.MAX_CLASSES, 30, 100)
    p = g["cal__grid8__probs"]
    assert shape["grid8"] == (45, 4, 30, 3) and (p * 8 == np.rint(p * 8)).all()
    for col in (p.max(1), p[:, 0]):                      # an adaptive bound repeats: the bins between are empty
        s = np.sort(col[col > 0])
        nb = 15 if col is not p[:, 0] else 30
        b = s[np.minimum(np.rint(np.arange(1, nb) * (len(s) / nb)), len(s) - 1).astype(int)]
        assert len(np.unique(b)) < len(b)
    assert shape["single_column"] == (50, 1, 30, 100) and set(g["cal__single_column__labels"].tolist()) == {0, 1}
    p = g["cal__dead_column__probs"]
    assert shape["dead_column"] == (120, 4, 30, 100) and (p[:, 2] == 0).all() and (p[:, 3] > 0).sum() == 1
    n_p = {c: (len(g[f"ood__{c}__in"]), len(g[f"ood__{c}__out"])) for c in _cases("ood")}
    assert n_p["pair"] == (1, 1) and n_p["ties3"] == (2, 1)
    assert len(np.unique(np.r_[g["ood__ties3__in"], g["ood__ties3__out"]])) == 1
    assert [sum(n_p[f"n{n}"]) for n in (1023, 1024, 1025, 2047, 2049)] == [1023, 1024, 1025, 2047, 2049]
    assert n_p["n1024"][0] == 1 and n_p["n1025"][1] == 1 and n_p["n2047"][1] == 1 and n_p["n1023"][0] == 1023 // 2
    both = np.r_[g["ood__long_run__in"], g["ood__long_run__out"]]
    assert len(both) == 2049 and (both == 0.5).sum() == 1024 and 0 < (g["ood__long_run__in"] == 0.5).sum() < 1024
    assert g["ood__separable_up__in"].min() > g["ood__separable_up__out"].max()
    assert float(g["ood__separable_up__auroc"]) == 1.0
    assert g["ood__separable_down__in"].max() < g["ood__separable_down__out"].min()
    assert float(g["ood__separable_down__auroc"]) == 0.0
    z = np.r_[g["ood__zeros__in"], g["ood__zeros__out"]]
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all() and (np.abs(z) == 5e-324).any()


def test_the_grids_cover_their_axes():
    assert {E for E, _, _ in ENS_GRID} == set(ENS_E) and {C for _, _, C in ENS_GRID} == set(ENS_C)
    assert [256 // C for C in ENS_C] == [256, 128, 85, 36, 3, 2, 2, 2]
    for E in ENS_E:
        assert len({C for e, _, C in ENS_GRID if e == E}) >= 2 and len({N for e, N, _ in ENS_GRID if e == E}) >= 2
    for C in ENS_C:
        assert len({E for E, _, c in ENS_GRID if c == C}) >= 2 and len({N for _, N, c in ENS_GRID if c == C}) >= 2
        assert {N for _, N, c in ENS_GRID if c == C} == set(_ens_rows(C))
    assert {(n + 1023) // 1024 for n in RANK_N} == {1, 2, 3, 5}


def test_limits_match_the_header():
    with open(HEADER) as f:
        limits = dict(re.findall(r"#define SGMCMC_CALIB_MAX_(\w+) (\d+)", f.read()))
    assert {k: int(v) for k, v in limits.items()} == {"CLASSES": cal.MAX_CLASSES, "ROWS": cal.MAX_ROWS,
                                                      "BINS": cal.MAX_BINS}


def test_wrappers_reject_bad_arguments_before_any_launch():
    y = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="classes"):
        cal.ece(y, torch.full((8, 129), 1 / 129))
    with pytest.raises(ValueError, match="classes"):
        cal.ensemble_probs(torch.zeros(2, 8, 129))
    with pytest.raises(ValueError, match="rows"):
        cal.ace(torch.zeros(cal.MAX_ROWS + 1, dtype=torch.int64), torch.zeros(cal.MAX_ROWS + 1, 10))
    with pytest.raises(ValueError, match="at most"):
        cal.auroc_auprc(torch.zeros(cal.MAX_ROWS), torch.zeros(1))
    with pytest.raises(ValueError, match="Only one class"):
        cal.auroc_auprc(torch.zeros(0), torch.zeros(5))
    for call in (lambda: cal.ece(y, torch.full((8, 10), 0.1)), lambda: cal.rmsce(y, torch.full((8, 10), 0.1)),
                 lambda: cal.ensemble_probs(torch.zeros(2, 8, 10)), lambda: cal.auroc_auprc(torch.zeros(3), torch.zeros(4))):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="num_bins"):
        cal.ece(y, torch.full((8, 10), 0.1), num_bins=cal.MAX_BINS + 1)


# ---- GPU --------------------------------------------------------------------------------------------------------------

def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases("cal"))
def test_calibration_kernels_match_the_reference_goldens(case):
    g = _golden()
    y, p = _dev(g[f"cal__{case}__labels"]), _dev(g[f"cal__{case}__probs"])
    num_bins, dpb = _bins(g, case)
    got = cal.calibration_metrics(y, p, num_bins=num_bins, datapoints_per_bin=dpb)
    for k in ("ece", "ace", "rmsce"):
        assert abs(got[k] - float(g[f"cal__{case}__{k}"])) <= 1e-12, (k, got[k], float(g[f"cal__{case}__{k}"]))
    assert cal.ece(y, p, num_bins) == got["ece"] and cal.ace(y, p, num_bins) == got["ace"]
    assert cal.rmsce(y, p, num_bins, dpb) == got["rmsce"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases("ood"))
def test_rank_kernel_matches_the_goldens_and_the_exact_rational(case):
    g = _golden()
    s_in, s_out = g[f"ood__{case}__in"], g[f"ood__{case}__out"]
    auroc, auprc = cal.auroc_auprc(_dev(s_in), _dev(s_out))
    assert abs(auroc - float(g[f"ood__{case}__auroc"])) <= 1e-12
    assert abs(auprc - float(g[f"ood__{case}__auprc"])) <= 1e-12
    exact, _ = exact_auroc_auprc(s_in, s_out)
    assert auroc == float(exact)                      # integer trapezoids, one correctly rounded division
    assert auroc == float(mann_whitney_auroc(s_in, s_out))        # ... and the pair count, which has no trapezoids


@pytest.mark.gpu
def test_ordering_kernel_is_numpy_stable_argsort():
    rng = np.random.default_rng(3)
    tiny = np.finfo(np.float64).tiny
    special = np.array([0.0, -0.0, 5e-324, -5e-324, tiny / 3, tiny, -tiny, 1.0, -1.0, np.inf, -np.inf, 1e308, 0.5])
    cols = [np.r_[special, rng.choice(special, 3000), rng.normal(size=1200)],       # ties, signed zeros, subnormals
            np.round(rng.random(4321) * 8) / 8,                                      # heavy ties
            rng.random(1)]
    for a in cols:
        got = cal._order(_dev(a), len(a), 1, 1, 0).cpu().numpy()[0]
        assert np.array_equal(got, np.argsort(a, kind="stable")), len(a)
    # strided columns of a row-major [N, C] matrix, as the class-conditional metric orders them
    m = np.round(rng.random((777, 7)) * 16) / 16
    got = cal._order(_dev(m), 777, 7, 7, 1).cpu().numpy()
    for j in range(7):
        assert np.array_equal(got[j], np.argsort(m[:, j], kind="stable"))
    a = np.r_[rng.random(50), np.nan, rng.random(50), np.nan]                     # NaN last, as numpy sorts it
    assert np.array_equal(cal._order(_dev(a), len(a), 1, 1, 0).cpu().numpy()[0], np.argsort(a, kind="stable"))


@pytest.mark.gpu
def test_ensemble_probs_match_the_categorical_of_the_log_mean():
    rng = np.random.default_rng(5)
    for E, N, C in ((7, 1001, 10), (1, 64, 128), (4, 33, 2), (300, 50, 3)):
        f = rng.normal(scale=3.0, size=(E, N, C))
        acc = f - np.log(np.exp(f).sum(-1, keepdims=True))
        y = rng.integers(0, C, N)
        ens = cal.ensemble_probs(_dev(acc), _dev(y))
        want = np_ensemble_probs(acc)
        np.testing.assert_allclose(ens.probs.cpu().numpy(), want, rtol=0, atol=1e-13)
        pred = ens.probs.cpu().numpy().argmax(1)
        assert np.array_equal(ens.pred.cpu().numpy(), pred)
        assert np.array_equal(ens.conf.cpu().numpy(), ens.probs.cpu().numpy()[np.arange(N), pred])
        assert np.array_equal(ens.hit.cpu().numpy(), (pred == y).astype(np.int64))
        assert cal.ensemble_probs(_dev(acc)).hit is None


@pytest.mark.gpu
def test_two_runs_give_identical_bits():
    g = _golden()
    rng = np.random.default_rng(9)
    acc = np.log(rng.dirichlet(np.full(10, 0.4), size=(20, 5000)))
    y = _dev(rng.integers(0, 10, 5000))
    runs = []
    for _ in range(2):
        ens = cal.ensemble_probs(_dev(acc), y)
        m = cal.calibration_metrics(y, ens.probs)
        r = cal.auroc_auprc(_dev(g["ood__continuous__in"]), _dev(g["ood__continuous__out"]))
        runs.append((ens.probs.cpu().numpy().tobytes(), ens.conf.cpu().numpy().tobytes(), m, r))
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_nan_probabilities_give_nan_and_nan_scores_raise():
    g = _golden()
    p = g["cal__dirichlet__probs"].copy()
    p[17] = np.nan
    got = cal.calibration_metrics(_dev(g["cal__dirichlet__labels"]), _dev(p))
    assert all(math.isnan(v) for v in got.values()), got
    s_in = g["ood__continuous__in"].copy()
    s_in[3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        cal.auroc_auprc(_dev(s_in), _dev(g["ood__continuous__out"]))


def _model_setup(name):
    from test_evaluation import _setup
    return _setup(name, n=320, device="cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["classificationdensenet", "classificationconvnet", "googleresnet"])
def test_evaluate_model_calibration_eval(name):
    net, loader, samples, _ = _model_setup(name)
    plain = ev.evaluate_model(net, loader, samples)
    got = ev.evaluate_model(net, loader, samples, calibration_eval=True)
    assert {k: got[k] for k in plain} == plain                 # the likelihood / accuracy keys keep their bits
    assert set(got) == set(plain) | {"ece", "ace", "rmsce"}
    _, acc, labels, _ = ev.predictive_tables(net, loader, samples)
    want = np_metrics(labels.cpu().numpy(), np_ensemble_probs(acc))
    for k in ("ece", "ace", "rmsce"):
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["classificationdensenet", "classificationconvnet", "googleresnet"])
def test_evaluate_ood_ignores_the_ood_labels(name):
    net, loader, samples, _ = _model_setup(name)
    x_in = loader.dataset.tensors[0]
    g = torch.Generator().manual_seed(2)
    x_out = torch.rand((200,) + tuple(x_in.shape[1:]), generator=g).to(x_in.device) * 2 - 0.5
    ood = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x_out, torch.full((200,), 17, device=x_in.device)),
                                      batch_size=32)
    got = ev.evaluate_ood(net, loader, ood, samples)
    E = ev._n_samples(samples)
    for k, v in samples.items():                                 # the model holds the last sample
        assert torch.equal(net.state_dict()[k], v[E - 1].to(net.state_dict()[k].device)), k
    acc_in, acc_out = ev.logit_tables(net, (loader, ood), samples)
    assert acc_out.shape == (E, 200, 10)
    auroc, ap = exact_auroc_auprc(np_ensemble_probs(acc_in).max(1), np_ensemble_probs(acc_out).max(1))
    assert abs(got["auroc"] - float(auroc)) <= 1e-12 and abs(got["auprc"] - ap) <= 1e-12
    # the reference's formula: mean over samples of float32 pred.probs, then the max
    p_in = torch.softmax(acc_in.float(), -1).cpu().numpy().mean(0).max(-1)
    p_out = torch.softmax(acc_out.float(), -1).cpu().numpy().mean(0).max(-1)
    auroc32, ap32 = exact_auroc_auprc(p_in, p_out)
    assert abs(got["auroc"] - float(auroc32)) <= 1e-3 and abs(got["auprc"] - ap32) <= 1e-3


@pytest.mark.gpu
def test_multichain_recipe():
    "ensemble_across_chains' lme fed back through ensemble_probs(lme.unsqueeze(0)) is the single-process ensemble"
    rng = np.random.default_rng(11)
    f = rng.normal(size=(6, 300, 10))
    acc = _dev(f - np.log(np.exp(f).sum(-1, keepdims=True)))
    lps = acc[..., 0]
    _, lme = ev.ensemble_across_chains(lps, acc)
    via_chains = cal.ensemble_probs(lme.unsqueeze(0)).probs.cpu().numpy()
    np.testing.assert_allclose(via_chains, cal.ensemble_probs(acc).probs.cpu().numpy(), rtol=0, atol=1e-13)


# ---- GPU: the C ABI at every geometry, outputs sentinel-filled and over-allocated -------------------------------------

GUARD = 64
NAN_SENTINEL = 0x7FF8_0000_0BAD_F00D        # a NaN (as int64 bits) that no arithmetic produces: a written NaN differs


def _sentinel(n, dtype):
    "n + GUARD elements of dtype, every one the sentinel (fp64: NAN_SENTINEL, integers: -1)"
    if dtype == torch.float64:
        return torch.full((n + GUARD,), NAN_SENTINEL, dtype=torch.int64, device="cuda:0").view(torch.float64)
    return torch.full((n + GUARD,), -1, dtype=dtype, device="cuda:0")


def _is_sentinel(buf):
    return buf.view(torch.int64) == NAN_SENTINEL if buf.dtype == torch.float64 else buf == -1


def _written(buf, n, what):
    "the first n elements of a _sentinel buffer, after asserting that all of them and nothing beyond were written"
    left = _is_sentinel(buf)
    assert bool(left[n:].all()), f"{what}: written beyond its {n} elements"
    assert not bool(left[:n].any()), f"{what}: {int(left[:n].sum())} of {n} elements never written"
    return buf[:n]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ensemble_direct(acc, labels=None):
    "sgmcmc_ensemble_probs on a numpy table -> numpy (probs, conf, pred, hit)"
    E, N, C = acc.shape
    a, y = _dev(acc), None if labels is None else _dev(labels, torch.int64)
    probs, conf = _sentinel(N * C, torch.float64), _sentinel(N, torch.float64)
    pred, hit = _sentinel(N, torch.int64), None if labels is None else _sentinel(N, torch.int64)
    assert _hip.lib().sgmcmc_ensemble_probs(a.data_ptr(), _ptr(y), E, N, C, probs.data_ptr(), conf.data_ptr(),
                                            pred.data_ptr(), _ptr(hit), _stream()) == 0
    torch.cuda.synchronize()
    return (_written(probs, N * C, "probs").view(N, C).cpu().numpy(), _written(conf, N, "conf").cpu().numpy(),
            _written(pred, N, "pred").cpu().numpy(), None if hit is None else _written(hit, N, "hit").cpu().numpy())


def _order_direct(keys, elem_stride, col_stride, n, ncols):
    "sgmcmc_stable_order on a device tensor -> device perm [ncols, n] (a view of a guarded buffer)"
    perm = _sentinel(ncols * n, torch.int32)
    assert _hip.lib().sgmcmc_stable_order(keys.data_ptr(), elem_stride, col_stride, n, ncols, perm.data_ptr(),
                                          _stream()) == 0
    torch.cuda.synchronize()
    return _written(perm, ncols * n, "perm").view(ncols, n)


def _calib_direct(keys, perm, target, class_conditional, n, ncols, elem_stride, col_stride, bounds, num_bins, l2):
    "sgmcmc_calibration_error -> (col_err [ncols] numpy, out float)"
    col_err, out = _sentinel(ncols, torch.float64), _sentinel(1, torch.float64)
    b = None if bounds is None else _dev(bounds)
    assert _hip.lib().sgmcmc_calibration_error(keys.data_ptr(), elem_stride, col_stride, perm.data_ptr(),
                                               target.data_ptr(), int(class_conditional), n, ncols, _ptr(b), num_bins,
                                               int(l2), col_err.data_ptr(), out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return _written(col_err, ncols, "col_err").cpu().numpy(), float(_written(out, 1, "out").cpu()[0])


def _rank_direct(scores, perm, n, n_pos):
    out = _sentinel(3, torch.float64)
    assert _hip.lib().sgmcmc_rank_metrics(scores.data_ptr(), perm.data_ptr(), n, n_pos, out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return _written(out, 3, "out").cpu().tolist()


def _table(rng, E, N, C, shift=None):
    "random normalised log-probabilities [E, N, C]; shift: added to the logits before normalising (-inf: a dead entry)"
    f = rng.normal(scale=3.0, size=(E, N, C))
    if shift is not None:
        f = f + shift
    with np.errstate(divide="ignore"):
        return f - np.log(np.exp(f).sum(-1, keepdims=True))


def _check_ensemble(got, acc, y):
    "device (probs, conf, pred, hit) against the host's fp64 and against the device's own probs"
    probs, conf, pred, hit = got
    np.testing.assert_allclose(probs, np_ensemble_probs(acc), rtol=0, atol=1e-13, equal_nan=True)
    arg = probs.argmax(1)                                   # np.argmax: the first maximum, the first NaN
    assert np.array_equal(pred, arg)
    assert np.array_equal(conf, probs[np.arange(len(arg)), arg], equal_nan=True)
    assert np.array_equal(hit, (arg == y).astype(np.int64))
    return float(np.nanmax(np.abs(probs - np_ensemble_probs(acc)))) if not np.isnan(probs).all() else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("C", ENS_C)
def test_ensemble_kernel_on_the_grid(C):
    rng = np.random.default_rng(500 + C)
    worst = 0.0
    for E, N, _ in [g for g in ENS_GRID if g[2] == C]:
        y = rng.integers(0, C, N)
        base = _table(rng, E, N, C)
        plain = _ensemble_direct(base, y)
        worst = max(worst, _check_ensemble(plain, base, y))
        assert _ensemble_direct(base)[0].tobytes() == plain[0].tobytes()            # without labels: hit stays NULL
        # one NaN entry: its row is NaN, every other row keeps its bits
        e0, n0, c0 = E // 2, N // 2, C // 2
        acc = base.copy()
        acc[e0, n0, c0] = np.nan
        got = _ensemble_direct(acc, y)
        _check_ensemble(got, acc, y)
        assert np.isnan(got[0][n0]).all() and np.isnan(got[1][n0]) and got[2][n0] == 0
        others = np.arange(N) != n0
        assert all(g_[others].tobytes() == p_[others].tobytes() for g_, p_ in zip(got, plain))
        if C == 1:
            assert (plain[0] == 1.0).all()                  # the softmax of one class
            continue
        # class c0 dead in every sample: exactly 0, and the row still sums to 1
        shift = np.zeros(C)
        shift[c0] = -np.inf
        acc = _table(rng, E, N, C, shift)
        got = _ensemble_direct(acc, y)
        worst = max(worst, _check_ensemble(got, acc, y))
        assert (got[0][:, c0] == 0.0).all() and np.abs(got[0].sum(1) - 1.0).max() <= 1e-13
        # ... dead in some (sample, row) pairs only
        shift = np.zeros((E, N, C))
        shift[..., c0] = np.where(rng.random((E, N)) < 0.5, -np.inf, 0.0)
        shift[E - 1, N - 1, c0] = -np.inf
        acc = _table(rng, E, N, C, shift)
        got = _ensemble_direct(acc, y)
        worst = max(worst, _check_ensemble(got, acc, y))
        # two identical columns that hold the maximum: the lower index is the prediction
        lo, hi = C // 3, C - 1
        f = rng.normal(scale=3.0, size=(E, N, C))
        f[..., lo] += 40.0
        f[..., hi] = f[..., lo]
        acc = f - np.log(np.exp(f).sum(-1, keepdims=True))
        got = _ensemble_direct(acc, y)
        _check_ensemble(got, acc, y)
        assert got[0][:, lo].tobytes() == got[0][:, hi].tobytes() and (got[2] == lo).all()
    print(f"ensemble_kernel at C = {C}: max |probs - host| = {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", ORDER_N)
def test_ordering_kernel_on_the_grid(n):
    rng = np.random.default_rng(600 + n)
    for kind in ORDER_KINDS:
        a = _order_keys(kind, n, rng)
        want = np.argsort(a, kind="stable")
        got = _order_direct(_dev(a), 1, 1, n, 1).cpu().numpy()                      # one contiguous column
        assert np.array_equal(got[0], want), (kind, n)
        m = np.stack([a, _order_keys(kind, n, rng), _order_keys(kind, n, rng)], 1)  # three columns of a row-major [n, 3]
        got = _order_direct(_dev(m), 3, 1, n, 3).cpu().numpy()
        for j in range(3):
            assert np.array_equal(got[j], np.argsort(m[:, j], kind="stable")), (kind, n, j)
        got = _order_direct(_dev(m), 3, 0, n, 3).cpu().numpy()                      # col_stride 0: column 0 three times
        for j in range(3):
            assert np.array_equal(got[j], want), (kind, n, j)


@pytest.mark.gpu
@pytest.mark.parametrize("n", CALIB_N)
def test_calibration_kernel_on_the_grid(n):
    "one column through sgmcmc_calibration_error against the rationals: every n x num_bins x scheme x key kind"
    rng = np.random.default_rng(100 + n)              # the inputs of test_exact_gce_and_np_gce_agree_on_the_grid
    worst = 0.0
    for num_bins in CALIB_BINS:
        for scheme, l2 in CALIB_SCHEMES:
            if scheme == "even" and num_bins == 0:
                continue                               # refused (test_c_abi_refuses_...)
            for kind in CALIB_KINDS:
                keys, hits = _calib_keys(kind, n, num_bins, rng), rng.integers(0, 2, n)
                bounds = _bounds(scheme, num_bins)
                exact = float(exact_gce(keys, hits, bounds=bounds, num_bins=num_bins, l2=l2))
                k = _dev(keys)
                col_err, out = _calib_direct(k, _order_direct(k, 1, 0, n, 1), _dev(hits), False, n, 1, 1, 0, bounds,
                                             num_bins, l2)
                what = (n, num_bins, scheme, l2, kind)
                assert abs(col_err[0] - exact) <= 1e-12, (what, col_err[0], exact)
                assert abs(out - (math.sqrt(exact) if l2 else exact)) <= 1e-12, (what, out, exact)
                if kind == "nonpositive":
                    assert col_err[0] == 0.0 and out == 0.0
                worst = max(worst, abs(col_err[0] - exact), abs(out - (math.sqrt(exact) if l2 else exact)))
    print(f"calib_kernel at n = {n}: max |device - exact| = {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", CALIB_C)
def test_class_conditional_calibration_on_the_grid(C):
    "C strided columns of a row-major matrix, column j of key kind j mod 6, hits = (label == j)"
    rng = np.random.default_rng(700 + C)
    worst = 0.0
    for n in CALIB_N:
        for num_bins in (0, 1, 3, 30, 257, 4096):
            keys = np.stack([_calib_keys(CALIB_KINDS[j % 6], n, num_bins, rng) for j in range(C)], 1)
            labels = rng.integers(0, C, n)
            exact = [exact_gce(keys[:, j], (labels == j).astype(np.int64), num_bins=num_bins) for j in range(C)]
            k = _dev(keys)
            col_err, out = _calib_direct(k, _order_direct(k, C, 1, n, C), _dev(labels), True, n, C, C, 1, None,
                                         num_bins, False)
            dev = max(np.abs(col_err - np.array([float(e) for e in exact])).max(), abs(out - float(sum(exact) / C)))
            assert dev <= 1e-12, (n, num_bins, dev)
            worst = max(worst, dev)
    print(f"calib_kernel, class-conditional at C = {C}: max |device - exact| = {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", CALIB_N)
def test_calibration_wrappers_on_the_grid(n):
    rng = np.random.default_rng(800 + n)
    worst = 0.0
    for C in (1, 2, 7, 128):
        p = rng.random((n, 1)) if C == 1 else rng.dirichlet(np.full(C, 0.5), size=n)
        y = rng.integers(0, max(C, 2), n)
        combos = ((1, 1), (2, 100), (3, 2), (30, 7), (255, 1), (256, 64), (257, 3), (4096, 1))
        for num_bins, dpb in combos if C < 128 else combos[2::5]:      # (the rationals of 128 columns take their time)
            got = cal.calibration_metrics(_dev(y), _dev(p), num_bins=num_bins, datapoints_per_bin=dpb)
            exact = exact_metrics(y, p, num_bins, dpb)
            want = {"ece": float(exact["ece"]), "ace": float(exact["ace"]), "rmsce": math.sqrt(exact["rmsce2"])}
            for k in want:
                assert abs(got[k] - want[k]) <= 1e-12, (n, C, num_bins, dpb, k, got[k], want[k])
                worst = max(worst, abs(got[k] - want[k]))
    print(f"calibration_metrics at N = {n}: max |device - exact| = {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", RANK_N)
def test_rank_kernel_on_the_grid(n):
    rng = np.random.default_rng(900 + n)
    worst = 0.0
    for P in _rank_P(n):
        for kind in RANK_KINDS:
            s = _rank_scores(kind, n, P, rng)
            sd = _dev(s)
            perm = _order_direct(sd, 1, 0, n, 1)
            assert np.array_equal(perm.cpu().numpy()[0], np.argsort(s, kind="stable"))
            auroc, ap, has_nan = _rank_direct(sd, perm, n, P)
            exact, want_ap = exact_auroc_auprc(s[:P], s[P:])
            assert has_nan == 0.0 and auroc == float(mann_whitney_auroc(s[:P], s[P:])) == float(exact), (n, P, kind)
            assert abs(ap - want_ap) <= 1e-12, (n, P, kind, ap, want_ap)
            if kind.startswith("separable"):
                assert auroc == (1.0 if kind == "separable_up" else 0.0)
            worst = max(worst, abs(ap - want_ap))
    print(f"rank_kernel at n = {n}: max |AP - host| = {worst:.3g}")


@pytest.mark.gpu
def test_order_and_rank_kernels_at_the_row_limit():
    """n = MAX_ROWS two-valued scores: the stable order is the low rows in order, then the high rows in order, and both
    metrics follow from four counts -- a positives and b negatives at the high value"""
    n, P = cal.MAX_ROWS, 50001
    rng = np.random.default_rng(131072)
    high = rng.random(n) < 0.375
    s = np.where(high, 0.75, 0.25)
    sd = _dev(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    perm = _order_direct(sd, 1, 0, n, 1)
    t1 = time.perf_counter()
    auroc, ap, has_nan = _rank_direct(sd, perm, n, P)
    t2 = time.perf_counter()
    print(f"n = {n}: sgmcmc_stable_order {t1 - t0:.4f} s, sgmcmc_rank_metrics {t2 - t1:.4f} s (launch to host)")
    assert np.array_equal(perm.cpu().numpy()[0], np.r_[np.nonzero(~high)[0], np.nonzero(high)[0]])
    Nn, a, b = n - P, int(high[:P].sum()), int(high[P:].sum())
    assert has_nan == 0.0
    assert auroc == float(Fraction(2 * a * (Nn - b) + a * b + (P - a) * (Nn - b), 2 * P * Nn))
    want_ap = (a / P) * (a / (a + b)) + (P / P - a / P) * (P / n)
    assert abs(ap - want_ap) <= 1e-12, (ap, want_ap)


@pytest.mark.gpu
def test_wrappers_take_other_dtypes_and_strides_to_the_same_bits():
    g = _golden()
    rng = np.random.default_rng(41)
    N, C = 333, 7
    p32 = rng.dirichlet(np.full(C, 0.5), size=N).astype(np.float32)
    y = rng.integers(0, C, N)
    kw = dict(num_bins=7, datapoints_per_bin=20)
    base = cal.calibration_metrics(_dev(y), _dev(p32.astype(np.float64)), **kw)
    wide = np.full((N, C + 5), 0.5, np.float32)
    wide[:, 2:2 + C] = p32
    sliced = _dev(wide)[:, 2:2 + C]
    assert not sliced.is_contiguous()
    assert cal.calibration_metrics(_dev(y, torch.int32), _dev(p32), **kw) == base
    assert cal.calibration_metrics(_dev(y), sliced, **kw) == base
    assert cal.calibration_metrics(_dev(y), _dev(wide.astype(np.float64))[:, 2:2 + C], **kw) == base
    acc32 = _table(rng, 5, N, C).astype(np.float32)
    want = cal.ensemble_probs(_dev(acc32.astype(np.float64)), _dev(y))
    got = cal.ensemble_probs(_dev(acc32), _dev(y, torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    got = cal.ensemble_probs(_dev(np.concatenate([acc32, acc32], 2))[..., :C], _dev(y))      # a non-contiguous table
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    s = rng.random(700).astype(np.float32)
    assert cal.auroc_auprc(_dev(s[:300]), _dev(s[300:])) == \
        cal.auroc_auprc(_dev(s[:300].astype(np.float64)), _dev(s[300:].astype(np.float64)))
    # [N, 1] is the binary problem [[1 - p, p]]
    y1, p1 = g["cal__single_column__labels"], g["cal__single_column__probs"]
    got = cal.calibration_metrics(_dev(y1), _dev(p1))
    assert got == cal.calibration_metrics(_dev(y1), _dev(np.concatenate([1.0 - p1, p1], 1)))
    for k in ("ece", "ace", "rmsce"):
        assert abs(got[k] - float(g[f"cal__single_column__{k}"])) <= 1e-12
    assert (cal.ensemble_probs(_dev(np.zeros((3, 5, 1)))).probs == 1.0).all()       # ... but stays one class here


@pytest.mark.gpu
def test_c_abi_refuses_out_of_range_arguments_and_writes_nothing():
    lib, stream = _hip.lib(), _stream()
    E, N, C = 3, 40, 5
    rng = np.random.default_rng(1)
    acc, y = _dev(_table(rng, E, N, C)), _dev(rng.integers(0, C, N))
    f64 = {k: _sentinel(n, torch.float64) for k, n in (("probs", N * C), ("conf", N), ("col_err", C), ("out", 3))}
    i64 = {k: _sentinel(N, torch.int64) for k in ("pred", "hit")}
    perm = _sentinel(C * N, torch.int32)
    A, Y, PR, CF, PD, HT = (t.data_ptr() for t in (acc, y, f64["probs"], f64["conf"], i64["pred"], i64["hit"]))
    PM, CE, OUT = perm.data_ptr(), f64["col_err"].data_ptr(), f64["out"].data_ptr()
    big = cal.MAX_ROWS + 1
    refused = {
        "sgmcmc_ensemble_probs": [
            (None, Y, E, N, C, PR, CF, PD, HT), (A, Y, E, N, C, None, CF, PD, HT), (A, Y, E, N, C, PR, None, PD, HT),
            (A, Y, E, N, C, PR, CF, None, HT), (A, Y, E, N, C, PR, CF, PD, None), (A, None, E, N, C, PR, CF, PD, HT),
            (A, Y, 0, N, C, PR, CF, PD, HT), (A, Y, -1, N, C, PR, CF, PD, HT), (A, Y, E, 0, C, PR, CF, PD, HT),
            (A, Y, E, -1, C, PR, CF, PD, HT), (A, Y, E, N, 0, PR, CF, PD, HT), (A, Y, E, N, -1, PR, CF, PD, HT),
            (A, Y, E, N, cal.MAX_CLASSES + 1, PR, CF, PD, HT)],
        "sgmcmc_row_max": [
            (None, Y, N, C, CF, PD, HT), (A, Y, N, C, None, PD, HT), (A, Y, N, C, CF, None, HT),
            (A, Y, N, C, CF, PD, None), (A, None, N, C, CF, PD, HT), (A, Y, 0, C, CF, PD, HT), (A, Y, -1, C, CF, PD, HT),
            (A, Y, N, 0, CF, PD, HT), (A, Y, N, -1, CF, PD, HT), (A, Y, N, cal.MAX_CLASSES + 1, CF, PD, HT)],
        "sgmcmc_stable_order": [
            (None, C, 1, N, C, PM), (A, C, 1, N, C, None), (A, C, 1, 0, C, PM), (A, C, 1, -1, C, PM),
            (A, C, 1, big, C, PM), (A, C, 1, N, 0, PM), (A, C, 1, N, -1, PM), (A, C, 1, N, 65536, PM),
            (A, 0, 1, N, C, PM), (A, -1, 1, N, C, PM), (A, C, -1, N, C, PM)],
        # (keys, elem_stride, col_stride, perm, target, class_conditional, n, ncols, bounds, num_bins, l2, col_err, out)
        "sgmcmc_calibration_error": [
            (None, C, 1, PM, Y, 1, N, C, None, 30, 0, CE, OUT), (A, C, 1, None, Y, 1, N, C, None, 30, 0, CE, OUT),
            (A, C, 1, PM, None, 1, N, C, None, 30, 0, CE, OUT), (A, C, 1, PM, Y, 1, N, C, None, 30, 0, None, OUT),
            (A, C, 1, PM, Y, 1, N, C, None, 30, 0, CE, None), (A, C, 1, PM, Y, 1, 0, C, None, 30, 0, CE, OUT),
            (A, C, 1, PM, Y, 1, -1, C, None, 30, 0, CE, OUT), (A, C, 1, PM, Y, 1, big, C, None, 30, 0, CE, OUT),
            (A, C, 1, PM, Y, 1, N, 0, None, 30, 0, CE, OUT), (A, C, 1, PM, Y, 1, N, -1, None, 30, 0, CE, OUT),
            (A, C, 1, PM, Y, 1, N, 65536, None, 30, 0, CE, OUT), (A, C, 1, PM, Y, 0, N, 2, None, 30, 0, CE, OUT),
            (A, 0, 1, PM, Y, 1, N, C, None, 30, 0, CE, OUT), (A, -1, 1, PM, Y, 1, N, C, None, 30, 0, CE, OUT),
            (A, C, -1, PM, Y, 1, N, C, None, 30, 0, CE, OUT), (A, C, 1, PM, Y, 1, N, C, None, -1, 0, CE, OUT),
            (A, C, 1, PM, Y, 1, N, C, None, cal.MAX_BINS + 1, 0, CE, OUT), (A, C, 1, PM, Y, 1, N, C, A, 0, 0, CE, OUT)],
        "sgmcmc_rank_metrics": [
            (None, PM, N, 7, OUT), (A, None, N, 7, OUT), (A, PM, N, 7, None), (A, PM, 0, 0, OUT), (A, PM, -1, -2, OUT),
            (A, PM, big, 7, OUT), (A, PM, N, 0, OUT), (A, PM, N, -1, OUT), (A, PM, N, N, OUT), (A, PM, N, N + 1, OUT)],
    }
    for name, calls in refused.items():
        for args in calls:
            assert getattr(lib, name)(*args, stream) == INVALID_VALUE, (name, args)
    torch.cuda.synchronize()
    for k, t in {**f64, **i64, "perm": perm}.items():
        assert bool(_is_sentinel(t).all()), k
    # ... and the same buffers are accepted with the arguments in range
    assert lib.sgmcmc_ensemble_probs(A, Y, E, N, C, PR, CF, PD, HT, stream) == 0
    assert lib.sgmcmc_stable_order(PR, C, 1, N, C, PM, stream) == 0
    assert lib.sgmcmc_calibration_error(PR, C, 1, PM, Y, 1, N, C, None, 30, 0, CE, OUT, stream) == 0
    torch.cuda.synchronize()
    probs = _written(f64["probs"], N * C, "probs").view(N, C)
    _written(perm, C * N, "perm"), _written(f64["col_err"], C, "col_err")
    assert bool(_is_sentinel(f64["out"])[1:].all())
    assert float(f64["out"][0]) == cal.ace(y, probs)
