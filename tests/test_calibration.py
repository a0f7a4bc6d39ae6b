"""Calibration and out-of-distribution metrics on the device (bnn_priors_amd/calibration.py, csrc/calib_hip.inc;
reference: bnn_priors/third_party/calibration_error.py, exp_utils.py:323-327,343-380).

A numpy restatement of the kernels' arithmetic -- sorted columns, bins as contiguous ranges of them, integer counts --
is pinned to the goldens the reference's own code produced (tests/golden/make_calibration_goldens.py) on the CPU; the
GPU tests hold the kernels to the goldens and to that restatement, and the model-level evaluation to the restatement
applied to its own predictive tables."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from bnn_priors_amd import calibration as cal
from bnn_priors_amd import evaluation as ev

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calibration.npz")
EPS = np.finfo(np.float64).eps


def _golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _cases(prefix):
    g = _golden()
    return sorted({k.split("__")[1] for k in g if k.startswith(prefix + "__")})


# ---- the numpy restatement ------------------------------------------------------------------------------------------

def np_gce(keys, hits, bounds=None, num_bins=None, l2=False):
    "one column: keys > 0 kept, sorted; bins = ranges of the sorted column between the np.digitize bounds"
    keep = keys > 0
    order = np.argsort(keys[keep], kind="stable")
    s, h = keys[keep][order], np.asarray(hits)[keep][order]
    m = len(s)
    if m == 0:
        return 0.0
    if bounds is None:                 # num_bins <= 1: no upper bound, one bin
        step = m / num_bins if num_bins else 0.0
        bounds = s[np.minimum(np.rint(np.arange(1, max(num_bins, 1)) * step), m - 1).astype(np.int64)]
    edges = np.concatenate([[0], np.searchsorted(s, bounds, side="left"), [m]])
    err = 0.0
    for a, b in zip(edges[:-1], edges[1:]):
        cnt = float(b - a) + EPS
        e = (float(h[a:b].sum()) / cnt - s[a:b].sum() / cnt) * (cnt / m)
        err += e * e if l2 else abs(e)
    return err


def np_metrics(labels, probs, num_bins=30, datapoints_per_bin=100):
    labels, probs = np.asarray(labels), np.asarray(probs, dtype=np.float64)
    N, C = probs.shape
    pred = probs.argmax(1)
    conf = probs[np.arange(N), pred]
    hit = (pred == labels).astype(np.int64)
    bounds = np.histogram_bin_edges([], bins=num_bins, range=(0.0, 1.0))[1:]
    return {"ece": np_gce(conf, hit, bounds=bounds),
            "ace": sum(np_gce(probs[:, j], (labels == j).astype(np.int64), num_bins=num_bins) / C for j in range(C)),
            "rmsce": math.sqrt(np_gce(conf, hit, num_bins=int(N / datapoints_per_bin), l2=True))}


def exact_auroc_auprc(s_in, s_out):
    """AUROC as an exact rational (trapezoids in Python ints) and average precision over the distinct thresholds in
    descending order"""
    scores = np.concatenate([s_in, s_out])
    pos = np.concatenate([np.ones(len(s_in), np.int64), np.zeros(len(s_out), np.int64)])
    order = np.argsort(-scores, kind="stable")
    scores, pos = scores[order], pos[order]
    P, Nn = len(s_in), len(s_out)
    last = np.r_[np.nonzero(np.diff(scores))[0], len(scores) - 1]      # the last position of each tie group
    tps = np.cumsum(pos)[last]
    fps = last + 1 - tps
    area2, ap, tp0, fp0 = 0, 0.0, 0, 0
    for tp, fp in zip(tps.tolist(), fps.tolist()):
        area2 += (fp - fp0) * (tp + tp0)
        ap += (tp / P - tp0 / P) * (tp / (tp + fp))
        tp0, fp0 = tp, fp
    return Fraction(area2, 2 * P * Nn), ap


def np_ensemble_probs(acc):
    "Categorical(logits=logsumexp_e acc - log E).probs, fp64 on the host"
    a = torch.as_tensor(acc, dtype=torch.float64).cpu()
    lme = a.logsumexp(0) - math.log(a.shape[0])
    return torch.softmax(lme, -1).numpy()


# ---- CPU: the restatement against the reference's numbers, argument checks ------------------------------------------

@pytest.mark.parametrize("case", _cases("cal"))
def test_restatement_reproduces_the_reference_calibration_goldens(case):
    g = _golden()
    got = np_metrics(g[f"cal__{case}__labels"], g[f"cal__{case}__probs"])
    for k in ("ece", "ace", "rmsce"):
        assert abs(got[k] - float(g[f"cal__{case}__{k}"])) <= 1e-15, (k, got[k], float(g[f"cal__{case}__{k}"]))


@pytest.mark.parametrize("case", _cases("ood"))
def test_restatement_reproduces_the_reference_ood_goldens(case):
    g = _golden()
    auroc, ap = exact_auroc_auprc(g[f"ood__{case}__in"], g[f"ood__{case}__out"])
    assert abs(float(auroc) - float(g[f"ood__{case}__auroc"])) <= 1e-15
    assert abs(ap - float(g[f"ood__{case}__auprc"])) <= 1e-15


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
    got = cal.calibration_metrics(y, p)
    for k in ("ece", "ace", "rmsce"):
        assert abs(got[k] - float(g[f"cal__{case}__{k}"])) <= 1e-12, (k, got[k], float(g[f"cal__{case}__{k}"]))
    assert cal.ece(y, p) == got["ece"] and cal.ace(y, p) == got["ace"] and cal.rmsce(y, p) == got["rmsce"]


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
