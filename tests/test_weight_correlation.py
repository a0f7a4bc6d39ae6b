"""Weight-correlation analysis on the device (bnn_priors_amd/weight_correlation.py, csrc/corr_hip.inc; definitions in
include/sgmcmc_hip.h, restated in tests/weight_correlation_reference.py).

On the CPU the restatement is held to independent code (numpy.cov, numpy.corrcoef, a Monte Carlo of Gaussian matrices for
Schott's moments), the geometry builder to a brute-force enumeration of (variable, observation) -> element offset, the
wrappers to their argument checks, and the permutation test to what it is for.  On the GPU the kernels are held to the
restatement.

Shapes.  The Gram pass forms TILE x TILE = 64 x 64 blocks from chunks of KC = CHUNK = 32 observations, ``splits(V, n,
workspace_bytes)`` workgroups sharing the chunks of a block pair: V in {1, 2, 17, 64, 65, 130} is one partial tile, one
exact tile, one past it and three block rows with a partial last (17 and 65 are also the test of the fp64 MFMA's C/D lane
map: the fp32 map would put 3 of 4 results in the wrong row); n in {2, 3, KC - 1, KC + 1} and 2 splits + 1 chunks with a
ragged tail, at the default workspace (64 splits) and at one that leaves 3.

Tolerances.  They are measured, not guessed: the restatement is evaluated on the GPU tests' own inputs in np.float64 and
in np.longdouble (80-bit), the largest deviation per quantity over all cases is recorded, and the GPU tolerance is 4 x that
(the factor allows for the kernels' other summation order and the MFMA's internal order).

  mean   relative to the variable's standard deviation:        measured 5.83e-13 (MEAN_DEVIATION = 5.9e-13; the variable
         1e4 standard deviations from 0 sets it: half an ulp of the mean itself)
  cov    relative to sqrt(cov_ii cov_jj):                       measured 1.13e-15 (COV_DEVIATION = 1.2e-15)
  corr   absolute (relative to 1):                              measured 9.65e-16 (CORR_DEVIATION = 9.7e-16)
  stats  mean r, mean |r|, rms r, max |r|, sum r^2 of the cases and the null tables of the permutation data, relative:
                                                                measured 1.79e-15 (STAT_DEVIATION = 1.8e-15)

``test_the_recorded_deviations_are_the_measured_ones`` re-measures them.  Counts, flags and arg-max pairs must be equal.

The permutation data (V = 24, n = 200, Student-t with 3 degrees of freedom times 0.05 rounded to float32, B = 99 tables
from ``numpy.random.default_rng(PERM_SEED).permutation``): PERM_SEED = 1 gives an rms p-value of 0.87 on the independent
data (the nearest null value of either statistic is 4.6e-5 away) and 0.01 with the shared factor (2.0e-3 away).
"""
import functools

import numpy as np
import pytest
import torch

import weight_correlation_reference as ref

MEAN_DEVIATION = 5.9e-13
COV_DEVIATION = 1.2e-15
CORR_DEVIATION = 9.7e-16
STAT_DEVIATION = 1.8e-15
PERM_SEED = 1
PERM_V, PERM_N, PERM_B = 24, 200, 99

LD = np.longdouble
KC, TILE = 32, 64                    # asserted against the module's constants below
STATS = ("mean", "mean_abs", "rms", "max_abs", "sum_sq")
SMALL = 3 * 8 * 65 * 65              # a workspace that leaves 3 splits at V = 65

# name: (S, shape, var_dim, dtype, view, special, ddof, workspace_bytes or None)
#   view: "t" a transposed stack (axes 1 and 2 of the allocation swapped), "s" every second sample of a longer one
#   special: "far" variable 1 lies 1e4 of its standard deviations from 0, "const" variable 0 is constant (0.1: no exact
#   float), "bad" one NaN and one Inf
CASES = {
    "v1": (5, (1, 7), 0, "float32", "", "", 1, None),
    "v2_n2": (2, (2,), 0, "float64", "", "", 1, None),
    "v17_n3": (3, (17,), 0, "float64", "", "", 0, None),
    "v64_kc_minus": (KC - 1, (64,), 0, "float32", "", "", 1, None),
    "v65_kc_plus": (KC + 1, (65,), 0, "float64", "", "", 2, None),
    "v65_three_splits": (7 * KC - 9, (65,), 0, "float32", "", "", 1, SMALL),
    "v130_all_splits": (3, (1367, 130), 1, "float32", "", "", 1, None),          # n = 4101 = 128 KC + 5: 129 chunks
    "dense_rows": (7, (17, 40), 0, "float32", "", "", 1, None),
    "dense_cols": (7, (17, 40), 1, "float64", "", "", 1, None),
    "dense_cols_negative": (7, (17, 40), -1, "float32", "", "", 1, None),
    "conv_out": (4, (6, 5, 3, 3), 0, "float32", "", "", 1, None),
    "conv_in": (4, (6, 5, 3, 3), 1, "float64", "", "", 1, None),
    "transposed": (9, (20, 70), 0, "float32", "t", "", 1, None),
    "transposed_cols": (9, (20, 70), 1, "float64", "t", "", 1, None),
    "strided_samples": (6, (66, 5), 0, "float64", "s", "", 1, None),
    "conv_strided_samples": (5, (3, 7, 3, 3), 1, "float32", "s", "", 1, None),
    "far_mean": (40, (9, 4), 0, "float64", "", "far", 1, None),
    "far_mean_f32": (40, (9, 4), 0, "float32", "", "far", 1, None),
    "constant": (11, (5, 13), 0, "float32", "", "const", 1, None),
    "constant_cols": (11, (5, 13), 1, "float64", "", "const", 1, None),
    "nan_inf": (6, (8, 9), 0, "float32", "", "bad", 1, None),
}
VIEWS = tuple(n for n in sorted(CASES) if CASES[n][4])


def _apply_view(base, view):
    if view == "t":
        return base.transpose(1, 2) if isinstance(base, torch.Tensor) else np.swapaxes(base, 1, 2)
    if view == "s":
        return base[::2]
    return base


@functools.lru_cache(maxsize=None)
def _base(name):
    "the allocation of a case as a read-only numpy array: ``_apply_view`` of it is the stack"
    S, shape, var_dim, dtype, view, special, _, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    axis = 1 + var_dim % len(shape)
    fshape = [S, *shape]
    fshape[axis] = 1
    # a shared factor per observation: the correlations are well away from 0, so every statistic is well conditioned
    w = 0.05 * (rng.standard_t(4, size=(S, *shape)) + 0.9 * rng.standard_t(4, size=fshape))
    w = w.astype(dtype)
    index = [slice(None)] * w.ndim
    if special == "far":
        index[axis] = 1
        w[tuple(index)] += np.asarray(1e4 * w[tuple(index)].std(), dtype=dtype)
    if special == "const":
        index[axis] = 0
        w[tuple(index)] = 0.1
    if special == "bad":
        w.reshape(-1)[7] = np.nan
        w.reshape(-1)[w.size - 3] = np.inf
    if view == "t":
        base = np.ascontiguousarray(np.swapaxes(w, 1, 2))
    elif view == "s":
        base = rng.standard_normal((2 * S, *shape)).astype(dtype)
        base[::2] = w
    else:
        base = w
    assert np.array_equal(_apply_view(base, view), w, equal_nan=True)
    base.setflags(write=False)
    return base


def _stack(name):
    return _apply_view(_base(name), CASES[name][4])


@functools.lru_cache(maxsize=None)
def _ref(name, wide):
    "the restatement of a case: covariance and the off-diagonal statistics of its correlation matrix"
    dtype = LD if wide else np.float64
    out = ref.covariance(ref.as_matrix(_stack(name), CASES[name][2]), CASES[name][6], dtype)
    out["offdiag"] = ref.offdiag(out["corr"], dtype)
    return out


@functools.lru_cache(maxsize=None)
def _perm_data():
    "(independent [V, n] float32, the same plus a shared factor, tables [B, V, n] int64)"
    rng = np.random.default_rng(PERM_SEED)
    z = rng.standard_t(3, size=(PERM_V, PERM_N))
    f = rng.standard_t(3, size=(1, PERM_N))
    tables = np.stack([np.stack([rng.permutation(PERM_N) for _ in range(PERM_V)]) for _ in range(PERM_B)])
    return (0.05 * z).astype(np.float32), (0.05 * (z + 0.35 * f)).astype(np.float32), tables.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _perm_ref(factor, wide):
    x = _perm_data()[1 if factor else 0]
    return ref.permutation_test(x, _perm_data()[2], LD if wide else np.float64)


def _rel(a, b):
    return float(abs(LD(a) - LD(b)) / abs(LD(b)))


def _deviations(got, wide):
    "largest deviation per quantity of a result (dict as the restatement's) from the 80-bit restatement"
    keep = ~wide["zero_variance"]
    sd = np.sqrt(np.diag(wide["cov"])[keep])
    out = dict(mean=0.0, cov=0.0, corr=0.0, stats=0.0)
    if keep.any() and not wide["nonfinite"]:
        scale = sd[:, None] * sd[None, :]
        pick = np.ix_(keep, keep)
        out["mean"] = float(np.max(np.abs(LD(1) * got["mean"][keep] - wide["mean"][keep]) / sd))
        out["cov"] = float(np.max(np.abs(LD(1) * got["cov"][pick] - wide["cov"][pick]) / scale))
        out["corr"] = float(np.max(np.abs(LD(1) * got["corr"][pick] - wide["corr"][pick])))
    if wide["offdiag"]["pairs"]:
        out["stats"] = max(_rel(got["offdiag"][k], wide["offdiag"][k]) for k in STATS)
    return out


@functools.lru_cache(maxsize=None)
def _measure():
    worst = dict(mean=0.0, cov=0.0, corr=0.0, stats=0.0)
    for name in CASES:
        for k, v in _deviations(_ref(name, False), _ref(name, True)).items():
            worst[k] = max(worst[k], v)
    for factor in (False, True):
        a, b = _perm_ref(factor, False), _perm_ref(factor, True)
        worst["stats"] = max(worst["stats"], float(np.max(np.abs(LD(1) * a["null"] - b["null"]) / b["null"])),
                             *(_rel(a["observed"][k], b["observed"][k]) for k in ("rms", "max_abs", "sum_sq")))
    return worst


# ------------------------------------------------------------------------------------------------------------------ CPU

def test_module_constants_are_the_ones_the_shapes_are_built_on():
    from bnn_priors_amd import _hip, weight_correlation as wc
    assert (wc.CHUNK, wc.TILE, wc.MAX_V) == (KC, TILE, 1024)
    assert wc.splits(130, 4101) == 64 and -(-4101 // KC) == 2 * 64 + 1 and 4101 % KC        # two each, one a third, ragged
    assert wc.splits(65, 7 * KC - 9, SMALL) == 3 and -(-(7 * KC - 9) // KC) == 2 * 3 + 1
    assert wc.splits(65, 100, 8 * 65 * 65 - 1) == 0
    lib = _hip.lib()
    for V, n, ws in ((1, 2, 1 << 20), (64, 31, 1 << 28), (65, 215, SMALL), (130, 4101, 1 << 28), (1024, 10 ** 6, 1 << 28),
                     (1024, 2 ** 31 - 1, 1 << 26), (784, 10 ** 4, 1 << 28), (300, 77, 0)):
        assert wc.splits(V, n, ws) == lib.sgmcmc_corr_splits(V, n, ws), (V, n, ws)
        assert wc.mean_blocks(V, n) == lib.sgmcmc_corr_mean_blocks(V, n), (V, n)
    assert lib.sgmcmc_corr_splits(1025, 10, 1 << 20) == -1 and lib.sgmcmc_corr_splits(4, 1, 1 << 20) == -1


def test_gram_splits_are_the_formulas_from_before_the_shared_helper():
    """``_gram_pass.splits`` and the two public ``splits`` against the formulas that ``weight_correlation.splits`` and
    ``stein.splits`` spelled out before they shared it, restated literally (TILE 64, CHUNK 32, 64 splits at most, 1,024
    target blocks), at the edges of every term: V around the tile, lengths around the chunk and at the limit, workspaces
    around one V x V matrix of doubles."""
    from bnn_priors_amd import _gram_pass, _hip, stein, weight_correlation as wc
    assert (wc.TILE, wc.CHUNK, wc.MAX_SPLITS, _hip.CORR_TARGET_BLOCKS) == (64, 32, 64, 1024)
    assert (stein.TILE, stein.CHUNK, stein.MAX_SPLITS, _hip.STEIN_TARGET_BLOCKS) == (64, 32, 64, 1024)

    def corr_before(V, n, workspace_bytes):
        nb = -(-V // 64)
        return max(0, min(-(-n // 32), 64, 1024 // (nb * (nb + 1) // 2), workspace_bytes // (8 * V * V)))

    def stein_before(S, D, workspace_bytes):
        nb = -(-2 * S // 64)
        return max(0, min(-(-D // 32), 64, 1024 // (nb * (nb + 1) // 2), workspace_bytes // (8 * 4 * S * S)))

    seen = set()
    for V in (1, 64, 65, 1024, 2048):
        for length in (1, 31, 32, 33, 2 ** 20, 2 ** 31 - 1):
            for ws in (0, 8 * V * V - 1, 8 * V * V, 256 << 20):
                want = corr_before(V, length, ws)
                assert _gram_pass.splits(V, length, ws, 64, 32, 64, 1024) == want == wc.splits(V, length, ws), (V, length, ws)
                assert stein.splits(V, length, ws) == stein_before(V, length, ws), (V, length, ws)
                if V % 2 == 0:                               # the same matrix as stein's 2S rows
                    assert stein.splits(V // 2, length, ws) == want, (V, length, ws)
                seen.add(want)
    assert {0, 1, 2, 7, 64} <= seen                          # every term of the minimum decides somewhere
    assert wc.splits(130, 4101) == corr_before(130, 4101, wc.WORKSPACE_BYTES) == 64
    assert stein.splits(65, 215) == stein_before(65, 215, stein.WORKSPACE_BYTES) == 7


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_numpy(name):
    x = ref.as_matrix(_stack(name), CASES[name][2])
    ddof = CASES[name][6]
    for dtype in (np.float64, LD):
        got = ref.covariance(x, ddof, dtype)
        assert got["mean"].dtype == dtype and got["n"] == x.shape[1]
        if CASES[name][5] == "bad":
            assert got["nonfinite"] == 2 and np.isnan(got["mean"]).all() and np.isnan(got["cov"]).all()
            assert np.isnan(got["corr"]).all() and not got["zero_variance"].any()
            assert ref.offdiag(got["corr"], dtype)["pairs"] == 0
            continue
        x64 = x.astype(np.float64)
        sd = x64.std(axis=1)
        zero = np.ptp(x64, axis=1) == 0
        assert np.array_equal(got["zero_variance"], zero) and zero.any() == (CASES[name][5] == "const")
        keep = ~zero
        far = 1e4 if CASES[name][5] == "far" else 1.0        # numpy.mean / numpy.cov lose those digits, not we
        assert np.max(np.abs(got["mean"] - x64.mean(axis=1))[keep] / sd[keep], initial=0) < 1e-14 * far
        cov = np.atleast_2d(np.cov(x64, ddof=ddof))
        scale = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))[np.ix_(keep, keep)]
        assert np.max(np.abs(got["cov"] - cov)[np.ix_(keep, keep)] / scale) < 1e-13 * far
        assert (got["cov"][zero] == 0).all() and (got["cov"][:, zero] == 0).all()
        with np.errstate(invalid="ignore", divide="ignore"):
            cc = np.atleast_2d(np.corrcoef(x64))
        assert np.max(np.abs(got["corr"] - cc)[np.ix_(keep, keep)]) < 1e-13 * far
        assert np.isnan(got["corr"][zero]).all() and np.isnan(got["corr"][:, zero]).all()
        od = ref.offdiag(got["corr"], dtype)
        kept = np.flatnonzero(keep)
        r = np.array([cc[i, j] for a, i in enumerate(kept) for j in kept[a + 1:]])
        assert od["pairs"] == len(r) == len(kept) * (len(kept) - 1) // 2
        if len(r):
            assert abs(od["mean"] - r.mean()) < 1e-13 * far and abs(od["mean_abs"] - np.abs(r).mean()) < 1e-13 * far
            assert abs(od["rms"] - np.sqrt((r * r).mean())) < 1e-13 * far and abs(od["sum_sq"] - (r * r).sum()) < 1e-11 * far
            i, j = od["argmax"]
            assert i < j and keep[i] and keep[j] and abs(od["max_abs"] - np.abs(r).max()) < 1e-13 * far
            assert od["max_abs"] == abs(got["corr"][i, j])
        else:
            assert od["argmax"] == (-1, -1) and np.isnan(od["rms"])


def test_restatement_breaks_a_tie_towards_the_first_pair():
    corr = np.eye(4)
    corr[0, 3] = corr[3, 0] = 0.5
    corr[1, 2] = corr[2, 1] = -0.5
    corr[0, 1] = corr[1, 0] = 0.25
    od = ref.offdiag(corr)
    assert od["argmax"] == (0, 3) and od["max_abs"] == 0.5 and od["pairs"] == 6
    corr[0, :] = corr[:, 0] = np.nan                       # variable 0 leaves: (1, 2) is what remains
    od = ref.offdiag(corr)
    assert od["argmax"] == (1, 2) and od["pairs"] == 3 and od["variables"] == 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_geometry_against_a_brute_force_enumeration(name):
    from bnn_priors_amd import weight_correlation as wc
    S, shape, var_dim, dtype, view = CASES[name][:5]
    base = _base(name)
    w = _apply_view(torch.from_numpy(np.array(base)), view)
    g = wc._geometry(w, var_dim)
    # the element offset of every (variable, observation), by numpy: number the allocation's elements and view them
    where = ref.as_matrix(_apply_view(np.arange(base.size, dtype=np.int64).reshape(base.shape), view), var_dim)
    assert (g.V, g.n) == where.shape
    sizes, strides = list(g.size), list(g.stride)
    assert int(np.prod(sizes)) == g.n and all(s >= 1 for s in sizes)
    idx = np.unravel_index(np.arange(g.n), sizes)
    offset = sum(i * s for i, s in zip(idx, strides))
    got = np.arange(g.V)[:, None] * g.v_stride + offset[None, :]
    assert np.array_equal(got, where)
    inner = [st for sz, st in zip(sizes, strides) if sz > 1][-1]
    assert g.v_major == int(g.V > 1 and g.v_stride < inner)
    assert w.storage_offset() == 0                          # (the view starts at the allocation's first element)


def test_geometry_merges_what_one_stride_walks_and_counts_the_rest():
    from bnn_priors_amd import weight_correlation as wc
    g = wc._geometry(torch.zeros(3, 4, 5, 6), 2)           # variables last: the other three axes are one walk
    assert (g.V, g.n, g.v_stride, g.v_major) == (6, 60, 1, 1) and list(g.size) == [1, 1, 1, 60] and g.stride[3] == 6
    g = wc._geometry(torch.zeros(3, 4, 5, 6), 0)           # variables first of the shape: S, then the trailing two
    assert (g.V, g.v_stride, g.v_major) == (4, 30, 0) and list(g.size) == [1, 1, 3, 30] and list(g.stride)[2:] == [120, 1]
    w = torch.zeros(4, 4, 4, 4, 4)[:, ::2, ::2, ::2, ::2]
    g = wc._geometry(w, 0)                                  # S and four sliced axes, of which one is V: four remain
    assert list(g.size) == [4, 2, 2, 2] and list(g.stride) == [256, 32, 8, 2] and g.v_stride == 128
    with pytest.raises(ValueError, match="at most 4"):
        wc._geometry(torch.zeros(4, 4, 4, 4, 4, 4)[:, ::2, ::2, ::2, ::2, ::2], 0)


def test_argument_checks():
    from bnn_priors_amd import weight_correlation as wc
    w = torch.zeros(6, 5, 4)
    for bad, match in ((torch.zeros(6, 5, dtype=torch.int64), "float32 or float64"), (torch.zeros(7), "float32 or float64"),
                       (torch.zeros(0, 3), "empty"), ([[1.0]], "float32 or float64")):
        with pytest.raises(ValueError, match=match):
            wc.covariance(bad, 0)
    for var_dim in (2, -3, 1.0, None, True):
        with pytest.raises(ValueError, match="var_dim"):
            wc.covariance(w, var_dim)
    with pytest.raises(ValueError, match="1 .. 1024"):
        wc.covariance(torch.zeros(2, 1025), 0)
    with pytest.raises(ValueError, match="2 .. 2147483647"):
        wc.covariance(torch.zeros(1, 3), 0)
    for ddof in (-1, 24, 1.0):
        with pytest.raises(ValueError, match="ddof"):
            wc.covariance(w, 0, ddof=ddof)
    with pytest.raises(ValueError, match="workspace_bytes = 199"):
        wc.covariance(w, 0, workspace_bytes=199)
    with pytest.raises(ValueError, match="workspace_bytes"):
        wc.covariance(w, 0, workspace_bytes=-1)
    with pytest.raises(ValueError, match="no CPU path"):
        wc.covariance(w, 0)
    with pytest.raises(ValueError, match="no CPU path"):
        wc.offdiag_stats(torch.eye(3, dtype=torch.float64))
    for bad in (torch.eye(3), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"\[V, V\]"):
            wc.offdiag_stats(bad)
    with pytest.raises(ValueError, match="1 .. 1024"):
        wc.offdiag_stats(torch.zeros(1025, 1025, dtype=torch.float64))
    for replicates in (0, 2 ** 24 + 1, 9.0):
        with pytest.raises(ValueError, match="replicates"):
            wc.independence_test(w, 0, replicates=replicates)
    with pytest.raises(ValueError, match="seed"):
        wc.independence_test(w, 0, seed=0.5)
    for perms in (torch.zeros(2, 5, 23, dtype=torch.int64), torch.zeros(2, 5, 24, dtype=torch.int32),
                  torch.zeros(5, 24, dtype=torch.int64), torch.zeros(0, 5, 24, dtype=torch.int64)):
        with pytest.raises(ValueError, match="perms must be"):
            wc.independence_test(w, 0, perms=perms)
    with pytest.raises(ValueError, match="no CPU path"):
        wc.independence_test(w, 0, perms=torch.zeros(2, 5, 24, dtype=torch.int64))
    with pytest.raises(ValueError, match="chains"):
        wc.layer_correlations({"a": torch.zeros(7, 2, 2)}, chains=2)
    with pytest.raises(ValueError, match="list of dicts"):
        wc.layer_correlations([])
    m, v, z = wc.schott(3.0, 28, 30)                        # plain numbers: V = 8, n = 30
    assert (m, v) == tuple(float(q) for q in ref.schott(8, 30)) and z == (3.0 - m) / v ** 0.5


def test_schott_moments_against_a_monte_carlo_of_gaussian_matrices():
    V, n, draws = 8, 30, 20000
    x = np.random.default_rng(5).standard_normal((draws, V, n))
    d = x - x.mean(axis=2, keepdims=True)
    G = d @ np.swapaxes(d, 1, 2)
    g = np.einsum("bii->bi", G)
    r2 = G * G / (g[:, :, None] * g[:, None, :])
    i, j = np.triu_indices(V, 1)
    t = r2[:, i, j].sum(axis=1)
    mean, var = (float(q) for q in ref.schott(V, n))
    se_mean = t.std(ddof=1) / np.sqrt(draws)
    m2, m4 = ((t - t.mean()) ** 2).mean(), ((t - t.mean()) ** 4).mean()
    se_var = np.sqrt((m4 - m2 * m2) / draws)
    print(t.mean(), mean, se_mean, t.var(ddof=1), var, se_var)
    assert abs(t.mean() - mean) < 4 * se_mean
    assert abs(t.var(ddof=1) - var) < 4 * se_var
    assert ref.schott(V, n, LD)[0].dtype == LD and abs(1 / np.sqrt(n - 1.0) - np.sqrt(r2[:, i, j].mean())) < 1e-3


def test_the_permutation_test_tells_independent_weights_from_a_shared_factor():
    x, xf, tables = _perm_data()
    assert x.dtype == np.float32 and tables.shape == (PERM_B, PERM_V, PERM_N)
    assert (np.sort(tables, axis=-1) == np.arange(PERM_N)).all()
    for wide in (False, True):
        ind, fac = _perm_ref(False, wide), _perm_ref(True, wide)
        print(ind["p_rms"], ind["p_max"], fac["p_rms"], fac["p_max"], ind["schott_z"], fac["schott_z"])
        assert 0.1 <= ind["p_rms"] <= 0.9
        assert fac["p_rms"] == 1 / (PERM_B + 1)
        for res in (ind, fac):                                 # no comparison >= can turn on rounding
            gap = np.abs(res["null"] - np.array([res["observed"]["rms"], res["observed"]["max_abs"]])).min(axis=0)
            print(gap)
            assert gap.min() > 1e-6
            # a permutation changes neither a mean nor a variance: the null's rms sits at the Gaussian reference
            assert abs(res["null"][:, 0].mean() / res["expected_rms"] - 1) < 0.05
        assert fac["schott_z"] > 10 > abs(ind["schott_z"]) and ind["observed"]["variables"] == PERM_V
    assert _perm_ref(False, False)["p_max"] == _perm_ref(False, True)["p_max"]


def test_the_recorded_deviations_are_the_measured_ones():
    got = _measure()
    print(got)
    for key, recorded in (("mean", MEAN_DEVIATION), ("cov", COV_DEVIATION), ("corr", CORR_DEVIATION),
                          ("stats", STAT_DEVIATION)):
        assert got[key] <= recorded <= max(2 * got[key], 2.0 ** -52 * 1.01), (key, got[key], recorded)
    for name in CASES:                                             # the integer outcomes do not depend on the precision
        a, b = _ref(name, False), _ref(name, True)
        assert a["nonfinite"] == b["nonfinite"] and np.array_equal(a["zero_variance"], b["zero_variance"])
        assert (a["offdiag"]["pairs"], a["offdiag"]["argmax"]) == (b["offdiag"]["pairs"], b["offdiag"]["argmax"])


# ------------------------------------------------------------------------------------------------------------------ GPU

def _bound(recorded):
    return 4 * max(recorded, 2.0 ** -53)        # a measured 0 leaves 4 roundings of the quantity: 2^-51


def _device_stack(name):
    return _apply_view(torch.from_numpy(np.array(_base(name))).cuda(), CASES[name][4])


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _offdiag_dict(od, r=0):
    out = {k: float(getattr(od, k)[r]) for k in STATS}
    out["pairs"], out["argmax"] = int(od.pairs[r]), tuple(int(q) for q in od.argmax[r])
    return out


def _kwargs(name):
    return {} if CASES[name][7] is None else dict(workspace_bytes=CASES[name][7])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_covariance_kernels_against_the_restatement(name):
    from bnn_priors_amd import weight_correlation as wc
    var_dim, ddof = CASES[name][2], CASES[name][6]
    w = _device_stack(name)
    assert w.is_contiguous() == (CASES[name][4] == "")
    c = wc.covariance(w, var_dim, ddof=ddof, **_kwargs(name))
    od = wc.offdiag_stats(c.corr)
    again = wc.covariance(w, var_dim, ddof=ddof, **_kwargs(name))
    for a, b in zip(list(c[1:]) + list(od), list(again[1:]) + list(wc.offdiag_stats(again.corr))):
        assert torch.equal(_bits(a), _bits(b))                     # two calls, the same bits
    wide = _ref(name, True)
    V = wide["mean"].shape[0]
    assert c.n == wide["n"] and isinstance(c.n, int) and int(c.nonfinite) == wide["nonfinite"]
    assert c.mean.shape == (V,) and c.cov.shape == c.corr.shape == (V, V) and c.zero_variance.dtype == torch.bool
    assert np.array_equal(c.zero_variance.cpu().numpy(), wide["zero_variance"])
    got = dict(mean=c.mean.cpu().numpy(), cov=c.cov.cpu().numpy(), corr=c.corr.cpu().numpy(), offdiag=_offdiag_dict(od))
    assert got["offdiag"]["pairs"] == wide["offdiag"]["pairs"] and got["offdiag"]["argmax"] == wide["offdiag"]["argmax"]
    if wide["nonfinite"]:
        assert all(np.isnan(got[k]).all() for k in ("mean", "cov", "corr"))
        assert all(np.isnan(got["offdiag"][k]) for k in STATS)
        return
    zero = wide["zero_variance"]
    assert np.array_equal(got["cov"], got["cov"].T) and np.array_equal(got["corr"], got["corr"].T, equal_nan=True)
    assert (got["cov"][zero] == 0).all() and np.isnan(got["corr"][zero]).all() and np.isnan(got["corr"][:, zero]).all()
    assert np.array_equal(got["mean"][zero], np.asarray(wide["mean"], np.float64)[zero])    # a constant: its own value
    if not wide["offdiag"]["pairs"]:
        assert all(np.isnan(got["offdiag"][k]) for k in STATS)
    dev = _deviations(got, wide)
    print(name, dev)
    assert dev["mean"] <= _bound(MEAN_DEVIATION) and dev["cov"] <= _bound(COV_DEVIATION)
    assert dev["corr"] <= _bound(CORR_DEVIATION) and dev["stats"] <= _bound(STAT_DEVIATION)


@pytest.mark.gpu
@pytest.mark.parametrize("name", VIEWS)
def test_a_view_and_its_contiguous_copy_give_the_same_bits(name):
    from bnn_priors_amd import weight_correlation as wc
    w = _device_stack(name)
    a = wc.covariance(w, CASES[name][2], **_kwargs(name))
    b = wc.covariance(w.contiguous(), CASES[name][2], **_kwargs(name))
    for p, q in zip(a[1:], b[1:]):
        assert torch.equal(_bits(p), _bits(q))


@pytest.mark.gpu
def test_offdiag_kernel_breaks_a_tie_towards_the_first_pair_and_takes_a_batch():
    from bnn_priors_amd import weight_correlation as wc
    V = 300                                                        # more columns than threads: the tie crosses threads
    corr = np.full((2, V, V), 0.125)
    corr[0, 1, 299] = corr[0, 299, 1] = -0.5
    corr[0, 2, 3] = corr[0, 3, 2] = 0.5
    corr[1, 5, 280] = corr[1, 280, 5] = 0.75
    corr[1, 4, :] = corr[1, :, 4] = np.nan
    corr[:, np.arange(V), np.arange(V)] = np.where(np.isnan(corr[:, np.arange(V), np.arange(V)]), np.nan, 1.0)
    od = wc.offdiag_stats(torch.from_numpy(corr).cuda())
    for r in range(2):
        want = ref.offdiag(corr[r], LD)
        got = _offdiag_dict(od, r)
        assert (got["pairs"], got["argmax"]) == (want["pairs"], want["argmax"])
        assert max(_rel(got[k], want[k]) for k in STATS) <= _bound(STAT_DEVIATION)
    assert _offdiag_dict(od, 0)["argmax"] == (1, 299) and _offdiag_dict(od, 1)["pairs"] == 299 * 298 // 2
    one = wc.offdiag_stats(torch.from_numpy(corr[1]).cuda())
    assert all(torch.equal(_bits(a[1:]), _bits(b)) for a, b in zip(od, one))


@pytest.mark.gpu
def test_a_batch_of_three_equals_three_single_calls_bit_for_bit():
    from bnn_priors_amd import weight_correlation as wc
    name = "v65_three_splits"
    w = _device_stack(name)
    V, n = 65, w.shape[0]
    rng = np.random.default_rng(11)
    tables = torch.from_numpy(np.stack([np.stack([rng.permutation(n) for _ in range(V)]) for _ in range(3)])).cuda()
    batch = wc.independence_test(w, 0, perms=tables, **_kwargs(name))
    singles = [wc.independence_test(w, 0, perms=tables[b:b + 1], **_kwargs(name)) for b in range(3)]
    assert torch.equal(_bits(batch.null), _bits(torch.cat([s.null for s in singles])))
    # ... and the matrices themselves: the Gram entry point on [3, V, n] and on each gathered copy, with the data's means
    g = wc._geometry(w, 0)
    sp = wc.splits(V, n, CASES[name][7])
    mean, bad = wc._mean(w, g)
    x = w.movedim(1, 0).reshape(V, n).contiguous()
    xp = torch.gather(x.unsqueeze(0).expand(3, V, n), 2, tables)
    gc = wc._contiguous_geometry(V, n)
    _, corr3, zero3 = wc._gram(xp, gc, 3, V * n, mean, bad, sp, 1, False)
    for b in range(3):
        cov1, corr1, zero1 = wc._gram(xp[b].clone(), gc, 1, 0, mean, bad, sp, 1, True)
        assert torch.equal(_bits(corr3[b]), _bits(corr1[0])) and torch.equal(zero3[b], zero1[0])
        want = ref.covariance(x.cpu().numpy(), 1, LD, m=mean.cpu().numpy(), order=tables[b].cpu().numpy())
        assert np.max(np.abs(LD(1) * corr1[0].cpu().numpy() - want["corr"])) <= _bound(CORR_DEVIATION)


@pytest.mark.gpu
@pytest.mark.parametrize("factor", (False, True))
def test_independence_test_with_given_tables_against_the_restatement(factor):
    from bnn_priors_amd import weight_correlation as wc
    data = _perm_data()
    w = torch.from_numpy(np.ascontiguousarray(data[1 if factor else 0].T)).cuda()      # [S = n, V]: observation k = s
    t = wc.independence_test(w, 0, perms=torch.from_numpy(data[2]).cuda())
    wide = _perm_ref(factor, True)
    assert (t.n, t.V) == (PERM_N, PERM_V) and t.null.shape == (PERM_B, 2)
    assert float(t.p_rms) == wide["p_rms"] and float(t.p_max) == wide["p_max"]
    assert np.max(np.abs(LD(1) * t.null.cpu().numpy() - wide["null"]) / wide["null"]) <= _bound(STAT_DEVIATION)
    got = _offdiag_dict(t.observed)
    assert (got["pairs"], got["argmax"]) == (wide["observed"]["pairs"], wide["observed"]["argmax"])
    assert max(_rel(got[k], wide["observed"][k]) for k in ("rms", "max_abs", "sum_sq")) <= _bound(STAT_DEVIATION)
    assert _rel(t.expected_rms, wide["expected_rms"]) <= 2.0 ** -52
    for k in ("schott_mean", "schott_var", "schott_z"):
        assert _rel(float(getattr(t, k)), wide[k]) <= 8 * _bound(STAT_DEVIATION)       # (a few operations on sum r^2)


@pytest.mark.gpu
def test_independence_test_by_seed():
    from bnn_priors_amd import weight_correlation as wc
    x, xf, _ = _perm_data()
    ind, fac = (torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (x, xf))
    a = wc.independence_test(ind, 0, replicates=PERM_B, seed=3)
    b = wc.independence_test(ind, 0, replicates=PERM_B, seed=3)
    assert torch.equal(_bits(a.null), _bits(b.null)) and torch.equal(_bits(a.p_rms), _bits(b.p_rms))
    assert not torch.equal(_bits(a.null), _bits(wc.independence_test(ind, 0, replicates=PERM_B, seed=4).null))
    assert abs(float(a.null[:, 0].mean()) * np.sqrt(PERM_N - 1.0) - 1) < 0.05
    f = wc.independence_test(fac, 0, replicates=PERM_B, seed=3)
    assert float(f.p_rms) == 1 / (PERM_B + 1)
    small = wc.independence_test(ind, 0, replicates=7, seed=3, workspace_bytes=1 << 16)     # one replicate per launch
    assert small.null.shape == (7, 2) and torch.isfinite(small.null).all()


@pytest.mark.gpu
def test_layer_correlations_equal_the_per_tensor_calls():
    from bnn_priors_amd import weight_correlation as wc
    rng = np.random.default_rng(21)
    samples = {"fc.weight": torch.from_numpy(rng.standard_normal((12, 6, 10)).astype(np.float32)),
               "conv.weight": torch.from_numpy(rng.standard_normal((12, 4, 1, 3, 3))),
               "fc.bias": torch.from_numpy(rng.standard_normal((12, 6))),
               "bn.num_batches_tracked": torch.zeros(12, 1, 1), "steps": torch.arange(12)}
    out = wc.layer_correlations(samples, chains=3, replicates=9, seed=2)
    assert sorted(out.layers) == [("conv.weight", 0), ("fc.weight", 0), ("fc.weight", 1)]
    assert [(n, a) for n, a, _ in out.skipped] == [("conv.weight", 1)] and "V = 1" in out.skipped[0][2]
    for (name, axis), got in out.layers.items():
        want = wc.independence_test(samples[name].cuda(), axis, replicates=9, seed=2)
        assert (got.n, got.V) == (want.n, want.V) == (samples[name].numel() // samples[name].shape[1 + axis],
                                                      samples[name].shape[1 + axis])
        tensors = lambda t: list(t.observed) + list(t[3:6]) + list(t[7:])     # (all but n, V and the float expected_rms)
        for p, q in zip(tensors(got), tensors(want)):
            assert torch.equal(_bits(p), _bits(q))
    chains = [{k: v[i::3] for k, v in samples.items()} for i in range(3)]
    assert sorted(wc.layer_correlations(chains, replicates=3).layers) == sorted(out.layers)


@pytest.mark.gpu
def test_the_gram_walk_reproduces_the_recorded_bits():
    """sha256 of mean, cov, corr, zero_variance, nonfinite and the off-diagonal statistics of every case of
    tests/golden/make_gram_bits.py, and of its batched permutation cases, against tests/golden/gram_bits.json -- recorded
    with the library of the commit before the two Gram passes came to share csrc/gram_hip.inc.  The library is built with
    -ffp-contract=off: the same operations in the same order are the same bits."""
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
    want, got = recorded["corr"], bits.corr_digests()
    assert sorted(got) == sorted(want) and len(got) == len(bits.corr_cases()) + 3
    for name in sorted(got):
        assert sorted(got[name]) == sorted(want[name])
        for array in got[name]:
            assert got[name][array] == want[name][array], (
                f"case {name}: {array} differs from the recording (recorded under {recorded['versions']}, running "
                f"{bits.versions()})")
