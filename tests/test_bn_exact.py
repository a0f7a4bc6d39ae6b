"""The BatchNorm kernels (csrc/bn_hip.inc) at every walk geometry ``bn::geo`` can choose, on inputs where their results
are owed exactly (tests/bn_reference.py).

The kernels pick an element walk, a slice layout and a prologue from (N, C, P, G) at run time; tests/test_bn.py runs the
trunk's geometries only, under tolerances that a lost element passes (``test_one_dropped_element_...`` below shows it on
the references).  Here every class of geometry (``bn_reference.classify``, held complete by
``test_cases_cover_every_walk_class``) runs on

* integer inputs: every fp32 per-thread sum of the statistics kernel is an integer below 2^24, the fp64 block and channel
  sums are exact, so the logged mean is ONE correctly rounded division of an exact sum: bit-equal to the reference;
* two-valued inputs (x = +-2^k, half of each sign per channel): mean 0 and invstd 2^-k exactly, xhat = +-1, and y, the
  ReLU mask, d_residual, dbeta and dgamma are fp32 numbers: ``assert_exact``, outputs prefilled with NaN;
* random inputs, under the tolerances of tests/test_bn.py.

Every tolerance below names where it comes from."""
import contextlib
import ctypes
import types
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_reference as R
from bnn_priors_amd import _hip, bn, bnlink
from exact_inputs import NAN, assert_budget, assert_exact, ints

GPU = pytest.mark.gpu
CASES = pytest.mark.parametrize("case", R.TABLE, ids=R.case_id)
VARIANTS = [(True, False), (True, True), (False, False), (False, True)]            # (relu, residual)
EPS = 1e-5
# fp64 sums that differ only in the order of summation: the project's bar (docstring of tests/test_hip_parity.py)
REL64 = 1e-12

# the classes the table must keep: ``bn_reference.fingerprint`` of its cases.  A case may be replaced by one with the same
# fingerprint, not dropped.
REQUIRED = [
    ('V==kT', 1, 8, 8, 'all', 'xcd', False, False, False, False, False),
    ('V==kT', 1, 7, 6, 'none', 'plain', True, False, False, False, False),
    ('V==kT', 1, 9, 8, 'some', 'plain', True, False, False, False, False),
    ('V==kT', 1, 8, 8, 'all', 'plain', False, True, False, False, False),
    ('V==kT', 1, 3, 2, 'none', 'plain', True, False, False, False, False),
    ('V==kT', 1, 3, 2, 'none', 'xcd', True, False, False, False, False),
    ('V<kT', 1, 6, 5, 'none', 'plain', False, True, False, False, True),
    ('V<kT,idle', 1, 5, 4, 'none', 'plain', False, True, False, False, True),
    ('V>kT', 4, 0, 0, 'none', 'plain', False, False, False, False, False),
    ('V>kT,tail', 2, 0, 0, 'none', 'plain', False, False, False, False, False),
    ('V>kT,tail', 2, 0, 0, 'none', 'plain', False, False, False, True, False),
    ('V<kT', 1, 1, 0, 'none', 'plain', False, False, False, False, False),
    ('V<kT', 1, 1, 0, 'none', 'plain', False, True, False, False, False),
    ('V<kT', 1, 1, 0, 'none', 'plain', False, False, True, False, False),
    ('V<kT', 1, 1, 0, 'none', 'plain', False, True, False, False, True),
    ('V==kT', 1, 2, 2, 'none', 'xcd', False, False, False, True, False),
    ('V==kT', 1, 1, 1, 'none', 'xcd', False, False, False, True, False),
    ('V==kT', 1, 1, 1, 'none', 'plain', False, False, False, True, False),
    ('V<kT', 1, 1, 0, 'none', 'plain', True, False, False, True, False),
    ('V<kT', 1, 1, 0, 'none', 'xcd', True, False, False, True, False),
    ('V==kT', 1, 4, 4, 'all', 'xcd', False, False, False, False, False),
    ('V<kT', 1, 2, 2, 'none', 'xcd', False, False, False, False, False),
    ('V<kT', 1, 1, 1, 'none', 'xcd', False, False, False, False, False),
]

# caller-supplied partials (``stats=``): (n, C, H, W, G, parts per group) -- one trunk shape and one V > kT shape at 1, 7,
# 512, 513 and 1030 parts (apply_kernel keeps two pairs per thread: 512; its loop beyond them starts at 513), and grouped
STATS_CASES = [(128, 64, 8, 8, 1, 1), (112, 64, 8, 8, 1, 7), (128, 64, 8, 8, 1, 512), (513, 64, 8, 8, 1, 513),
               (515, 64, 8, 8, 1, 1030), (224, 64, 8, 8, 2, 7), (1026, 64, 8, 8, 2, 513),
               (3, 2, 64, 64, 1, 1), (7, 2, 64, 64, 1, 7), (3, 2, 64, 64, 1, 512), (513, 2, 64, 64, 1, 513),
               (515, 2, 64, 64, 1, 1030), (14, 2, 64, 64, 2, 7)]
STATS_IDS = [R.case_id(c[:5]) + f"-parts{c[5]}" for c in STATS_CASES]


def _dims(case):
    n, C, H, W, G = case
    return n, C, H * W, G, R.geo(n, C, H * W, G)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the premise, on the CPU

def test_cases_cover_every_walk_class():
    "the table reaches every class the classifier can return, and keeps every fingerprint it was built with"
    seen = set()
    for case in R.TABLE:
        n, C, P, G, g = _dims(case)
        assert g is not None and n * C * P * 4 <= 36e6, case              # (a case stays below about 35 MB per tensor)
        seen |= R.tags(R.classify(n, C, P, G))
    assert seen == R.ALL_TAGS, (sorted(R.ALL_TAGS - seen), sorted(seen - R.ALL_TAGS))
    prints = {R.fingerprint(c) for c in R.TABLE}
    missing = [f for f in REQUIRED if f not in prints]
    assert not missing, missing
    assert prints == set(REQUIRED), sorted(prints - set(REQUIRED))        # (a new class is recorded when it is added)


@CASES
def test_integer_inputs_meet_the_budget_and_the_slice_then_chan_order_stays_inside_the_bar(case):
    """Integer inputs: the budget (per slice, sum |x - K| and sum (x - K)^2 within 2^24) holds, so the statistics kernel's
    partial sums are exact; a float64 NumPy restatement of its slice-then-Chan order then gives the exact mean BIT FOR BIT
    and an unbiased variance within 1e-12 relative of the exact rational's rounding -- worst ratio over the table
    4.5e-16, a margin of 2000 under the bar the GPU test applies (asserted here with a margin of 100)."""
    n, C, P, G, g = _dims(case)
    x = R.int_input(case)
    assert x.abs().max() <= 8
    mean, _, var_u = R.exact_stats(x, G)
    assert bool((var_u > 0).all())
    m, _, u = R.chan_order(x, g)                                       # (asserts the budget)
    assert np.array_equal(m, mean.numpy())
    assert np.abs(u / var_u.numpy() - 1).max() <= REL64 / 100


@pytest.mark.parametrize("sc", STATS_CASES, ids=STATS_IDS)
def test_caller_supplied_partials_stay_inside_the_bar(sc):
    "the same for equal-part partials computed by the caller in float64 (worst ratio 3.4e-16)"
    *case, parts = sc
    n, C, P, G, g = _dims(case)
    x = R.int_input(tuple(case))
    mean, _, var_u = R.exact_stats(x, G)
    p = R.equal_parts(x, G, parts).view(C, G, parts, 2).permute(1, 0, 2, 3).numpy()
    M = float(g.N * P)
    m, _, u = R.chan_from_partials(p[..., 0], p[..., 1], M / parts, M)
    assert np.array_equal(m, mean.numpy())
    assert np.abs(u / var_u.numpy() - 1).max() <= REL64 / 100


@CASES
def test_two_valued_inputs_make_forward_and_backward_exact(case):
    """Two-valued inputs: in a float64 evaluation the mean is 0, the variance 4^k, y / dz / dbeta / dgamma are fp32 numbers
    within the budget (``two_valued_ref`` asserts it); the kernel's own variance order rounds to invstd = 2^-k exactly; the
    fp32 restatement of apply_kernel's expression IS the float64 y, and that of bwd_dx_body's stays within HALF of the
    bound the GPU test applies: of the 9 roundings the bound counts, only four act here (mdb, mdg, d - mdb, the second
    subtraction; the others are by powers of two or of exact values), each at most 2^-24 of a partial result that
    |d| + |mdb| + |mdg| bounds (measured worst: 0.22 of the bound)."""
    n, C, P, G, g = _dims(case)
    d = R.two_valued(case)
    M = d["M"]
    # the variance in the kernel's order, on x * 4 (integers; a power of two commutes with every operation)
    _, var, _ = R.chan_order(d["x"] * 4, g)
    want = np.exp2(-d["k"].numpy().astype(np.float64))
    assert np.array_equal((1.0 / np.sqrt(var / 16)).astype(np.float32), np.broadcast_to(want.astype(np.float32), var.shape))
    cv = lambda t: t.numpy()[None, None, :, None]
    x = R.grouped_view(d["x"], G).numpy()
    invstd = want.astype(np.float32)[None, None, :, None]
    for relu, residual in VARIANTS:
        ref = R.two_valued_ref(d, relu, residual)
        y32 = R.apply32(x, 0.0, invstd * cv(d["gamma"]), cv(d["beta"]),
                        R.grouped_view(d["res"], G).numpy() if residual else None, relu)
        assert np.array_equal(y32.astype(np.float64), R.grouped_view(ref["y"], G).numpy()), (relu, residual)
        if residual:
            continue                                 # (the residual reaches dx through the mask alone)
        dx32 = R.bwd_dx32(R.grouped_view(ref["dz"], G).numpy(), x, 0.0, invstd, cv(d["gamma"]),
                          ref["dbeta"].numpy()[:, None, :, None], ref["dgamma"].numpy()[:, None, :, None], M)
        err = np.abs(dx32.astype(np.float64) - R.grouped_view(ref["dx"], G).numpy())
        assert (err <= 0.5 * R.grouped_view(ref["bound"], G).numpy()).all(), (relu, err.max())


def test_one_dropped_element_passes_the_old_bounds_and_fails_the_new():
    """What the tolerances of test_bn.py::test_fused_bn_matches_aten cannot see, on the REFERENCES of (128, 16, 32, 32)
    alone (no kernel involved): one plane element left out of a channel's sums.

    Statistics (integer inputs, an element of value +-1 dropped): running_mean and running_var after a momentum-0.1
    update stay within that test's (rtol 1e-6, atol 1e-6) and (rtol 1e-5, atol 1e-6); the new comparisons -- logged mean
    bit-equal, logged variance to 1e-12, running statistics to one fp32 ulp -- all reject it.  (An element of magnitude
    above about 1.6 moves running_mean past the old bar: it sees the larger elements only.)

    Backward sums (that test's own random inputs): the old (rtol 1e-4, atol 3e-5 sqrt(M) = 0.011) passes every dropped
    element with |dz| and |dz xhat| below it, here 2.8 % of the elements (asserted above 0.5 %); on the two-valued
    inputs ANY dropped element with dz != 0 moves dbeta and dgamma by at least 1, which ``assert_exact`` rejects."""
    case = (128, 16, 32, 32, 1)
    n, C, P, G, g = _dims(case)
    M = n * P
    x = R.int_input(case)
    mean, _, var_u = R.exact_stats(x, 1)
    ch = x[:, 0].flatten().long()
    i = int((ch.abs() == 1).nonzero()[0])
    s, q = int(ch.sum() - ch[i]), int((ch * ch).sum() - ch[i] * ch[i])
    mean_d = float(s) / float(M)                                         # the kernel's M is the launch's: unchanged
    var_d = float(Fraction(M * q - s * s, M) / (M - 1))
    m0, v0 = mean[0, 0].item(), var_u[0, 0].item()
    rm0, rv0, mom = np.float32(0.3), np.float32(0.8), 0.1
    upd = lambda old, new: torch.tensor(np.float32((1 - mom) * float(old) + mom * new)).double()
    torch.testing.assert_close(upd(rm0, mean_d), upd(rm0, m0), rtol=1e-6, atol=1e-6)          # the old bars: blind
    torch.testing.assert_close(upd(rv0, var_d), upd(rv0, v0), rtol=1e-5, atol=1e-6)
    assert mean_d != m0 and abs(var_d / v0 - 1) > REL64                                       # the new ones: not
    assert abs(upd(rm0, mean_d) - upd(rm0, m0)) > R.ulp32(upd(rm0, m0))
    assert abs(upd(rv0, var_d) - upd(rv0, v0)) > R.ulp32(upd(rv0, v0))

    gen = torch.Generator().manual_seed(n * 1000 + C)                    # test_fused_bn_matches_aten's inputs
    xr = (torch.randn(n, C, 32, 32, generator=gen) * 1.7 + 0.4).double()
    torch.rand(C, generator=gen), torch.randn(C, generator=gen)          # (its weight and bias)
    dz = torch.randn(n, C, 32, 32, generator=gen).double()
    xhat = (xr - xr.mean((0, 2, 3), keepdim=True)) / (xr.var((0, 2, 3), unbiased=False, keepdim=True) + EPS).sqrt()
    dbeta, dgamma = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
    atol, rtol = 3e-5 * M ** .5, 1e-4
    tb, tg = (atol + rtol * dbeta.abs())[None, :, None, None], (atol + rtol * dgamma.abs())[None, :, None, None]
    slips = (dz.abs() <= tb) & ((dz * xhat).abs() <= tg)
    assert slips.double().mean() > 0.005
    worst = (dz.abs() * slips).flatten().argmax()
    c = (worst // 1024) % C
    for total, term in ((dbeta, dz), (dgamma, dz * xhat)):
        dropped = total.clone()
        dropped[c] -= term.flatten()[worst]
        torch.testing.assert_close(dropped, total, rtol=rtol, atol=atol)                      # the old bar: blind
    d = R.two_valued(case)
    ref = R.two_valued_ref(d, True, True)
    j = int((ref["dz"][:, 0] != 0).flatten().nonzero()[0])
    for key, term in (("dbeta", ref["dz"][:, 0].flatten()[j]),
                      ("dgamma", (ref["dz"][:, 0] * ref["xhat"][0, :, 0].reshape(n, 32, 32)).flatten()[j])):
        dropped = ref[key].clone()
        dropped[0, 0] -= term
        with pytest.raises(AssertionError):
            assert_exact(dropped, ref[key], key)


# ---------------------------------------------------------------------------------------------------------------------
# GPU plumbing

def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _no_nan(**tensors):
    for k, t in tensors.items():
        assert not torch.isnan(t).any(), f"{k}: {int(torch.isnan(t).sum())} elements were never written"


def _within_ulp(got, ref64, what):
    "``got`` (fp32) within one fp32 ulp of the float rounding of ``ref64``"
    r32 = np.asarray(ref64, np.float64).astype(np.float32)
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - r32.astype(np.float64))
    bad = err > R.ulp32(r32)
    assert not bad.any(), f"{what}: {int(bad.sum())} beyond one ulp, worst {(err / R.ulp32(r32)).max():.2f} ulp"


def _logged_forward(x, G, stats_in):
    "one logged training forward with weight 1, bias 0 -> (log [G, C, 2], saved [2, G, C]); the running statistics stay"
    C = x.shape[1]
    w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    rm, rv = torch.full((C,), -77.0, device="cuda"), torch.full((C,), -78.0, device="cuda")
    slot = _nan(G, C, 2, dtype=torch.float64)
    with torch.no_grad(), bn.logging_running_stats({id(rm): slot if G > 1 else slot[0]}), bn.grouped(G):
        y, saved = bn._BNTrain.apply(x, w, b, None, rm, rv, 0.1, EPS, False, stats_in)
    assert bool((rm == -77).all()) and bool((rv == -78).all())
    _no_nan(y=y, saved=saved, log=slot)
    return slot.cpu(), saved.view(2, G, C).cpu()


def _check_stats(x, G, log, saved):
    "the logged and the saved statistics of integer ``x`` against the exact ones"
    mean, var_b, var_u = R.exact_stats(x, G)
    assert_exact(log[..., 0], mean, "logged mean (one correctly rounded division of an exact sum)")
    rel = (log[..., 1] / var_u - 1).abs().max().item()
    assert rel <= REL64, f"logged unbiased variance: {rel:.3g} relative"
    assert_exact(saved[0], mean.float().double(), "save_mean")
    _within_ulp(saved[1], 1.0 / np.sqrt(var_b.numpy() + EPS), "save_invstd")
    return mean, var_u


# ---------------------------------------------------------------------------------------------------------------------
# 2. statistics at fp64

@GPU
def test_scratch_size_is_the_restated_geometry():
    "``bn_reference.geo`` IS ``bn::geo``: S through sgmcmc_bn_scratch_doubles, for every case of every table"
    for case in R.TABLE + [tuple(c[:5]) for c in STATS_CASES]:
        n, C, P, G, g = _dims(case)
        assert _hip.lib().sgmcmc_bn_scratch_doubles(n, C, P, G) == C * G * g.S * 2, case
    assert _hip.lib().sgmcmc_bn_scratch_doubles(6, 4, 6, 1) == -1 and R.geo(6, 4, 6) is None


@GPU
@CASES
def test_statistics_are_exact_at_fp64(case):
    """Integer inputs through the layer's own statistics pass: logged mean bit-equal, logged unbiased variance to 1e-12
    (the CPU restatement of the kernel's order stays 2000 times inside: 4.5e-16), save_mean the float rounding of the
    mean, save_invstd and -- without logging, momentum 0.1 and 1 -- the running statistics within one fp32 ulp of the
    float rounding of the float64 expression (one ulp: the kernel's float64 operand differs from the reference's in its
    last bits, which can move the ONE rounding to float across a tie, no further)."""
    n, C, P, G, g = _dims(case)
    x = R.int_input(case)
    R.stats_budget(x, g)                                    # exactness is owed: asserted on these inputs
    xc = x.cuda()
    mean, var_u = _check_stats(x, G, *_logged_forward(xc, G, None))
    if G > 1:
        return                                              # (groups advance running statistics through the log only)
    w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    rm0, rv0 = ints((C,), -5, 5, C).cuda() / 4, ints((C,), 1, 9, C + 1).cuda() / 8
    for mom in (0.1, 1.0):
        rm, rv = rm0.clone(), rv0.clone()
        with torch.no_grad():
            bn.bn_train(xc, w, b, rm, rv, mom, EPS)
        _within_ulp(rm, (1 - mom) * rm0.double().cpu().numpy() + mom * mean[0].numpy(), f"running_mean, momentum {mom}")
        _within_ulp(rv, (1 - mom) * rv0.double().cpu().numpy() + mom * var_u[0].numpy(), f"running_var, momentum {mom}")


@GPU
@pytest.mark.parametrize("sc", STATS_CASES, ids=STATS_IDS)
def test_statistics_from_caller_supplied_partials_are_exact_at_fp64(sc):
    "``stats=``: equal-part partials computed here in float64 (sums exact: ``equal_parts`` asserts it); the same bars"
    *case, parts = sc
    n, C, P, G, g = _dims(case)
    x = R.int_input(tuple(case))
    stats = R.equal_parts(x, G, parts).cuda()
    _check_stats(x, G, *_logged_forward(x.cuda(), G, stats))


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact forward and backward

def _two_valued_on_device(case):
    d = R.two_valued(case)
    return d, {k: d[k].cuda() for k in ("x", "gamma", "beta", "res", "dy")}


@GPU
@CASES
def test_forward_and_backward_are_exact_on_two_valued_inputs(case):
    """sgmcmc_bn_train_fwd + sgmcmc_bn_train_bwd through the C ABI, every output prefilled with NaN, relu x residual:
    save_mean = 0, save_invstd = 2^-k, y, d_residual, dbeta, dgamma equal the float64 evaluation exactly (the budget:
    ``two_valued_ref``), no NaN is left, and dx is within (9 roundings, counted at ``bn_reference.DX_ROUNDINGS``) x 2^-24 x
    |k| (|d| + |mdb| + |mdg|) of the float64 formula (the fp32 restatement stays within half of it on the CPU)."""
    lib = _hip.lib()
    n, C, P, G, g = _dims(case)
    d, t = _two_valued_on_device(case)
    invstd_want = torch.exp2(-d["k"].double()).repeat(G)
    n_scratch = lib.sgmcmc_bn_scratch_doubles(n, C, P, G)
    for relu, residual in VARIANTS:
        what = f"relu={relu}, residual={residual}: "
        ref = R.two_valued_ref(d, relu, residual)
        y, mean, invstd = _nan(*t["x"].shape), _nan(G * C), _nan(G * C)
        scratch = _nan(n_scratch, dtype=torch.float64)
        err = lib.sgmcmc_bn_train_fwd(t["x"].data_ptr(), t["res"].data_ptr() if residual else 0, t["gamma"].data_ptr(),
                                      t["beta"].data_ptr(), 0, 0, 0.1, 0.0, int(relu), n, C, P, y.data_ptr(),
                                      mean.data_ptr(), invstd.data_ptr(), scratch.data_ptr(), 0, 0, G, _stream())
        _hip.check(err, "sgmcmc_bn_train_fwd")
        assert_exact(mean, torch.zeros(G * C, dtype=torch.float64), what + "save_mean")
        assert_exact(invstd, invstd_want, what + "save_invstd")
        assert_exact(y, ref["y"], what + "y")
        _no_nan(scratch=scratch)
        dx, dres, dgb = _nan(*t["x"].shape), _nan(*t["x"].shape) if residual else None, _nan(G, 2, C)
        scratch = _nan(n_scratch, dtype=torch.float64)
        err = lib.sgmcmc_bn_train_bwd(t["dy"].data_ptr(), y.data_ptr(), t["x"].data_ptr(), t["gamma"].data_ptr(),
                                      mean.data_ptr(), invstd.data_ptr(), int(relu), n, C, P, dx.data_ptr(),
                                      dres.data_ptr() if residual else 0, dgb.data_ptr(), scratch.data_ptr(), G, _stream())
        _hip.check(err, "sgmcmc_bn_train_bwd")
        if residual:
            assert_exact(dres, ref["dz"], what + "d_residual")
        assert_exact(dgb[:, 0], ref["dgamma"], what + "dgamma")
        assert_exact(dgb[:, 1], ref["dbeta"], what + "dbeta")
        _no_nan(dx=dx, scratch=scratch)
        over = (dx.double().cpu() - ref["dx"]).abs() - ref["bound"]
        assert over.max() <= 0, what + f"dx: {int((over > 0).sum())} elements beyond the bound, worst by {over.max():.3g}"


ROUTE_CASES = [(256, 16, 32, 32, 1), (17, 256, 32, 32, 1), (3, 8, 64, 64, 1), (80, 16, 32, 32, 1), (11, 600, 16, 32, 1),
               (18, 8, 40, 40, 2), (46, 64, 8, 8, 2)]


@GPU
@pytest.mark.parametrize("case", ROUTE_CASES, ids=R.case_id)
def test_backward_through_the_separate_sums_and_dx_launches_is_exact(case):
    """The other backward route, through autograd: out = bn_train(x, relu=True, residual=bn_train(r_in)) runs
    sgmcmc_bn_bwd_sums, then sgmcmc_bn_bwd_dx with the shortcut BatchNorm's sums riding along, then the shortcut's dx
    launch on those sums (off the trunk: count > 4, V > kT, ragged slices, groups).  Both layers two-valued: the outputs,
    dz and all four parameter gradients equal float64 exactly, both input gradients are within the counted bound."""
    n, C, P, G, g = _dims(case)
    d, t = _two_valued_on_device(case)
    M = d["M"]
    # the shortcut's input: x with every plane rolled and negated (still half of each sign per group and channel)
    r_in = -torch.roll(d["x"], 1, dims=3)
    gs, bs = d["gamma"].flip(0) * 2, ints((C,), -2, 2, C + 9, nonzero=False)
    cv = lambda v: v.double()[None, None, :, None]
    pw = cv(torch.exp2(-d["k"].double()))
    xhat_r = R.grouped_view(r_in, G).double() * pw
    s64 = (cv(gs) * xhat_r + cv(bs)).reshape(d["x"].shape)
    assert torch.equal(s64.float().double(), s64)
    ref = R.two_valued_ref(d, True, True, res=s64.float())
    rdb, rdg, rdx, rbound = R.bwd64(R.grouped_view(ref["dz"], G), xhat_r, cv(gs) * pw, M)
    assert_budget(ref["dz"].abs().sum((0, 2, 3)))             # the groups' integer sums added: still within 2^24

    leaves = [v.clone().requires_grad_() for v in (t["x"], t["gamma"], t["beta"], r_in.cuda(), gs.cuda(), bs.cuda())]
    before = dict(bnlink.STATS)
    with bn.grouped(G):
        s = bn.bn_train(leaves[3], leaves[4], leaves[5], None, None, 0.1, 0.0)
        out = bn.bn_train(leaves[0], leaves[1], leaves[2], None, None, 0.1, 0.0, residual=s, relu=True)
        out.backward(t["dy"])
    # the route: the outer backward launched its own sums, the shortcut found its sums on the gradient it was handed
    assert (bnlink.STATS["own"] - before["own"], bnlink.STATS["upstream"] - before["upstream"]) == (1, 1)
    assert_exact(s, s64, "shortcut BatchNorm output")
    assert_exact(out, ref["y"], "out")
    for leaf, want, name in ((leaves[1], ref["dgamma"].sum(0), "dgamma"), (leaves[2], ref["dbeta"].sum(0), "dbeta"),
                             (leaves[4], rdg.sum(0), "shortcut dgamma"), (leaves[5], rdb.sum(0), "shortcut dbeta")):
        assert_exact(leaf.grad, want, name)
    for leaf, want, bound, name in ((leaves[0], ref["dx"], ref["bound"], "dx"),
                                    (leaves[3], rdx.reshape(d["x"].shape), rbound.reshape(d["x"].shape), "shortcut dx")):
        over = (leaf.grad.double().cpu() - want).abs() - bound
        assert over.max() <= 0, f"{name}: {int((over > 0).sum())} elements beyond the bound, worst by {over.max():.3g}"


# ---------------------------------------------------------------------------------------------------------------------
# 4. random inputs against float64 across the table

def _slice_sums(t, g):
    "[G, N, C, P] -> float64 sums per (channel, group, slice): the layout of the kernels' partials"
    out = [t[:, s * g.NB:min(g.N, (s + 1) * g.NB)].sum((1, 3), dtype=torch.float64) for s in range(g.S)]
    return torch.stack(out, -1).permute(1, 0, 2)


@GPU
@CASES
def test_random_inputs_match_float64_across_the_table(case):
    """tests/test_bn.py::test_fused_bn_matches_aten's comparison (its tolerances, its ReLU-flip allowance, its repeat for
    identical bits) at every table case, relu x residual, groups in log mode against float64 on each group alone.

    With ReLU the backward partials are also read (sgmcmc_bn_bwd_sums):
    * each slice's pair is within (float4 per thread + 2) x 2^-24 x sum |terms| of the float64 sum of the kernel's own fp32
      terms d and d * ((x - mean) * invstd) -- counted: a term passes through two additions inside its float4 and at most
      one per float4 of the thread's running fp32 sum; everything after is float64;
    * dgamma / dbeta from sgmcmc_bn_bwd_dx are the float roundings of the partials' float64 sums to 1e-12 relative
      (order of summation only: the bar of tests/test_hip_parity.py), and its dx has the bits of the autograd route."""
    lib = _hip.lib()
    n, C, P, G, g = _dims(case)
    H, W = case[2], case[3]
    N, M = g.N, g.N * P
    gen = torch.Generator().manual_seed(n * 1000 + C)
    x = (torch.randn(n, C, H, W, generator=gen) * 1.7 + 0.4).cuda()
    x[N:] += 0.8                                               # (the groups' statistics differ)
    res_all = torch.randn(n, C, H, W, generator=gen).cuda()
    w, b = (torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda()
    dy = torch.randn(n, C, H, W, generator=gen).cuda()
    rm0, rv0 = torch.randn(C, generator=gen).cuda(), (torch.rand(C, generator=gen) + 0.5).cuda()
    per_thread = max([c for k in R.slice_images(g) for c in R.thread_counts(g, k)],
                     default=((P // 4 + R.kT - 1) // R.kT) * g.NB)

    def run(res):
        leaves = [v.clone().requires_grad_() for v in (x, w, b)] + ([res.clone().requires_grad_()] if res is not None else [])
        rm, rv = rm0.clone(), rv0.clone()
        slot = torch.zeros((G, C, 2), dtype=torch.float64, device="cuda")
        log = bn.logging_running_stats({id(rm): slot}) if G > 1 else contextlib.nullcontext()
        with log, bn.grouped(G):
            y = bn.bn_train(leaves[0], leaves[1], leaves[2], rm, rv, 0.1, EPS, leaves[3] if res is not None else None, relu)
            y.backward(dy)
        return y, leaves, rm, rv, slot

    for relu, residual in VARIANTS:
        res = res_all if residual else None
        y, leaves, rm, rv, slot = run(res)
        yd = y.detach()
        leaves64 = [v.double().requires_grad_() for v in (x, w, b)] + ([res.double().requires_grad_()] if residual else [])
        pres, y64 = [], []
        for k in range(G):
            sl = slice(k * N, (k + 1) * N)
            rm64, rv64 = rm0.double().clone(), rv0.double().clone()
            pre = F.batch_norm(leaves64[0][sl], rm64, rv64, leaves64[1], leaves64[2], True, 0.1, EPS)
            if residual:
                pre = pre + leaves64[3][sl]
            pres.append(pre.detach())
            y64.append(pre * (yd[sl] > 0).double() if relu else pre)          # (the fp32 output's ReLU pattern)
            if G == 1:
                torch.testing.assert_close(rm.double(), rm64, rtol=1e-6, atol=1e-6)
                torch.testing.assert_close(rv.double(), rv64, rtol=1e-5, atol=1e-6)
            else:
                xd = x[sl].double()
                torch.testing.assert_close(slot[k, :, 0], xd.mean((0, 2, 3)), rtol=1e-6, atol=1e-6)
                torch.testing.assert_close(slot[k, :, 1], xd.var((0, 2, 3), unbiased=True), rtol=1e-5, atol=1e-6)
        y64, pre = torch.cat(y64), torch.cat(pres)
        y64.backward(dy.double())
        torch.testing.assert_close(yd.double(), y64.detach(), rtol=1e-5, atol=2e-5)
        if relu:
            flipped = (yd > 0) != (pre > 0)
            assert flipped.sum() <= 8 and (pre[flipped].abs() < 1e-5).all()
        scale = M ** .5
        torch.testing.assert_close(leaves[0].grad.double(), leaves64[0].grad, rtol=2e-4, atol=2e-5 + 2e-4 / scale)
        torch.testing.assert_close(leaves[1].grad.double(), leaves64[1].grad, rtol=1e-4, atol=3e-5 * scale)
        torch.testing.assert_close(leaves[2].grad.double(), leaves64[2].grad, rtol=1e-4, atol=3e-5 * scale)
        if residual:
            torch.testing.assert_close(leaves[3].grad.double(), leaves64[3].grad, rtol=1e-6, atol=1e-6)
        y2, leaves2, *_ = run(res)                               # reproducible bit for bit
        assert torch.equal(y2, y)
        for a, bb in zip(leaves, leaves2):
            assert torch.equal(a.grad, bb.grad)
        if not relu:
            continue
        saved = bnlink.source_of(y)[1]
        sums, n_sums = _nan(C, G, g.S, 2, dtype=torch.float64), ctypes.c_int(0)
        _hip.check(lib.sgmcmc_bn_bwd_sums(dy.data_ptr(), yd.data_ptr(), x.data_ptr(), saved[0].data_ptr(),
                                          saved[1].data_ptr(), sums.data_ptr(), ctypes.byref(n_sums), n, C, P, G, _stream()),
                   "sgmcmc_bn_bwd_sums")
        assert n_sums.value == G * g.S
        _no_nan(sums=sums)
        # the kernel's own fp32 terms (one rounding per operation here as there: the library is built without contraction)
        col = lambda v: v.view(G, 1, C, 1)
        dz = R.grouped_view(dy * (yd > 0), G)
        tx = dz * ((R.grouped_view(x, G) - col(saved[0])) * col(saved[1]))
        for k, term in enumerate((dz, tx)):
            err = (sums[..., k] - _slice_sums(term, g)).abs()
            room = (per_thread + 2) * 2.0 ** -24 * _slice_sums(term.abs(), g)
            assert (err <= room).all(), f"partial {k}: worst {(err / room.clamp_min(1e-300)).max():.3g} of the bound"
        dx, dres, dgb = _nan(n, C, H, W), _nan(n, C, H, W) if residual else None, _nan(G, 2, C)
        _hip.check(lib.sgmcmc_bn_bwd_dx(dy.data_ptr(), yd.data_ptr(), x.data_ptr(), w.data_ptr(), saved[0].data_ptr(),
                                        saved[1].data_ptr(), 1, n, C, P, sums.data_ptr(), n_sums.value, dx.data_ptr(),
                                        dres.data_ptr() if residual else 0, dgb.data_ptr(), None, G, _stream()),
                   "sgmcmc_bn_bwd_dx")
        total, room = sums.sum(2).permute(1, 2, 0), REL64 * sums.abs().sum(2).permute(1, 2, 0)      # [G, 2, C]: dbeta first
        total, room = total.flip(1), room.flip(1)
        assert ((total - room).float() <= dgb).all() and (dgb <= (total + room).float()).all()
        assert torch.equal(dx, leaves[0].grad)                   # the same two kernels on the same operands
        if residual:
            assert torch.equal(dres, leaves[3].grad)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the dual launch off the trunk

DUAL_CASES = [(256, 16, 32, 32, 1, 1024), (13, 256, 32, 32, 1, 26), (3, 8, 64, 64, 1, 768), (64, 16, 32, 32, 2, 64)]


@GPU
@pytest.mark.parametrize("dc", DUAL_CASES, ids=[R.case_id(c[:5]) + f"-parts{c[5]}" for c in DUAL_CASES])
def test_dual_launch_has_the_bits_of_the_two_operators_off_the_trunk(dc):
    """relu(BN(x) + BN_s(r)) in one launch (_BNTrainDual) with equal-part partials computed here in float64, against
    bn_train of the shortcut, then bn_train(..., residual, relu=True) with the same ``stats=``: output, both layers' saved
    statistics, both layers' running (one group) or logged (groups) statistics and all six gradients are ``torch.equal``.
    No budget is involved: apply_dual_kernel is apply_kernel's arithmetic operation for operation on the same operands
    (its header comment), and the backward launches are the same; this runs it where the walk is not the trunk's."""
    *case, parts = dc
    n, C, P, G, g = _dims(case)
    H, W = case[2], case[3]
    gen = torch.Generator().manual_seed(n + C)
    x, r = (torch.randn(n, C, H, W, generator=gen) * 1.3 + 0.2).cuda(), (torch.randn(n, C, H, W, generator=gen) - 0.5).cuda()
    params = [(torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda(),
              (torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda()]
    dy = torch.randn(n, C, H, W, generator=gen).cuda()
    stats, r_stats = R.random_parts(x.cpu(), G, parts).cuda(), R.random_parts(r.cpu(), G, parts).cuda()

    def run(dual):
        xs, rs = x.clone().requires_grad_(), r.clone().requires_grad_()
        w, b, ws, bs = (p.clone().requires_grad_() for p in params)
        run_stats = [torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"),
                     torch.ones(C, device="cuda")]
        slots = {id(run_stats[0]): _nan(G, C, 2, dtype=torch.float64), id(run_stats[2]): _nan(G, C, 2, dtype=torch.float64)}
        log = bn.logging_running_stats(slots) if G > 1 else contextlib.nullcontext()
        with log, bn.grouped(G):
            if dual:
                out, saved = bn._BNTrainDual.apply(xs, w, b, stats, rs, ws, bs, r_stats, (run_stats[0], run_stats[1], 0.1, EPS),
                                                   (run_stats[2], run_stats[3], 0.05, 2e-5))
                r_saved = out.grad_fn.saved_tensors[6]
            else:
                s = bn.bn_train(rs, ws, bs, run_stats[2], run_stats[3], 0.05, 2e-5, stats=r_stats)
                out = bn.bn_train(xs, w, b, run_stats[0], run_stats[1], 0.1, EPS, residual=s, relu=True, stats=stats)
                saved, r_saved = bnlink.source_of(out)[1], bnlink.linear_source_of(s)[1]
            out.backward(dy)
        state = run_stats if G == 1 else list(slots.values())
        return [out.detach(), saved, r_saved] + state + [v.grad for v in (xs, w, b, rs, ws, bs)]

    names = ["out", "saved", "shortcut saved"] + ["running / logged statistics"] * (4 if G == 1 else 2) \
        + ["dx", "dgamma", "dbeta", "shortcut dx", "shortcut dgamma", "shortcut dbeta"]
    one, two = run(True), run(False)
    assert len(one) == len(two) == len(names)
    for name, a, bb in zip(names, one, two):
        _no_nan(**{name: a})
        assert torch.equal(a, bb), name
    # and the statistics are the batch's: the output against float64 (test_bn.py's forward tolerance)
    y64 = 0
    for t, (wt, bt) in ((x, params[:2]), (r, params[2:])):
        td = t.double().view(G, n // G, C, H, W)
        mu, var = td.mean((1, 3, 4), keepdim=True), td.var((1, 3, 4), unbiased=False, keepdim=True)
        eps = EPS if t is x else 2e-5
        y64 = y64 + ((td - mu) / (var + eps).sqrt() * wt.double().view(1, 1, C, 1, 1) + bt.double().view(1, 1, C, 1, 1))
    torch.testing.assert_close(one[0].double(), y64.clamp_min(0).view(n, C, H, W), rtol=1e-5, atol=4e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the evaluation kernel

EVAL_SHAPES = [(9, 8, 256, 256), (1, 1, 2, 2), (5, 3, 6, 10)]          # the first: a second grid-stride iteration


@GPU
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_kernel_is_exact_and_matches_aten(shape):
    """bn_eval beyond one grid (total4 = 9 * 8 * 16384 > 4096 * 256 blocks x threads) and at the smallest planes.
    Exact construction: integer x, running_mean and residual, running_var = 4^k (its float square root and the division
    1 / 2^k are exact), eps = 0, gamma a power of two, beta an integer: every operation of (x - mean) * invstd * g + b [+ r]
    is exact (asserted: the float64 result is an fp32 number of magnitude below 2^10 in steps of 2^-4 or coarser), with
    and without relu and residual.  Then random inputs at test_eval_mode_batchnorm_kernel_matches_aten's tolerance."""
    n, C, H, W = shape
    assert n * C * (H * W // 4) > 4096 * 256 or n < 9
    c = torch.arange(C)
    x, res = ints(shape, -8, 8, 5 + n).cuda(), ints(shape, -4, 4, 6 + n, nonzero=False).cuda()
    rm, rv = ints((C,), -3, 3, 7 + n, nonzero=False).cuda(), torch.exp2(2.0 * (c % 4 - 1)).cuda()
    gamma = (torch.exp2((c + 1) % 3 - 1.0) * torch.where((c // 2) % 2 == 1, -1.0, 1.0)).cuda()
    beta = ints((C,), -3, 3, 8 + n, nonzero=False).cuda()
    assert torch.equal(torch.sqrt(rv) ** 2, rv)
    cv = lambda v: v.double().view(1, C, 1, 1)
    base = (x.double() - cv(rm)) / cv(rv).sqrt() * cv(gamma) + cv(beta)
    with torch.no_grad():
        for relu, residual in VARIANTS:
            ref = base + res.double() if residual else base
            ref = ref.clamp_min(0) if relu else ref
            assert torch.equal(ref * 16, (ref * 16).round()) and ref.abs().max() < 2 ** 10
            assert bn.eval_supported(x, gamma, beta, rm, rv)
            assert_exact(bn.bn_eval(x, gamma, beta, rm, rv, 0.0, res if residual else None, relu), ref,
                         f"relu={relu}, residual={residual}")
        gen = torch.Generator().manual_seed(n + C)
        x = (torch.randn(shape, generator=gen) * 2 + 0.5).cuda()
        res = torch.randn(shape, generator=gen).cuda()
        w, b = (torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda()
        rm, rv = torch.randn(C, generator=gen).cuda(), (torch.rand(C, generator=gen) + 0.1).cuda()
        for relu, residual in VARIANTS:
            ref = F.batch_norm(x, rm, rv, w, b, False, 0.1, EPS)
            ref = ref + res if residual else ref
            ref = torch.relu(ref) if relu else ref
            torch.testing.assert_close(bn.bn_eval(x, w, b, rm, rv, EPS, res if residual else None, relu), ref,
                                       rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the replay kernels

SENTINEL = -77.0


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _replay_layers(widths, momenta, seed):
    "layers with running statistics inside sentinel-padded buffers (5 channels beyond each layer's own)"
    gen = torch.Generator().manual_seed(seed)
    layers = []
    for C, m in zip(widths, momenta):
        buf = torch.full((2, C + 5), SENTINEL)
        buf[0, :C], buf[1, :C] = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
        buf = buf.cuda()
        layers.append(types.SimpleNamespace(buf=buf, running_mean=buf[0, :C], running_var=buf[1, :C], momentum=m, num_features=C))
    return layers


def _clone_layers(layers):
    out = []
    for l in layers:
        buf = l.buf.clone()
        C = l.num_features
        out.append(types.SimpleNamespace(buf=buf, running_mean=buf[0, :C], running_var=buf[1, :C], momentum=l.momentum,
                                         num_features=C))
    return out


def _replay_log(n_entries, widths, seed):
    "[n_entries + 2, layers, cmax, 2] float64: NaN wherever no layer's entry lives (wider columns, rows past n_entries)"
    gen = torch.Generator().manual_seed(seed)
    log = torch.full((n_entries + 2, len(widths), max(widths) + 3, 2), NAN, dtype=torch.float64)
    for i, C in enumerate(widths):
        log[:n_entries, i, :C, 0] = torch.randn(n_entries, C, generator=gen, dtype=torch.float64)
        log[:n_entries, i, :C, 1] = torch.rand(n_entries, C, generator=gen, dtype=torch.float64) + 0.2
    return log.cuda()


def _check_replay(layers, log, n_entries, start):
    """each layer against the NumPy recurrence (float storage, float64 update) within one fp32 ulp.  The ONE licensed
    difference is a contraction of (1 - m) * r + m * e into a fused multiply-add: it changes the float64 value in its last
    bit, which moves the rounding to float across a tie at most, and the recurrence contracts (factor 1 - m) what it
    inherits.  Channels past C keep their sentinel."""
    for i, (l, l0) in enumerate(zip(layers, start)):
        C = l.num_features
        want = R.replay_reference(log[:n_entries, i, :C].cpu().numpy(), l.momentum, l0.buf[0, :C].cpu().numpy(),
                                  l0.buf[1, :C].cpu().numpy())
        _within_ulp(l.running_mean, want[0], f"layer {i}: running_mean")
        _within_ulp(l.running_var, want[1], f"layer {i}: running_var")
        assert bool((l.buf[:, C:] == SENTINEL).all()), f"layer {i}: channels past {C} were written"


@GPU
@pytest.mark.parametrize("n_entries", [1, 7, 8, 9, 16, 19])
def test_single_layer_replay(n_entries):
    "bn.replay_running_stats around its 8-deep block (tail only, block only, block + tail), widths around the 64-thread block"
    widths = [1, 63, 64, 65, 130]
    for C, mom in zip(widths, (0.1, 1.0, 0.37, 0.05, 0.1)):
        start = _replay_layers([C], [mom], 100 * n_entries + C)
        log = _replay_log(n_entries, [C], n_entries + C)
        keep = log.clone()
        assert log.stride(0) > 2 * C
        layers = _clone_layers(start)
        bn.replay_running_stats(log.data_ptr(), log.stride(0), n_entries, mom, layers[0].running_mean,
                                layers[0].running_var, _stream())
        _check_replay(layers, log, n_entries, start)
        assert torch.equal(_bits(log), _bits(keep))


@GPU
@pytest.mark.parametrize("n_layers,n_entries", [(1, 9), (32, 8), (33, 19), (40, 7)])
def test_many_layer_replay_has_the_bits_of_the_single_layer_kernel(n_layers, n_entries):
    """bn.replay_running_stats_many up to and past the 32 layers of one launch, mixed widths and momenta: the NumPy
    recurrence to one ulp, the single-layer kernel on the same log column BIT FOR BIT (both run ``replay_channel``),
    sentinels and the log untouched"""
    widths = [(1, 63, 64, 65, 130, 16, 32)[i % 7] for i in range(n_layers)]
    momenta = [(0.1, 0.05, 1.0, 0.37)[i % 4] for i in range(n_layers)]
    start = _replay_layers(widths, momenta, n_layers)
    log = _replay_log(n_entries, widths, n_layers + 1)
    keep = log.clone()
    many, single = _clone_layers(start), _clone_layers(start)
    bn.replay_running_stats_many(many, log, n_entries, _stream())
    _check_replay(many, log, n_entries, start)
    for i, l in enumerate(single):
        bn.replay_running_stats(log[0, i].data_ptr(), log.stride(0), n_entries, l.momentum, l.running_mean, l.running_var,
                                _stream())
    for i, (a, bb) in enumerate(zip(many, single)):
        assert torch.equal(a.buf, bb.buf), i
    assert torch.equal(_bits(log), _bits(keep))


@GPU
def test_replay_of_logged_forwards_equals_the_forwards_run_in_sequence():
    """nine logged forwards replayed -- by either kernel -- against the same nine forwards advancing the running
    statistics themselves: ``torch.equal``.  No budget: the log holds the float64 (mean, unbiased variance) the unlogged
    forward uses, and ``replay_channel`` writes apply_kernel's update expression (its header comment)."""
    n_entries, shape = 9, (6, 65, 4, 4)
    C = shape[1]
    gen = torch.Generator().manual_seed(3)
    xs = [(torch.randn(shape, generator=gen) * (1 + j) + j).cuda() for j in range(n_entries)]
    w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    start = _replay_layers([C], [0.1], 11)
    seq, one, many = _clone_layers(start), _clone_layers(start), _clone_layers(start)
    log = _nan(n_entries, 1, C, 2, dtype=torch.float64)
    with torch.no_grad():
        for j, x in enumerate(xs):
            bn.bn_train(x, w, b, seq[0].running_mean, seq[0].running_var, 0.1, EPS)
            with bn.logging_running_stats({id(one[0].running_mean): log[j, 0]}):
                bn.bn_train(x, w, b, one[0].running_mean, one[0].running_var, 0.1, EPS)
    assert torch.equal(one[0].buf, start[0].buf)
    _no_nan(log=log)
    bn.replay_running_stats(log.data_ptr(), log.stride(0), n_entries, 0.1, one[0].running_mean, one[0].running_var, _stream())
    bn.replay_running_stats_many(many, log, n_entries, _stream())
    assert torch.equal(one[0].buf, seq[0].buf) and torch.equal(many[0].buf, seq[0].buf)
    assert not torch.equal(seq[0].buf, start[0].buf)
