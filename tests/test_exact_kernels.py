"""The GEMM-like kernels and the slab / slice reductions on inputs where fp32 arithmetic is exact (tests/exact_inputs.py):
small integers, so every product and every partial sum is an fp32 number whatever the order of summation, and a kernel
has to equal the float64 reference of the same operator BIT FOR BIT.  One lost, doubled or misplaced term -- the last
pixel column of a slab's last image, a ragged item group, a slab skipped where one loop tier of ``reduce_block`` hands
over to the next -- moves the result by at least 1.  The random-input tests (test_conv.py, test_pool.py) bound rounding
error; these bound nothing: every comparison is ``torch.equal`` against float64 (``assert_exact``), after
``assert_budget`` has confirmed on the test's own inputs that exactness is owed.

Integer inputs also put exact zeros under the ReLU masks ([out > 0], not >= 0) and exact ties into the max-pool windows
(first position in scan order, as ATen), which random normals never do."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from bnn_priors_amd import _hip, conv, pool
from exact_inputs import NAN, assert_budget, assert_exact, assert_guard, guarded, ints
from test_conv import ALT, _check_stats

GPU = pytest.mark.gpu
EPS = torch.finfo(torch.float32).eps


# ---------------------------------------------------------------------------------------------------------------------
# float64 references with their budgets

def _run64(op, tensors, douts, dev):
    "``op`` on float64 copies of ``tensors``, backward with ``douts`` -> (outputs, gradients of the tensors)"
    leaves = [t.to(dev).double().requires_grad_() for t in tensors]
    outs = op(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward(outs, [d.to(dev).double() for d in douts])
    return [o.detach() for o in outs], [l.grad for l in leaves]


def _ref(op, tensors, douts, dev, unit=1.0):
    """float64 reference of a (multi)linear ``op`` and, from the same operator on the absolute values, the budget: the sum
    of |products| of every output and every gradient element, in units of ``unit`` (the values' common power of two)"""
    a_outs, a_grads = _run64(op, [t.abs() for t in tensors], [d.abs() for d in douts], dev)
    assert_budget(*(a / unit for a in a_outs + a_grads))
    return _run64(op, tensors, douts, dev)


def _dev():
    return "cuda" if torch.cuda.is_available() else "cpu"


# ---------------------------------------------------------------------------------------------------------------------
# the parametrization (shared by the CPU budget tests and the GPU tests)

TRUNK = sorted(conv.SHAPES)
TRUNK_N = [1, 3, 5, 37, 128]
# 515 images at 64 channels: the only way to 128 and more slabs there (4 images per slab) -- the 32-deep loads
TRUNK_CASES = [(c, hw, n) for c, hw in TRUNK for n in TRUNK_N] + [(64, 8, 515)]
MULTS = (0, 2, 4)
GROUP_IMGS = {1: 1, 3: 1, 5: 5, 37: 37, 128: 32, 515: 103}          # images per BatchNorm group: divides n
DOWN_CASES = [(cin, hwi, n) for cin, hwi in sorted(conv.DOWN_SHAPES) for n in (1, 3, 7, 37, 80, 128)]
N_OTHER = [1, 3, 37, 128]
N_TAIL = [1, 3, 5, 37, 128]
POOL_SHAPES = [(128, 50, 28, 28), (37, 50, 14, 14), (5, 3, 6, 10), (1, 1, 2, 2)]
HEAD_SHAPES = [(64, 8, 10), (16, 4, 3)]
LINEAR_SHAPES = [(2450, 10), (7, 1), (50, 16)]

# The classifier tail's edge grids (csrc/pool_hip.inc), through the C ABI into guarded outputs.  Crosses, not cubes.
# lin:: 48 kernels (K = 1..16 x fwd / fwd_loss / bwd); a thread column is 256 wide, one pass of fwd_body / the dx loop
# 1024 = 256 x CH; the weight gradient walks row groups of 16, and 16 rows x 16 outputs fill the 256-thread staging.
LIN_J = [1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2450]
LIN_N = [1, 15, 16, 17, 31, 32, 33, 128]
LINEAR_GRID = sorted({(j, k, n, wb) for j, n in ((257, 17), (1025, 16)) for k in range(1, 17) for wb in (True, False)}
                     | {(j, k, 17, True) for j in LIN_J for k in (1, 10, 16)}
                     | {(j, k, n, True) for j, k in ((300, 10), (257, 16)) for n in LIN_N})
# head:: P a power of two (the mean stays exact, each map its own unit 1 / P); C that leave a wave partly active;
# C * P / 4 below one block stride (256) and off its multiples; P != 64 takes the general pooling loop
HEAD_C = [1, 3, 16, 33, 63, 64]
HEAD_MAPS = [(4, 4), (4, 8), (8, 8), (8, 16), (16, 16)]
HEAD_GRID = [(c, m, k, n) for c, m in sorted({(c, m) for c in HEAD_C for m in ((4, 8), (16, 16))}
                                             | {(c, m) for c in (3, 64) for m in HEAD_MAPS})
             for k in (1, 10, 16) for n in (1, 3, 37)]
# pool::geo, S = 512 / C slices of the batch: S = 1 (C = 512), S clamped from 0 to 1 (C = 513), S recomputed from the
# images per slice (C = 100, N = 7: 5 -> 4), N < S, W = 2, H != W
POOL_GRID = [(3, 512, 2, 2), (2, 513, 2, 4), (7, 100, 4, 2), (7, 100, 2, 2), (2, 3, 4, 6), (5, 50, 4, 2), (3, 7, 2, 6), (1, 1, 4, 6)]
# the head's BatchNorm-backward partials (8 x 8 maps): channels, rows, rows per statistics group (0: one batch)
SUMS_GRID = [(c, n, g) for c in (1, 16, 33, 64) for n in (1, 3, 6, 37) for g in sorted({0, 1, 3, n}) if g == 0 or n % g == 0]


def _trunk_data(c, hw, n):
    s = 100000 * c + 100 * n
    return ints((n, c, hw, hw), -3, 3, s), ints((c, c, 3, 3), -3, 3, s + 1), ints((n, c, hw, hw), -3, 3, s + 2)


def _conv_op(**kw):
    return lambda x, w: F.conv2d(x, w, **kw)


@functools.lru_cache(maxsize=4)
def _trunk_ref(c, hw, n):
    "(x, w, dy) on the device and float64 (y, dx, dw); cached: the autograd and the C-ABI tests of a case share it"
    dev = _dev()
    x, w, dy = _trunk_data(c, hw, n)
    (y,), (dx, dw) = _ref(_conv_op(padding=1), (x, w), (dy,), dev)
    return tuple(t.to(dev) for t in (x, w, dy)), (y, dx, dw)


def _down_data(cin, hwi, n):
    s = 7000 * cin + n
    return (ints((n, cin, hwi, hwi), -3, 3, s), ints((2 * cin, cin, 3, 3), -3, 3, s + 1), ints((2 * cin, cin, 1, 1), -3, 3, s + 2),
            ints((n, 2 * cin, hwi // 2, hwi // 2), -3, 3, s + 3), ints((n, 2 * cin, hwi // 2, hwi // 2), -3, 3, s + 4))


def _down_op(x, wm, ws):
    return F.conv2d(x, wm, stride=2, padding=1), F.conv2d(x, ws, stride=2)


def _stem_data(n):
    return ints((n, 3, 32, 32), -3, 3, 300 + n), ints((16, 3, 3, 3), -3, 3, 301 + n), ints((n, 16, 32, 32), -3, 3, 302 + n)


def _first_data(n):
    return ints((n, 1, 28, 28), -3, 3, 280 + n), ints((50, 1, 3, 3), -3, 3, 281 + n), ints((n, 50, 28, 28), -3, 3, 282 + n)


def _conv50_data(n):
    return ints((n, 50, 14, 14), -3, 3, 500 + n), ints((50, 50, 3, 3), -3, 3, 501 + n), ints((n, 50, 14, 14), -3, 3, 502 + n)


def _tail_data(n, cin, hw, with_bias):
    "conv -> + bias -> ReLU -> MaxPool2d(2): zeros allowed everywhere, so ReLU edges and tied windows are common"
    s = 9000 * cin + 10 * n + with_bias
    return (ints((n, cin, hw, hw), -3, 3, s, nonzero=False), ints((50, cin, 3, 3), -2, 2, s + 1, nonzero=False),
            ints((50,), -3, 3, s + 2, nonzero=False) if with_bias else None, ints((n, 50, hw // 2, hw // 2), -3, 3, s + 3))


def _tail_ref(x, w, b, dp, dev):
    """float64 ATen composition of the fused tail and its gradients (x, w[, b]).  Budget: the convolution (+ bias) on
    absolute values; for the gradients every position of a window carries |dpooled| -- an upper bound of wherever the
    maximum routes it."""
    spread = F.interpolate(dp.abs(), scale_factor=2, mode="nearest")
    ts = (x, w) if b is None else (x, w, b)
    _ref(lambda x, w, b=None: F.conv2d(x, w, b, padding=1), ts, (spread,), dev)
    return _run64(lambda x, w, b=None: F.max_pool2d(F.relu(F.conv2d(x, w, b, padding=1)), 2), ts, (dp,), dev)


def _head_data(c, hw, k, n, with_bias):
    s = 100 * c + 10 * k + n
    return (ints((n, c, hw, hw), -3, 3, s), ints((k, c), -3, 3, s + 1), ints((k,), -3, 3, s + 2) if with_bias else None,
            ints((n, k), -3, 3, s + 3))


def _head_op(h, w, b=None):
    return F.linear(h.mean(dim=(2, 3)), w, b)


def _linear_data(j, k, n, with_bias):
    s = 10 * j + k + 1000 * n
    return ints((n, j), -3, 3, s), ints((k, j), -3, 3, s + 1), ints((k,), -3, 3, s + 2) if with_bias else None, ints((n, k), -3, 3, s + 3)


def _opt(*ts):
    return tuple(t for t in ts if t is not None)


def _head_grid_data(c, m, k, n, with_bias):
    s = 1000 * c + 100 * m[0] + 10 * m[1] + 7 * k + n
    return (ints((n, c) + tuple(m), -3, 3, s), ints((k, c), -3, 3, s + 1), ints((k,), -3, 3, s + 2) if with_bias else None,
            ints((n, k), -3, 3, s + 3))


def _sums_data(c, n, group_rows, k=10):
    """operands of the head's backward with the last BatchNorm's sums: integers, exact zeros under the mask [out > 0],
    integer BatchNorm input and mean, invstd a power of two per (group,) channel"""
    s = 77 * c + 5 * n + group_rows
    groups = n // group_rows if group_rows else 1
    pick = torch.tensor([0.5, 1.0, 2.0])
    return dict(dl=ints((n, k), -3, 3, s), pooled=ints((n, c), -3, 3, s + 1), w=ints((k, c), -3, 3, s + 2),
                y=ints((n, c, 8, 8), -3, 3, s + 3, nonzero=False), out=ints((n, c, 8, 8), -2, 2, s + 4, nonzero=False),
                mean=ints((groups, c), -2, 2, s + 5, nonzero=False),
                invstd=pick[ints((groups, c), 0, 2, s + 6, nonzero=False).long()])


def _sums_ref(D, group_rows, dev):
    """float64: dh[n, c, p] = (sum_k dl[n, k] w[k, c]) / 64;  partial[c, n, 0] = sum_p dh [out > 0];
    partial[c, n, 1] = sum_p dh [out > 0] (y - mean) invstd, with the statistics of the row's group.
    Budget in units of 1 / 128 (dh is a multiple of 1 / 64, xhat of 1 / 2)."""
    D = {k: v.to(dev).double() for k, v in D.items()}
    n, c = D["pooled"].shape
    g = (torch.arange(n, device=dev) // group_rows) if group_rows else torch.zeros(n, dtype=torch.long, device=dev)
    dh = ((D["dl"] @ D["w"]) / 64)[:, :, None, None].expand(n, c, 8, 8)
    a_dh = ((D["dl"].abs() @ D["w"].abs()) / 64)[:, :, None, None].expand(n, c, 8, 8)
    xhat = (D["y"] - D["mean"][g][:, :, None, None]) * D["invstd"][g][:, :, None, None]
    mask = (D["out"] > 0).double()
    assert_budget(128 * (a_dh * mask).sum((2, 3)), 128 * (a_dh * mask * xhat.abs()).sum((2, 3)), 64 * a_dh,
                  (D["dl"].abs()[:, :, None] * D["pooled"].abs()[:, None, :]).sum(0))
    partial = torch.stack([(dh * mask).sum((2, 3)).t(), (dh * mask * xhat).sum((2, 3)).t()], dim=-1)       # [c][n][2]
    slab_w = (D["dl"][:, :, None] * D["pooled"][:, None, :]).reshape(n, -1)
    return dh.contiguous(), partial.contiguous(), slab_w, D["dl"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the helper and the premise, on the CPU

def test_ints_are_integers_in_range_and_nonzero_on_request():
    a = ints((1000,), -3, 3, 0)
    assert a.dtype == torch.float32 and torch.equal(a, a.round()) and a.min() == -3 and a.max() == 3 and (a != 0).all()
    assert set(a.tolist()) == {-3., -2., -1., 1., 2., 3.}
    b = ints((1000,), -3, 3, 0, nonzero=False)
    assert set(b.tolist()) == {-3., -2., -1., 0., 1., 2., 3.}
    assert set(ints((100,), 1, 2, 0).tolist()) == {1., 2.} and torch.equal(ints((5, 4), -9, 9, 3), ints((5, 4), -9, 9, 3))


def test_assert_exact_reports_count_indices_and_unwritten_elements():
    ref = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    assert_exact(ref.float(), ref, "equal")
    got = ref.float()
    got[1, 2] += 1
    got[2, 3] = NAN
    with pytest.raises(AssertionError) as e:
        assert_exact(got, ref, "dw")
    msg = str(e.value)
    assert "dw: 2 of 12" in msg and "(1, 2): got 7.0, want 6.0, difference 1.0" in msg and "1 still hold the NaN" in msg
    with pytest.raises(AssertionError, match="2\\^24"):
        assert_budget(torch.tensor([2.0 ** 24 + 2], dtype=torch.float64))
    with pytest.raises(AssertionError, match="float64"):
        assert_budget(torch.tensor([1.0]))
    assert_budget(torch.tensor([2.0 ** 24], dtype=torch.float64))


@pytest.mark.parametrize("c,hw", TRUNK)
def test_budget_holds_for_the_trunk_shapes(c, hw):
    """values in [-3, 3]: a weight-gradient element sums n * hw^2 products of at most 9, an output 9c of them -- the
    largest case of every shape bounds the smaller ones, whose own inputs the GPU tests check again"""
    n = max(m for cc, hh, m in TRUNK_CASES if (cc, hh) == (c, hw))
    assert 9 * n * hw * hw <= 2 ** 24 and 9 * c * 9 <= 2 ** 24
    x, w, dy = (torch.full(s, 3.0) for s in ((2, c, hw, hw), (c, c, 3, 3), (2, c, hw, hw)))
    (y,), (dx, dw) = _run64(_conv_op(padding=1), (x, w), (dy,), "cpu")
    assert y.max() == dx.max() == 81 * c and dw.max() == 9 * 2 * hw * hw        # the interior: every tap inside
    assert_budget(y, dx, dw * (n / 2))
    for m in (1, 5):                                                            # and as the GPU tests do it
        _ref(_conv_op(padding=1), _trunk_data(c, hw, m)[:2], (_trunk_data(c, hw, m)[2],), "cpu")


def test_budget_holds_for_the_other_shapes():
    "the same worst cases in closed form for every other family: |values| <= 3, the largest n of its parametrization"
    for cin, hwi, n in DOWN_CASES:
        assert 9 * n * (hwi // 2) ** 2 <= 2 ** 24 and 9 * 9 * cin + 9 * 2 * cin * 9 <= 2 ** 24
    n = max(N_TAIL)
    assert 9 * n * 32 * 32 <= 2 ** 24 and 9 * n * 28 * 28 <= 2 ** 24 and 9 * n * 14 * 14 <= 2 ** 24      # stem, first, 50 -> 50
    assert 9 * 450 + 3 <= 2 ** 24 and 9 * 27 <= 2 ** 24
    for c, hw, k in HEAD_SHAPES:           # in units of 1 / hw^2: pooled values are sums of hw^2 integers
        assert 3 * hw * hw * 3 * c + 3 * hw * hw <= 2 ** 24 and 9 * hw * hw * n <= 2 ** 24 and 9 * k <= 2 ** 24
    for j, k in LINEAR_SHAPES:
        assert 9 * j + 3 <= 2 ** 24 and 9 * n <= 2 ** 24 and 9 * k <= 2 ** 24
    assert 300 * 1000 <= 2 ** 24                                                                         # the synthetic slabs
    # ... and on inputs as the GPU tests draw them, one small case per family
    _ref(_down_op, _down_data(16, 32, 3)[:3], _down_data(16, 32, 3)[3:], "cpu")
    _ref(_conv_op(padding=1), _stem_data(3)[:2], _stem_data(3)[2:], "cpu")
    _ref(_conv_op(padding=1), _first_data(3)[:2], _first_data(3)[2:], "cpu")
    _ref(_conv_op(padding=1), _conv50_data(3)[:2], _conv50_data(3)[2:], "cpu")
    x, w, b, dp = _tail_data(3, 50, 14, True)
    _tail_ref(x, w, b, dp, "cpu")
    h, w, b, dl = _head_data(16, 4, 3, 3, True)
    _ref(_head_op, (h, w, b), (dl,), "cpu", unit=1 / 16)
    x, w, b, dy = _linear_data(2450, 10, 3, True)
    _ref(F.linear, (x, w, b), (dy,), "cpu")


def test_budget_holds_for_the_tail_grids():
    """the classifier tail's edge grids: |values| <= 3, the worst case of each grid in closed form, then the largest cases
    on inputs as the GPU tests draw them"""
    for j, k, n, _ in LINEAR_GRID:
        assert 9 * j + 3 <= 2 ** 24 and 9 * n <= 2 ** 24 and 9 * k <= 2 ** 24          # y, dW / db, dx
    for c, (h, w), k, n in HEAD_GRID:           # in units of 1 / P: pooled values are sums of P integers, P a power of two
        P = h * w
        assert P & (P - 1) == 0 and 9 * P * c + 3 * P <= 2 ** 24 and 9 * P * n <= 2 ** 24 and 9 * k <= 2 ** 24
    for n, c, h, w in POOL_GRID:
        assert 3 * n * h * w <= 2 ** 24                                                # the bias gradient
    for c, n, g in SUMS_GRID:                   # in units of 1 / 128: 64 pixels of |dh| <= 90 / 64 times |xhat| <= 10
        assert 64 * 128 * (90 / 64) * 10 <= 2 ** 24
    assert max(j for j, _, _, _ in LINEAR_GRID) == 2450 and max(n for _, _, n, _ in LINEAR_GRID) == 128
    for j, k, n in ((2450, 16, 17), (300, 10, 128), (1025, 16, 16)):
        x, w, b, dy = _linear_data(j, k, n, True)
        _ref(F.linear, (x, w, b), (dy,), "cpu")
    for c, m, k, n in ((64, (16, 16), 16, 37), (3, (4, 4), 1, 1), (63, (4, 8), 10, 3)):
        h, w, b, dl = _head_grid_data(c, m, k, n, True)
        _ref(_head_op, (h, w, b), (dl,), "cpu", unit=1.0 / (m[0] * m[1]))
    for c, n, g in ((64, 37, 37), (33, 6, 3), (1, 1, 0)):
        _sums_ref(_sums_data(c, n, g), g, "cpu")


@pytest.mark.parametrize("c,hw,n", [(16, 32, 128), (64, 8, 128)])
def test_fp32_library_convolution_is_exact_on_these_inputs(c, hw, n):
    "the premise, independently of this repository's kernels: torch's own fp32 CPU convolution equals float64 here"
    x, w, dy = _trunk_data(c, hw, n)
    (y,), (_, dw) = _ref(_conv_op(padding=1), (x, w), (dy,), "cpu")
    assert_exact(F.conv2d(x, w, padding=1), y, "fp32 forward")
    assert_exact(torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=1), dw, "fp32 weight gradient")


def test_one_dropped_product_passes_the_old_bound_and_fails_the_exact_one():
    """the gap this file closes, stated on the float64 reference itself at (16, 32, 128): take ONE product
    x[n, ci, h, w] * dy[n, co, h', w'] out of one weight-gradient element -- the old test_conv.py bound
    64 eps sqrt(n hw^2) max|ref| accepts the result, ``assert_exact`` rejects it"""
    c, hw, n = 16, 32, 128
    x, w, dy = _trunk_data(c, hw, n)
    ref = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), padding=1)
    co, ci, r, s, img, h, v = 5, 11, 0, 2, n - 1, 7, hw - 2           # tap (0, 2) reads x one up, one right of dy's pixel
    term = x[img, ci, h + r - 1, v + s - 1].double() * dy[img, co, h, v].double()
    assert term != 0
    wrong = ref.clone()
    wrong[co, ci, r, s] -= term
    old = 64 * EPS * (n * hw * hw) ** .5 * max(1.0, ref.abs().max().item())
    assert (wrong - ref).abs().max() <= old and old > 1.0
    with pytest.raises(AssertionError, match="1 of 2304 elements differ"):
        assert_exact(wrong.float(), ref, "dw")
    assert_exact(ref.float(), ref, "dw")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the slab reduction on synthetic slabs

P_ALL = [1, 2, 3, 4, 5, 7, 15, 16, 17, 31, 32, 33, 63, 127, 128, 129, 255, 256, 257, 300]
# E: 2304 = 16 channels (vector path; wide from 256 slabs), 432 = the stem, 450 = the first layer (E % 4 != 0: scalar path),
# 9216 / 36864 = 32 / 64 channels (never wide), 4100 = just above the wide limit (no multiple of 9), 22500 = the 50 -> 50 layer
E_TAPS = [(2304, 9), (2304, 1), (432, 9), (432, 1), (450, 9), (450, 1), (9216, 9), (9216, 1), (36864, 9), (36864, 1),
          (4100, 1), (22500, 9), (22500, 1)]


@functools.lru_cache(maxsize=None)
def _slabs(E):
    "300 slabs of E nonzero integers in [-1000, 1000] (device), a job of P slabs takes the first P"
    part = ints((max(P_ALL), E), -1000, 1000, E).cuda()
    assert_budget(part.double().abs().sum(0))
    return part


def _slab_sum(part, P, E, taps):
    "the independent sum (ATen, float64), with the [taps][E / taps] -> [E / taps][taps] transposition of sgmcmc_reduce_job"
    ref = part[:P].double().sum(0)
    return ref.view(taps, E // taps).t().reshape(-1) if taps > 1 else ref


def _reduce_jobs(entries):
    jobs = (_hip.ReduceJob * len(entries))()
    for j, (part, out, P, taps) in zip(jobs, entries):
        j.part, j.out, j.n_slabs, j.numel, j.taps = part.data_ptr(), out.data_ptr(), P, out.numel(), taps
    return jobs


def _reduce_many(entries):
    jobs = _reduce_jobs(entries)
    _hip.check(_hip.lib().sgmcmc_wrw_reduce_many(ctypes.cast(jobs, ctypes.c_void_p), len(entries),
                                                 torch.cuda.current_stream().cuda_stream), "sgmcmc_wrw_reduce_many")
    torch.cuda.synchronize()


@GPU
@pytest.mark.parametrize("P", P_ALL)
@pytest.mark.parametrize("E,taps", E_TAPS)
def test_slab_reduction_equals_an_independent_sum(E, taps, P):
    """sgmcmc_wrw_reduce_many on [P][E] integers against part.double().sum(0): every remainder length of the 32-, 8- and
    4-deep tiers (16- and 4-deep on the scalar path) on both sides of the 16-, 32- and 128-slab boundaries, the wide path
    from 256 slabs where E <= 4096"""
    part = _slabs(E)
    assert part.data_ptr() % 16 == 0
    out = torch.full((E,), NAN, device="cuda")
    _reduce_many([(part, out, P, taps)])
    assert_exact(out, _slab_sum(part, P, E, taps), f"reduce P={P} E={E} taps={taps}")


@GPU
@pytest.mark.parametrize("P", [1, 3, 4, 17, 33, 129, 300])
@pytest.mark.parametrize("E,taps", [(2304, 9), (9216, 1), (4100, 1)])
def test_slab_reduction_of_unaligned_slabs(E, taps, P):
    "slabs one float off a 16-byte boundary with E % 4 == 0: the four scalar loads of reduce_block_vec"
    src = _slabs(E)
    buf = torch.empty(P * E + 4, device="cuda")
    part = buf[1:1 + P * E].view(P, E)
    part.copy_(src[:P])
    assert part.data_ptr() % 16 == 4 and E % 4 == 0
    out = torch.full((E,), NAN, device="cuda")
    _reduce_many([(part, out, P, taps)])
    assert_exact(out, _slab_sum(src, P, E, taps), f"unaligned reduce P={P} E={E} taps={taps}")


@GPU
@pytest.mark.parametrize("n_jobs", [2, 32, 33, 67])
def test_several_reductions_in_one_call(n_jobs):
    "mixed (P, E, taps) jobs in one call, up to and beyond the 32 (SGMCMC_REDUCE_JOBS) of a launch: the entry point splits"
    specs = [(P_ALL[(7 * i + 3) % len(P_ALL)], *E_TAPS[(5 * i) % len(E_TAPS)]) for i in range(n_jobs)]
    assert len({(P >= 256 and E <= 4096, E % 4 == 0) for P, E, _ in specs}) >= 3 or n_jobs < 8
    outs = [torch.full((E,), NAN, device="cuda") for _, E, _ in specs]
    _reduce_many([(_slabs(E), o, P, taps) for (P, E, taps), o in zip(specs, outs)])
    for i, ((P, E, taps), o) in enumerate(zip(specs, outs)):
        assert_exact(o, _slab_sum(_slabs(E), P, E, taps), f"job {i} of {n_jobs}: P={P} E={E} taps={taps}")


RIDER_SETS = [[(31, 2304, 9)], [(300, 2304, 9), (32, 450, 9)], [(33, 9216, 1), (300, 432, 9), (31, 4100, 1)],
              [(31, 36864, 9), (32, 2304, 1), (33, 22500, 9), (300, 450, 1)],
              [(300, 9216, 9), (33, 432, 1), (32, 22500, 1), (31, 450, 9)]]


@GPU
@pytest.mark.parametrize("first", [0, 1], ids=["riders_last", "riders_first"])
@pytest.mark.parametrize("riders", RIDER_SETS, ids=lambda r: "+".join(f"{P}x{E}x{t}" for P, E, t in r))
def test_ridden_reductions_equal_an_independent_sum(riders, first):
    """the same synthetic jobs as riders (``reduce_block<8>``: 8 loads in flight, no 32-deep tier) of one small carrier,
    sgmcmc_conv3x3_bwd_ride at (16, 32, n = 2) -- P on both sides of the 8-deep tier and on the wide path; the carrier's
    own gradients, on integer inputs, are exact beside them"""
    assert max(len(r) for r in RIDER_SETS) == _hip.RIDE_JOBS
    lib, s = _hip.lib(), torch.cuda.current_stream().cuda_stream
    n = 2
    x, w, dy = _cuda(*_trunk_data(16, 32, n))
    ref_dx = torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), padding=1)
    ref_dw = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), padding=1)
    dx, dw = torch.full_like(x, NAN), torch.full_like(w, NAN)
    scratch = torch.full((lib.sgmcmc_conv3x3_wrw_scratch_floats(n, 16, 32),), NAN, device="cuda")
    outs = [torch.full((E,), NAN, device="cuda") for _, E, _ in riders]
    jobs = _reduce_jobs([(_slabs(E), o, P, taps) for (P, E, taps), o in zip(riders, outs)])
    E0 = _hip.ConvBwdEpilogue()
    _hip.check(lib.sgmcmc_conv3x3_bwd_ride(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), ctypes.byref(E0),
                                           dw.data_ptr(), scratch.data_ptr(), n, 16, 32, None,
                                           ctypes.cast(jobs, ctypes.c_void_p), len(riders), first, s), "sgmcmc_conv3x3_bwd_ride")
    torch.cuda.synchronize()
    for (P, E, taps), o in zip(riders, outs):
        assert_exact(o, _slab_sum(_slabs(E), P, E, taps), f"rider P={P} E={E} taps={taps}")
    assert_exact(dx, ref_dx, "the carrier's dx")
    assert_exact(dw, ref_dw, "the carrier's dw")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the kernels on integer inputs: the trunk

def _items_per_slab(lib, c, hw):
    "WrwCfg::ITEMS, read off the library's own scratch size at 128 images (a whole number of slabs)"
    return 128 * (hw // 8) // (lib.sgmcmc_conv3x3_wrw_scratch_floats(128, c, hw) // (c * c * 9))


def _slab_count(lib, c, hw, n, mult):
    "P = ceil(n * (hw / 8) / (ITEMS * mult))"
    return -(-n * (hw // 8) // (_items_per_slab(lib, c, hw) * max(1, mult)))


@pytest.mark.parametrize("c,hw", TRUNK)
def test_trunk_cases_cover_the_reduction_tiers(c, hw):
    """the slab counts that the trunk parametrization (n x wrw_mult) produces at this shape, from the library's own scratch
    size: every residue mod 4, fewer than 4 slabs, 32..127 (8-deep loads only) and 128 or more (32-deep, or wide) -- so
    that a later change of the items per slab cannot hollow the coverage out unnoticed"""
    lib = _hip.lib()
    Ps = {_slab_count(lib, c, hw, n, m) for cc, hh, n in TRUNK_CASES if (cc, hh) == (c, hw) for m in MULTS}
    for cc, hh, n in TRUNK_CASES:
        if (cc, hh) == (c, hw):
            assert lib.sgmcmc_conv3x3_wrw_scratch_floats(n, c, hw) == _slab_count(lib, c, hw, n, 1) * c * c * 9
    assert {P % 4 for P in Ps} == {0, 1, 2, 3}, sorted(Ps)
    assert any(P < 4 for P in Ps) and any(32 <= P < 128 for P in Ps) and any(P >= 128 for P in Ps), sorted(Ps)


@GPU
@pytest.mark.parametrize("persistent", [False, True], ids=["default", "persistent"])
@pytest.mark.parametrize("c,hw,n", TRUNK_CASES)
def test_trunk_convolution_through_autograd(c, hw, n, persistent):
    "conv.conv3x3: forward, band sums, data gradient and weight gradient on the default and the persistent kernels"
    (x, w, dy), (ref_y, ref_dx, ref_dw) = _trunk_ref(c, hw, n)
    with conv.persistent(persistent):
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
        y, stats = conv.conv3x3(xg, wg, want_stats=True)
        y.backward(dy)
        torch.cuda.synchronize()
    assert not conv._pending
    assert_exact(y, ref_y, "y")
    assert_exact(xg.grad, ref_dx, "dx")
    assert_exact(wg.grad, ref_dw, "dw")
    bands = hw // (4 if persistent else 8)
    assert_exact(stats[:, :, 0], ref_y.reshape(n, c, bands, -1).sum(-1).permute(1, 0, 2).reshape(c, n * bands), "band sums")
    _check_stats(stats, ref_y, bands)                          # (M2 around a rounded mean: on its tolerance)
    with torch.no_grad(), conv.persistent(persistent):
        assert_exact(conv.conv3x3(x, w), ref_y, "y without autograd")
        assert_exact(conv._weight_grad(x, dy, w), ref_dw, "dw alone")
        assert_exact(conv._run(dy, w, True)[0], ref_dx, "dx alone")


EPIS = ["none", "add", "add_masked", "sums", "add_masked+sums", "add+sums+mask_dx", "add_masked+sums+mask_dx+groups"]


@functools.lru_cache(maxsize=2)
def _epilogue_data(c, hw, n):
    "operands of the epilogues: exact zeros under both ReLU masks; integer BatchNorm input and mean, invstd in {1/2, 1, 2}"
    s = 31 * c + n
    shape, groups = (n, c, hw, hw), n // GROUP_IMGS[n]
    pick = torch.tensor([0.5, 1.0, 2.0])
    return dict(e_dout=ints(shape, -3, 3, s).cuda(), e_out=ints(shape, -2, 2, s + 1, nonzero=False).cuda(),
                s_y=ints(shape, -3, 3, s + 2, nonzero=False).cuda(), s_out=ints(shape, -2, 2, s + 3, nonzero=False).cuda(),
                mean=ints((groups, c), -2, 2, s + 4, nonzero=False).cuda(),
                invstd=pick[ints((groups, c), 0, 2, s + 5, nonzero=False).long()].cuda())


def _epilogue_ref(c, hw, n, epi, ref_dx):
    """dx after the epilogue and the BatchNorm-backward sums, float64: dx += e_dout [* (e_out > 0)]; dz = dx * (s_out > 0);
    partial[c][img * bands + band] = (sum dz, sum dz * xhat), xhat = (s_y - mean) * invstd; mask_dx: dx leaves as dz.
    Budget of the sums in units of 1/2 (xhat is a multiple of it)."""
    D = _epilogue_data(c, hw, n)
    dx, partial = ref_dx, None
    if "add" in epi:
        dx = dx + D["e_dout"].double() * ((D["e_out"] > 0) if "add_masked" in epi else 1)
    if "sums" in epi:
        grouped = "groups" in epi
        g = (torch.arange(n, device="cuda") // GROUP_IMGS[n]) if grouped else torch.zeros(n, dtype=torch.long, device="cuda")
        mean, invstd = D["mean"].double()[g][:, :, None, None], D["invstd"].double()[g][:, :, None, None]
        dz = dx * (D["s_out"] > 0)
        xhat = (D["s_y"].double() - mean) * invstd
        bands = hw // 8
        slices = lambda t: t.reshape(n, c, bands, -1).sum(-1).permute(1, 0, 2).reshape(c, n * bands)
        assert_budget(slices(dz.abs()), slices(2 * dz.abs() * xhat.abs()))
        partial = torch.stack([slices(dz), slices(dz * xhat)], dim=-1)
        if "mask_dx" in epi:
            dx = dz
    return dx, partial


def _epilogue_struct(c, hw, n, epi, partial, mult):
    D, E = _epilogue_data(c, hw, n), _hip.ConvBwdEpilogue()
    if "add" in epi:
        E.e_dout = D["e_dout"].data_ptr()
        E.e_out = D["e_out"].data_ptr() if "add_masked" in epi else None
    if "sums" in epi:
        E.s_y, E.s_out = D["s_y"].data_ptr(), D["s_out"].data_ptr()
        E.s_mean, E.s_invstd, E.s_partial = D["mean"].data_ptr(), D["invstd"].data_ptr(), partial.data_ptr()
        E.group_imgs = GROUP_IMGS[n] if "groups" in epi else 0
        E.mask_dx = int("mask_dx" in epi)
    E.wrw_mult = mult
    return E


@GPU
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("c,hw,n", TRUNK_CASES)
def test_trunk_backward_with_its_epilogues_through_the_c_abi(c, hw, n, epi):
    """sgmcmc_conv3x3_bwd_ex with wrw_mult 0, 2 and 4 (grouped items: "equal to rounding" in the header, EQUAL here), the
    slab count of each as the header states it, reduced immediately and deferred to sgmcmc_wrw_reduce_many"""
    lib, s = _hip.lib(), torch.cuda.current_stream().cuda_stream
    (x, w, dy), (_, ref_dx0, ref_dw) = _trunk_ref(c, hw, n)
    ref_dx, ref_partial = _epilogue_ref(c, hw, n, epi, ref_dx0)
    slices = lib.sgmcmc_conv3x3_stat_slices(n, c, hw)
    assert slices == n * (hw // 8)
    for mult in MULTS:
        P_want = _slab_count(lib, c, hw, n, mult if "sums" in epi else 0)      # (grouped items come with the sums epilogue)
        for deferred in (False, True):
            dx, dw = torch.full_like(x, NAN), torch.full_like(w, NAN)
            partial = torch.full((c, slices, 2), NAN, dtype=torch.float64, device="cuda")
            scratch = torch.full((lib.sgmcmc_conv3x3_wrw_scratch_floats(n, c, hw),), NAN, device="cuda")
            E = _epilogue_struct(c, hw, n, epi, partial, mult)
            P = ctypes.c_int(0)
            _hip.check(lib.sgmcmc_conv3x3_bwd_ex(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), ctypes.byref(E),
                                                 0 if deferred else dw.data_ptr(), scratch.data_ptr(), n, c, hw,
                                                 ctypes.byref(P) if deferred else None, s), "sgmcmc_conv3x3_bwd_ex")
            what = f"wrw_mult={mult} deferred={deferred}"
            if deferred:
                assert P.value == P_want, what
                _reduce_many([(scratch, dw, P.value, 9)])
            torch.cuda.synchronize()
            assert_exact(dw, ref_dw, "dw " + what)
            assert_exact(dx, ref_dx, "dx " + what)
            if ref_partial is not None:
                assert_exact(partial, ref_partial, "BatchNorm-backward sums " + what)
        if "sums" not in epi:
            break


@ALT
@GPU
@pytest.mark.parametrize("epi", ["none", "add_masked+sums", "add+sums+mask_dx"])
@pytest.mark.parametrize("c,hw,n", [t for t in TRUNK_CASES if t[0] < 64])
def test_uniform_backward_on_integer_inputs(c, hw, n, epi):
    "the measured alternative sgmcmc_conv3x3_bwd_uniform: dx, the sums and the reduced weight gradient, exact as well"
    lib, s = _hip.lib(), torch.cuda.current_stream().cuda_stream
    (x, w, dy), (_, ref_dx0, ref_dw) = _trunk_ref(c, hw, n)
    ref_dx, ref_partial = _epilogue_ref(c, hw, n, epi, ref_dx0)
    dx, dw = torch.full_like(x, NAN), torch.full_like(w, NAN)
    partial = torch.full((c, n * (hw // 8), 2), NAN, dtype=torch.float64, device="cuda")
    E = _epilogue_struct(c, hw, n, epi, partial, 0)
    P = lib.sgmcmc_conv3x3_bwd_uniform_slabs(n, c, hw)
    part = torch.full((P * w.numel(),), NAN, device="cuda")
    _hip.check(lib.sgmcmc_conv3x3_bwd_uniform(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), ctypes.byref(E),
                                              part.data_ptr(), n, c, hw, s), "sgmcmc_conv3x3_bwd_uniform")
    _reduce_many([(part, dw, P, 9)])
    assert_exact(dx, ref_dx, "dx")
    assert_exact(dw, ref_dw, "dw")
    if ref_partial is not None:
        assert_exact(partial, ref_partial, "BatchNorm-backward sums")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the other kernels

def _band_sums(ref, parts):
    n, c = ref.shape[:2]
    return ref.reshape(n, c, parts, -1).sum(-1).permute(1, 0, 2).reshape(c, n * parts)


def _cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _leaves(*ts):
    return tuple(None if t is None else t.clone().requires_grad_() for t in ts)


@GPU
@pytest.mark.parametrize("cin,hwi,n", DOWN_CASES)
def test_down_block_pair(cin, hwi, n):
    "conv.conv_down: both outputs, their band sums, all three gradients"
    data = _down_data(cin, hwi, n)
    (rm, rs), (rdx, rdwm, rdws) = _ref(_down_op, data[:3], data[3:], "cuda")
    x, wm, ws, dym, dys = _cuda(*data)
    xg, wmg, wsg = _leaves(x, wm, ws)
    ym, ys, sm, ss = conv.conv_down(xg, wmg, wsg, True)
    torch.autograd.backward((ym, ys), (dym, dys))
    torch.cuda.synchronize()
    for got, ref, what in ((ym, rm, "main output"), (ys, rs, "shortcut output"), (xg.grad, rdx, "dx"),
                           (wmg.grad, rdwm, "dw of the 3x3"), (wsg.grad, rdws, "dw of the 1x1")):
        assert_exact(got, ref, what)
    for st, ref, what in ((sm, rm, "main"), (ss, rs, "shortcut")):
        assert_exact(st[:, :, 0], _band_sums(ref, hwi // 16), what + " band sums")
        _check_stats(st, ref, hwi // 16)


@GPU
@pytest.mark.parametrize("n", N_OTHER)
def test_stem_convolution(n):
    data = _stem_data(n)
    (ry,), (_, rdw) = _ref(_conv_op(padding=1), data[:2], data[2:], "cuda")
    x, w, dy = _cuda(*data)
    (wg,) = _leaves(w)
    y, st = conv.conv_stem(x, wg, True)
    y.backward(dy)
    torch.cuda.synchronize()
    assert_exact(y, ry, "y")
    assert_exact(wg.grad, rdw, "dw")
    assert_exact(st[:, :, 0], _band_sums(ry, 4), "band sums")
    _check_stats(st, ry, 4)


@GPU
@pytest.mark.parametrize("n", N_OTHER)
def test_first_layer_convolution(n):
    data = _first_data(n)
    (ry,), (_, rdw) = _ref(_conv_op(padding=1), data[:2], data[2:], "cuda")
    x, w, dy = _cuda(*data)
    (wg,) = _leaves(w)
    y = conv.conv_first(x, wg)
    y.backward(dy)
    torch.cuda.synchronize()
    assert_exact(y, ry, "y")
    assert_exact(wg.grad, rdw, "dw")


@GPU
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("n", N_TAIL)
def test_first_layer_with_its_tail(n, with_bias):
    "conv.conv_first_pool == ATen's conv -> + bias -> ReLU -> MaxPool2d(2) in float64, zeros and ties included"
    x, w, b, dp = _tail_data(n, 1, 28, with_bias)
    (rp,), grads = _tail_ref(x, w, b, dp, "cuda")
    assert (rp == 0).any() and (rp > 0).any()
    x, w, b, dp = _cuda(x, w, b, dp)
    wg, bg = _leaves(w, b)
    out = conv.conv_first_pool(x, wg, bg)
    out.backward(dp)
    torch.cuda.synchronize()
    assert_exact(out, rp, "pooled map")
    assert_exact(wg.grad, grads[1], "dw")
    if with_bias:
        assert_exact(bg.grad, grads[2], "db")


@GPU
@pytest.mark.parametrize("n", N_TAIL)
def test_conv50(n):
    "conv.conv50: value and both gradients; the data gradient alone with a frozen weight"
    data = _conv50_data(n)
    (ry,), (rdx, rdw) = _ref(_conv_op(padding=1), data[:2], data[2:], "cuda")
    x, w, dy = _cuda(*data)
    xg, wg = _leaves(x, w)
    y = conv.conv50(xg, wg)
    y.backward(dy)
    (xf,) = _leaves(x)
    conv.conv50(xf, w).backward(dy)
    torch.cuda.synchronize()
    assert_exact(y, ry, "y")
    assert_exact(xg.grad, rdx, "dx")
    assert_exact(wg.grad, rdw, "dw")
    assert_exact(xf.grad, rdx, "dx with a frozen weight")


@GPU
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("n", N_TAIL)
def test_conv50_with_its_tail(n, with_bias):
    x, w, b, dp = _tail_data(n, 50, 14, with_bias)
    (rp,), grads = _tail_ref(x, w, b, dp, "cuda")
    assert (rp == 0).any() and (rp > 0).any()
    x, w, b, dp = _cuda(x, w, b, dp)
    xg, wg, bg = _leaves(x, w, b)
    out = conv.conv50_pool(xg, wg, bg)
    out.backward(dp)
    torch.cuda.synchronize()
    assert_exact(out, rp, "pooled map")
    assert_exact(xg.grad, grads[0], "dx")
    assert_exact(wg.grad, grads[1], "dw")
    if with_bias:
        assert_exact(bg.grad, grads[2], "db")


@GPU
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_bias_relu_pool(shape, with_bias):
    "integers in [-2, 2] WITH zeros: tied windows and x + b == 0 under the ReLU on purpose"
    s = sum(shape) + with_bias
    x = ints(shape, -2, 2, s, nonzero=False)
    b = ints((shape[1],), -1, 1, s + 1, nonzero=False) if with_bias else None
    dy = ints((shape[0], shape[1], shape[2] // 2, shape[3] // 2), -3, 3, s + 2)
    op = lambda x, b=None: F.max_pool2d(F.relu(x if b is None else x + b.view(1, -1, 1, 1)), 2)
    assert_budget(F.interpolate(dy.double().abs(), scale_factor=2, mode="nearest").sum((0, 2, 3)))      # the bias gradient
    (ry,), grads = _run64(op, _opt(x, b), (dy,), "cuda")
    x, b, dy = _cuda(x, b, dy)
    xg, bg = _leaves(x, b)
    y = pool.bias_relu_pool(xg, bg)
    y.backward(dy)
    torch.cuda.synchronize()
    assert_exact(y, ry, "y")
    assert_exact(xg.grad, grads[0], "dx")
    if with_bias:
        assert_exact(bg.grad, grads[1], "db")


@GPU
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("n", N_OTHER)
@pytest.mark.parametrize("c,hw,k", HEAD_SHAPES)
def test_pool_linear_head(c, hw, k, n, with_bias):
    "the mean over hw^2 = 64 or 16 pixels is a power-of-two scaling: pooled values and both gradients stay exact"
    h, w, b, dl = _head_data(c, hw, k, n, with_bias)
    (ry,), grads = _ref(_head_op, _opt(h, w, b), (dl,), "cuda", unit=1.0 / (hw * hw))
    h, w, b, dl = _cuda(h, w, b, dl)
    hg, wg, bg = _leaves(h, w, b)
    out = pool.pool_linear(hg, wg, bg)
    out.backward(dl)
    torch.cuda.synchronize()
    assert_exact(out, ry, "logits")
    assert_exact(hg.grad, grads[0], "dh")
    assert_exact(wg.grad, grads[1], "dW")
    if with_bias:
        assert_exact(bg.grad, grads[2], "db")


@GPU
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("n", N_OTHER)
@pytest.mark.parametrize("j,k", LINEAR_SHAPES)
def test_narrow_linear(j, k, n, with_bias):
    x, w, b, dy = _linear_data(j, k, n, with_bias)
    (ry,), grads = _ref(F.linear, _opt(x, w, b), (dy,), "cuda")
    x, w, b, dy = _cuda(x, w, b, dy)
    xg, wg, bg = _leaves(x, w, b)
    y = pool.linear(xg, wg, bg)
    y.backward(dy)
    torch.cuda.synchronize()
    assert_exact(y, ry, "y")
    assert_exact(xg.grad, grads[0], "dx")
    assert_exact(wg.grad, grads[1], "dW")
    if with_bias:
        assert_exact(bg.grad, grads[2], "db")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the classifier tail at its geometry edges: the C ABI into NaN-filled outputs with a guard tail behind each (a write
#    at j >= J, past the pass tail of dx or past a slab shows as a touched guard, not as a fault), then through autograd

INVALID = 1          # hipErrorInvalidValue


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_guards(outs, what):
    for name, (out, whole) in outs.items():
        assert_guard(whole, out, f"{what}: {name}")


@GPU
@pytest.mark.parametrize("j,k,n,with_bias", LINEAR_GRID)
def test_narrow_linear_grid(j, k, n, with_bias):
    "sgmcmc_linear_fwd / _bwd (every K of the dispatch, J and N on both sides of every stride) and pool.linear"
    lib = _hip.lib()
    x, w, b, dy = _linear_data(j, k, n, with_bias)
    (ry,), grads = _ref(F.linear, _opt(x, w, b), (dy,), "cuda")
    x, w, b, dy = _cuda(x, w, b, dy)
    rg = lib.sgmcmc_linear_row_groups(n)
    assert rg == -(-n // 16)
    outs = dict(y=guarded((n, k)), dx=guarded((n, j)), slabs=guarded((rg, k, j)), db=guarded((k,)))
    o = {name: v[0] for name, v in outs.items()}
    _hip.check(lib.sgmcmc_linear_fwd(x.data_ptr(), w.data_ptr(), _p(b), o["y"].data_ptr(), n, j, k, _stream()), "sgmcmc_linear_fwd")
    _hip.check(lib.sgmcmc_linear_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), o["dx"].data_ptr(), o["slabs"].data_ptr(),
                                     o["db"].data_ptr(), n, j, k, _stream()), "sgmcmc_linear_bwd")
    torch.cuda.synchronize()
    _check_guards(outs, "narrow linear")
    assert_exact(o["y"], ry, "y")
    assert_exact(o["dx"], grads[0], "dx")
    assert_exact(o["slabs"].double().sum(0), grads[1], "dW (the row groups' slabs, summed)")
    for g in range(rg):           # ... and every slab is ITS rows' sum
        rows = slice(16 * g, min(n, 16 * g + 16))
        assert_exact(o["slabs"][g], dy[rows].double().t() @ x[rows].double(), f"slab of row group {g}")
    assert_exact(o["db"], dy.double().sum(0), "db")
    xg, wg, bg = _leaves(x, w, b)
    y = pool.linear(xg, wg, bg)
    y.backward(dy)
    torch.cuda.synchronize()
    assert_exact(y, ry, "y through autograd")
    assert_exact(xg.grad, grads[0], "dx through autograd")
    assert_exact(wg.grad, grads[1], "dW through autograd")
    if with_bias:
        assert_exact(bg.grad, grads[2], "db through autograd")


@GPU
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("c,m,k,n", HEAD_GRID, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pool_linear_head_grid(c, m, k, n, with_bias):
    "sgmcmc_pool_linear_fwd / _bwd on maps of 16 .. 256 pixels, square or not, and pool.pool_linear"
    lib, P = _hip.lib(), m[0] * m[1]
    h, w, b, dl = _head_grid_data(c, m, k, n, with_bias)
    (ry,), grads = _ref(_head_op, _opt(h, w, b), (dl,), "cuda", unit=1.0 / P)
    h, w, b, dl = _cuda(h, w, b, dl)
    outs = dict(pooled=guarded((n, c)), logits=guarded((n, k)), dh=guarded(h.shape), slab_w=guarded((n, k * c)),
                slab_b=guarded((n, k)))
    o = {name: v[0] for name, v in outs.items()}
    _hip.check(lib.sgmcmc_pool_linear_fwd(h.data_ptr(), w.data_ptr(), _p(b), o["pooled"].data_ptr(), o["logits"].data_ptr(),
                                          n, c, P, k, _stream()), "sgmcmc_pool_linear_fwd")
    torch.cuda.synchronize()
    _hip.check(lib.sgmcmc_pool_linear_bwd(dl.data_ptr(), o["pooled"].data_ptr(), w.data_ptr(), o["dh"].data_ptr(),
                                          o["slab_w"].data_ptr(), o["slab_b"].data_ptr(), n, c, P, k, _stream()),
               "sgmcmc_pool_linear_bwd")
    torch.cuda.synchronize()
    _check_guards(outs, "head")
    assert_exact(o["pooled"], h.double().mean(dim=(2, 3)), "pooled")
    assert_exact(o["logits"], ry, "logits")
    assert_exact(o["dh"], grads[0], "dh")
    assert_exact(o["slab_w"].double().sum(0).view(k, c), grads[1], "dW (the rows' slabs, summed)")
    assert_exact(o["slab_b"], dl.double(), "the rows of db")
    hg, wg, bg = _leaves(h, w, b)
    out = pool.pool_linear(hg, wg, bg)
    out.backward(dl)
    torch.cuda.synchronize()
    assert_exact(out, ry, "logits through autograd")
    assert_exact(hg.grad, grads[0], "dh through autograd")
    assert_exact(wg.grad, grads[1], "dW through autograd")
    if with_bias:
        assert_exact(bg.grad, grads[2], "db through autograd")


@GPU
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("shape", POOL_GRID)
def test_bias_relu_pool_grid(shape, with_bias):
    "the slice geometry of pool::geo at its edges, on tiny planes: integers in [-2, 2] with zeros (ties, x + b == 0)"
    lib = _hip.lib()
    n, c, hh, ww = shape
    s = sum(shape) + with_bias
    x = ints(shape, -2, 2, s, nonzero=False)
    b = ints((c,), -1, 1, s + 1, nonzero=False) if with_bias else None
    dy = ints((n, c, hh // 2, ww // 2), -3, 3, s + 2)
    op = lambda x, b=None: F.max_pool2d(F.relu(x if b is None else x + b.view(1, -1, 1, 1)), 2)
    assert_budget(F.interpolate(dy.double().abs(), scale_factor=2, mode="nearest").sum((0, 2, 3)))
    (ry,), grads = _run64(op, _opt(x, b), (dy,), "cuda")
    x, b, dy = _cuda(x, b, dy)
    S = lib.sgmcmc_pool_slices(n, c, hh, ww)
    want_S = min(max(512 // c, 1), n)
    want_S = -(-n // -(-n // want_S))
    assert S == want_S and 1 <= S <= n
    outs = dict(y=guarded(ry.shape), dx=guarded(shape), part=guarded((S, c)))
    o = {name: v[0] for name, v in outs.items()}
    _hip.check(lib.sgmcmc_bias_relu_pool_fwd(x.data_ptr(), _p(b), o["y"].data_ptr(), n, c, hh, ww, _stream()), "sgmcmc_bias_relu_pool_fwd")
    _hip.check(lib.sgmcmc_bias_relu_pool_bwd(x.data_ptr(), _p(b), dy.data_ptr(), o["dx"].data_ptr(), o["part"].data_ptr(),
                                             n, c, hh, ww, _stream()), "sgmcmc_bias_relu_pool_bwd")
    torch.cuda.synchronize()
    _check_guards(outs, "bias_relu_pool")
    assert_exact(o["y"], ry, "y")
    assert_exact(o["dx"], grads[0], "dx")
    ref_db = grads[1] if with_bias else _run64(op, (x.cpu(), torch.zeros(c)), (dy.cpu(),), "cuda")[1][1]
    assert_exact(o["part"].double().sum(0), ref_db, "db (the slices' partials, summed)")
    xg, bg = _leaves(x, b)
    y = pool.bias_relu_pool(xg, bg)
    y.backward(dy)
    torch.cuda.synchronize()
    assert_exact(y, ry, "y through autograd")
    assert_exact(xg.grad, grads[0], "dx through autograd")
    if with_bias:
        assert_exact(bg.grad, grads[1], "db through autograd")


def _sums_outputs(n, c, k):
    return dict(dh=guarded((n, c, 8, 8)), slab_w=guarded((n, k * c)), slab_b=guarded((n, k)),
                partial=guarded((c, n, 2), dtype=torch.float64))


@GPU
@pytest.mark.parametrize("c,n,group_rows", SUMS_GRID)
def test_head_batchnorm_backward_partials(c, n, group_rows):
    """sgmcmc_pool_linear_bwd_sums: partial[c, n, 0] = sum_p dh [out > 0], partial[c, n, 1] = sum_p dh [out > 0] xhat with
    the statistics of the row's group, EXACT on integer operands; then sgmcmc_pool_linear_loss with a non-null partial,
    whose dh / slabs / partials must be, bit for bit, those of the backward kernel fed the loss launch's own dlogits"""
    lib, k = _hip.lib(), 10
    D = _sums_data(c, n, group_rows, k)
    ref_dh, ref_partial, ref_sw, ref_sb = _sums_ref(D, group_rows, "cuda")
    D = {name: t.cuda() for name, t in D.items()}
    outs = _sums_outputs(n, c, k)
    o = {name: v[0] for name, v in outs.items()}
    _hip.check(lib.sgmcmc_pool_linear_bwd_sums(
        D["dl"].data_ptr(), D["pooled"].data_ptr(), D["w"].data_ptr(), o["dh"].data_ptr(), o["slab_w"].data_ptr(),
        o["slab_b"].data_ptr(), D["y"].data_ptr(), D["out"].data_ptr(), D["mean"].data_ptr(), D["invstd"].data_ptr(),
        o["partial"].data_ptr(), group_rows, n, c, 64, k, _stream()), "sgmcmc_pool_linear_bwd_sums")
    torch.cuda.synchronize()
    _check_guards(outs, "bwd_sums")
    assert_exact(o["dh"], ref_dh, "dh")
    assert_exact(o["partial"], ref_partial, "BatchNorm-backward partials")
    assert_exact(o["slab_w"], ref_sw, "the rows of dW")
    assert_exact(o["slab_b"], ref_sb, "the rows of db")
    # the fused launch: h = the BatchNorm + ReLU's output (the mask), random valid labels, counters advanced on the way
    labels = (ints((n,), 0, k - 1, 3 * c + n, nonzero=False)).long().cuda()
    bias = ints((k,), -3, 3, c + n).cuda()
    counters = torch.full((21 + 8,), -7, dtype=torch.int64, device="cuda")
    L = dict(_sums_outputs(n, c, k), pooled=guarded((n, c)), logits=guarded((n, k)), dlogits=guarded((n, k)),
             loss_rows=guarded((n,)))
    lo = {name: v[0] for name, v in L.items()}
    _hip.check(lib.sgmcmc_pool_linear_loss(
        D["out"].data_ptr(), D["w"].data_ptr(), bias.data_ptr(), labels.data_ptr(), lo["pooled"].data_ptr(),
        lo["logits"].data_ptr(), lo["dlogits"].data_ptr(), lo["loss_rows"].data_ptr(), lo["dh"].data_ptr(),
        lo["slab_w"].data_ptr(), lo["slab_b"].data_ptr(), D["y"].data_ptr(), D["out"].data_ptr(), D["mean"].data_ptr(),
        D["invstd"].data_ptr(), lo["partial"].data_ptr(), group_rows, counters.data_ptr(), 21, n, c, 64, k, 0.25, _stream()),
        "sgmcmc_pool_linear_loss")
    torch.cuda.synchronize()
    _check_guards(L, "pool_linear_loss with sums")
    assert (counters[:21] == -6).all() and (counters[21:] == -7).all()
    assert_exact(lo["pooled"], D["out"].double().mean(dim=(2, 3)), "pooled of the fused launch")
    assert_exact(lo["logits"], F.linear(D["out"].double().mean(dim=(2, 3)), D["w"].double(), bias.double()), "logits of the fused launch")
    again = _sums_outputs(n, c, k)
    a = {name: v[0] for name, v in again.items()}
    _hip.check(lib.sgmcmc_pool_linear_bwd_sums(
        lo["dlogits"].data_ptr(), lo["pooled"].data_ptr(), D["w"].data_ptr(), a["dh"].data_ptr(), a["slab_w"].data_ptr(),
        a["slab_b"].data_ptr(), D["y"].data_ptr(), D["out"].data_ptr(), D["mean"].data_ptr(), D["invstd"].data_ptr(),
        a["partial"].data_ptr(), group_rows, n, c, 64, k, _stream()), "sgmcmc_pool_linear_bwd_sums")
    torch.cuda.synchronize()
    for name in ("dh", "slab_w", "slab_b", "partial"):
        assert torch.equal(lo[name], a[name]), f"{name}: the fused launch and the backward kernel differ"
    assert not torch.isnan(lo["partial"]).any() and not torch.isnan(lo["loss_rows"]).any()


@GPU
def test_head_entry_points_refuse_what_they_cannot_do():
    """sums on another plane than 64, a row count that is no multiple of group_rows, 0 or more than 256 counters: each
    returns hipErrorInvalidValue before any launch -- every output still holds what it was filled with"""
    lib, n, c, k = _hip.lib(), 6, 16, 10
    D = {name: t.cuda() for name, t in _sums_data(c, n, 3, k).items()}
    labels = torch.zeros(n, dtype=torch.int64, device="cuda")
    counters = torch.full((300,), -7, dtype=torch.int64, device="cuda")

    def bwd_sums(plane, group_rows):
        outs = _sums_outputs(n, c, k)
        o = {name: v[0] for name, v in outs.items()}
        err = lib.sgmcmc_pool_linear_bwd_sums(
            D["dl"].data_ptr(), D["pooled"].data_ptr(), D["w"].data_ptr(), o["dh"].data_ptr(), o["slab_w"].data_ptr(),
            o["slab_b"].data_ptr(), D["y"].data_ptr(), D["out"].data_ptr(), D["mean"].data_ptr(), D["invstd"].data_ptr(),
            o["partial"].data_ptr(), group_rows, n, c, plane, k, _stream())
        torch.cuda.synchronize()
        return err, outs

    def loss(plane, group_rows, with_partial, n_counters):
        outs = dict(_sums_outputs(n, c, k), pooled=guarded((n, c)), logits=guarded((n, k)), dlogits=guarded((n, k)),
                    loss_rows=guarded((n,)))
        o = {name: v[0] for name, v in outs.items()}
        err = lib.sgmcmc_pool_linear_loss(
            D["out"].data_ptr(), D["w"].data_ptr(), None, labels.data_ptr(), o["pooled"].data_ptr(), o["logits"].data_ptr(),
            o["dlogits"].data_ptr(), o["loss_rows"].data_ptr(), o["dh"].data_ptr(), o["slab_w"].data_ptr(),
            o["slab_b"].data_ptr(), D["y"].data_ptr(), D["out"].data_ptr(), D["mean"].data_ptr(), D["invstd"].data_ptr(),
            o["partial"].data_ptr() if with_partial else None, group_rows,
            None if n_counters is None else counters.data_ptr(), n_counters or 0, n, c, plane, k, 1.0, _stream())
        torch.cuda.synchronize()
        return err, outs

    refused = [("bwd_sums, plane 16", bwd_sums(16, 0)), ("bwd_sums, 6 rows in groups of 4", bwd_sums(64, 4)),
               ("loss with sums, plane 16", loss(16, 0, True, None)), ("loss, 6 rows in groups of 4", loss(64, 4, True, None)),
               ("loss, 0 counters", loss(64, 0, True, 0)), ("loss, 257 counters", loss(64, 0, False, 257))]
    for what, (err, outs) in refused:
        assert err == INVALID, f"{what}: returned {err}"
        for name, (out, whole) in outs.items():
            assert torch.isnan(whole).all(), f"{what}: {name} was written"
    assert (counters == -7).all()
    # ... and what they CAN do next to it: the same calls with the offending argument put right
    for what, (err, outs) in (("bwd_sums", bwd_sums(64, 3)), ("loss", loss(64, 3, True, 256))):
        assert err == 0, f"{what}: returned {err}"
        written = [name for name, (out, whole) in outs.items() if not torch.isnan(out).any()]
        assert "dh" in written and "slab_w" in written, (what, written)
        _check_guards(outs, what)
    assert (counters[:256] == -6).all() and (counters[256:] == -7).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the dense path's slice sums

@GPU
@pytest.mark.parametrize("n_slices", [1, 2, 8, 9])
@pytest.mark.parametrize("n", [3, 259, 1027])
def test_accumulate_parts(n, n_slices):
    "sgmcmc_accumulate_parts as fused_dense.exact calls it: first = 1, then first = 0 onto the accumulator, out_f32 last"
    lib, s = _hip.lib(), torch.cuda.current_stream().cuda_stream
    stride = n + 5
    acc = torch.full((stride,), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((stride,), NAN, device="cuda")
    stats = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
    want, want_stats = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    budget = torch.zeros_like(want)
    for call in range(3):
        gpart = ints((n_slices, stride), -1000, 1000, 10 * n + n_slices + call).cuda()
        loss, corr = ints((n_slices,), 1, 50, call).cuda(), ints((n_slices,), 0, 16, call + 5).cuda()
        last = call == 2
        _hip.check(lib.sgmcmc_accumulate_parts(gpart.data_ptr(), n_slices, stride, acc.data_ptr(), out.data_ptr() if last else None,
                                               n, loss.data_ptr(), corr.data_ptr(), stats.data_ptr(), int(call == 0), s),
                   "sgmcmc_accumulate_parts")
        torch.cuda.synchronize()
        want += gpart.double().sum(0)[:n]
        budget += gpart.double().abs().sum(0)[:n]
        want_stats += torch.stack([loss.double().sum(), corr.double().sum()])
        assert_exact(acc[:n], want, f"accumulator after call {call}")
        assert_exact(stats, want_stats, f"loss / correct sums after call {call}")
    assert_budget(budget)                                                       # (float)acc is exact
    assert_exact(out[:n], want, "out_f32")
    assert torch.isnan(acc[n:]).all() and torch.isnan(out[n:]).all()            # nothing past n is touched


@GPU
@pytest.mark.parametrize("n_slices", [1, 2, 8, 9])
def test_grad_reduce_prior_without_priors(n_slices):
    """sgmcmc_grad_reduce_prior with every segment SGMCMC_PRIOR_NONE: g of every segment = the sum over the slices of its
    range of gpart -- full 4-wide items, a ragged last item (numel % 4 != 0), a segment of several chunks"""
    from bnn_priors_amd.mcmc.engine import Engine
    params = [torch.zeros(shape, device="cuda").requires_grad_() for shape in ((7,), (50, 10), (1030,), (1,), (2, 3, 4))]
    for p in params:
        p.grad = torch.full_like(p, NAN)
    eng = Engine([{"params": params}], seed=1)
    eng.refresh([1.0] * len(params))
    assert (eng.seg_host["prior_kind"] == _hip.PRIOR_NONE).all() and eng.layout.prior_flags == 0
    stride = int(eng.seg_host["noise_base"][-1]) + -(-params[-1].numel() // 4) * 4
    gpart = ints((n_slices, stride), -1000, 1000, n_slices).cuda()
    assert_budget(gpart.double().abs().sum(0))
    loss, corr = ints((n_slices,), 1, 50, 1).cuda(), ints((n_slices,), 0, 16, 2).cuda()
    _hip.check(eng.lib.sgmcmc_grad_reduce_prior(ctypes.byref(eng.layout), gpart.data_ptr(), n_slices, stride, loss.data_ptr(),
                                                corr.data_ptr(), 4, 1000.0, 0, None, eng.stream()), "sgmcmc_grad_reduce_prior")
    torch.cuda.synchronize()
    total = gpart.double().sum(0)
    for i, p in enumerate(params):
        base = int(eng.seg_host["noise_base"][i])
        assert_exact(p.grad.reshape(-1), total[base:base + p.numel()], f"g of segment {i}")
    assert_exact(eng.scalars[4:6], torch.stack([loss.double().sum(), corr.double().sum()]) / 4, "loss / accuracy scalars")
