"""The softmax cross-entropy of the classifiers (csrc/pool_hip.inc, xent::row) against longdouble, PER ROW and per
element, on every route that computes it: ``pool.cross_entropy`` / ``cross_entropy_backward``, the raw
sgmcmc_softmax_xent_fwd / _fwd_grad / _bwd, and the two launches that carry the likelihood with the last layer
(sgmcmc_linear_fwd_loss, sgmcmc_pool_linear_loss), fed inputs that make the logits the chosen numbers exactly.

No tolerance is a constant of this file: for each quantity of each (family, K) group it is 4 x the largest deviation
from longdouble of the SAME operation order restated in numpy float32 (likelihood_reference.rows32) over the group's row
counts -- the 4 covers the device's expf / logf (a few ulp from numpy's), the shuffle-tree total and the float32 scale.
Where the restatement is exact (K = 1, underflowed one-hot rows, all-equal rows of a power-of-two K) so must the kernel be.

A label outside [0, K) (include/sgmcmc_hip.h, "Labels"): NaN loss row, d = gscale * p, every other row untouched, and
nothing read or written outside the arrays (guard tails)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bnn_priors_amd import _hip, pool
from exact_inputs import assert_guard, guarded
from likelihood_reference import CLASSES, EPS32, FAMILIES, LD, ROWS, case, dev, reference, rows32, rows64, total32

GPU = pytest.mark.gpu
GROUPS = [(f, k) for f in FAMILIES for k in CLASSES]
GROUP_IDS = [f"{f}-K{k}" for f, k in GROUPS]


# ---------------------------------------------------------------------------------------------------------------------
# the references themselves, on the CPU

def _gap(x, y):
    "|x_t - m| per row and |x_k - m| per element, float64"
    x = x.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    return np.abs(x[np.arange(x.shape[0]), y] - m[:, 0]), np.abs(x - m)


@pytest.mark.parametrize("family,K", GROUPS, ids=GROUP_IDS)
def test_rows64_agrees_with_torch_float64(family, K):
    "likelihood_reference.rows64 == F.cross_entropy(reduction='none') / softmax of the float64 logits, to float64 rounding"
    eps64 = float(np.finfo(np.float64).eps)
    for B in ROWS:
        x, y = case(family, K, B)
        assert x.dtype == np.float32 and np.isfinite(x).all() and y.min() >= 0 and y.max() < K
        (loss, p, d), _ = reference(family, K, B)
        xt, yt = torch.from_numpy(x.copy()).double(), torch.from_numpy(y.copy())
        ref_loss = F.cross_entropy(xt, yt, reduction="none").numpy()
        ref_p = F.log_softmax(xt, dim=1).exp().numpy()
        gt, gk = _gap(x, y)
        assert (np.abs(loss.astype(np.float64) - ref_loss) <= (K + 6) * eps64 * (1 + gt + np.log(K))).all(), (family, K, B)
        assert (np.abs(p.astype(np.float64) - ref_p) <= (K + 6) * eps64 * (1 + gk) * ref_p + 1e-300).all(), (family, K, B)
        hot = F.one_hot(yt, K).numpy()
        assert dev(d, p - hot.astype(LD)) == 0.0 and dev(p.sum(axis=1), np.ones(B)) <= 4 * eps64


def test_rows64_and_rows32_follow_the_label_rule():
    "a label outside [0, K) -- K, -1, 2^32 + 1 (class 1 after a cast to int) -- gives a NaN loss and d = p; the others stay"
    x, y = case("randn4", 10, 65)
    for bad in (10, -1, 2 ** 32 + 1):
        y2 = y.copy()
        y2[7] = bad
        for rows in (rows64, rows32):
            (l0, p0, d0), (l1, p1, d1) = rows(x, y), rows(x, y2)
            keep = np.arange(65) != 7
            assert np.isnan(l1[7]) and not np.isnan(l1[keep]).any()
            assert dev(l1[keep], l0[keep]) == 0.0 and dev(p1, p0) == 0.0 and dev(d1[keep], d0[keep]) == 0.0
            assert dev(d1[7], p1[7]) == 0.0


@pytest.mark.parametrize("family,K", GROUPS, ids=GROUP_IDS)
def test_the_float32_restatement_stays_under_its_derived_cap(family, K):
    """rows32 - rows64, bounded from the operation order: s carries (K - 1) additions of terms that are each off by one
    expf rounding and the rounding of (x_k - m), the logarithm, (x_t - m) and the final subtraction one rounding each:
        |loss32 - loss| <= (K + 6) eps (1 + |x_t - m| + log K)
        |d32 - d|       <= (K + 6) eps ((1 + |x_k - m|) p_k + |d_k|)       (+ one float32 denormal)
    The cap only keeps the measured tolerance of the GPU tests from growing silently."""
    for B in ROWS:
        x, y = case(family, K, B)
        (loss, p, d), (loss32, p32, d32) = reference(family, K, B)
        gt, gk = _gap(x, y)
        cap_l = (K + 6) * EPS32 * (1 + gt + np.log(K))
        cap_d = (K + 6) * EPS32 * ((1 + gk) * p.astype(np.float64) + np.abs(d.astype(np.float64))) + 2.0 ** -149
        err_l = np.abs(loss32.astype(LD) - loss).astype(np.float64)
        err_d = np.abs(d32.astype(LD) - d).astype(np.float64)
        assert (err_l <= cap_l).all(), (family, K, B, float((err_l / cap_l).max()))
        assert (err_d <= cap_d).all(), (family, K, B, float((err_d / cap_d).max()))
        assert (np.abs(p32.astype(LD) - p).astype(np.float64) <= cap_d).all(), (family, K, B)


def test_the_restatement_is_exact_where_the_arithmetic_is():
    "K = 1: loss 0, p 1; underflow200: loss exactly x_max - x_t and p one-hot; all-equal rows of K = 2, 16: p = 1 / K"
    for family in FAMILIES:
        (loss, p, d), (loss32, p32, d32) = reference(family, 1, 65)
        assert (loss32 == 0).all() and (p32 == 1).all() and (d32 == 0).all() and dev(loss32, loss) == 0.0
    for K in CLASSES:
        x, y = case("underflow200", K, 128)
        (loss, p, d), (loss32, p32, d32) = reference("underflow200", K, 128)
        assert dev(loss32, x.max(axis=1).astype(LD) - x[np.arange(128), y].astype(LD)) == 0.0
        assert dev(loss32, loss) == 0.0 and set(np.unique(p32)) <= {0.0, 1.0} and dev(p32, p) < 1e-80
    for K in (2, 16):
        x = np.repeat(np.arange(-3, 4, dtype=np.float32)[:, None], K, axis=1)
        _, p32, _ = rows32(x, np.zeros(7, dtype=np.int64))
        assert (p32 == np.float32(1 / K)).all()


def test_total32_is_the_tree_order():
    "integer rows sum exactly whatever the order; on other rows the tree differs from the float64 sum by rounding only"
    for B in ROWS:
        l = np.arange(B, dtype=np.float32) % 7
        assert total32(l, 0.5) == np.float32(l.astype(np.float64).sum() * 0.5)
        r = np.random.RandomState(B).rand(B).astype(np.float32)
        assert abs(float(total32(r, 1.0)) - r.astype(np.float64).sum()) <= 8 * EPS32 * B


# ---------------------------------------------------------------------------------------------------------------------
# the kernels

class Tally:
    "per quantity: the largest deviation from longdouble of the float32 restatement and of the kernel over a group"

    def __init__(self, route, group):
        self.route, self.group, self.q = route, group, {}

    def add(self, qty, got, restated, ref):
        got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
        a = self.q.setdefault(qty, [0.0, 0.0])
        a[0], a[1] = max(a[0], dev(restated, ref)), _nanmax(a[1], dev(got, ref))

    def check(self):
        for qty, (r, k) in self.q.items():
            print(f"LIKELIHOOD {self.route} {self.group} {qty}: restatement {r:.3e} kernel {k:.3e}")
        for qty, (r, k) in self.q.items():
            assert k <= 4 * r, f"{self.route} {self.group} {qty}: the kernel is off by {k:.3e}, 4 x the restatement is {4 * r:.3e}"


def _nanmax(a, b):
    return float("nan") if (a != a or b != b) else max(a, b)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_case(family, K, B):
    x, y = case(family, K, B)
    return torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()


def _xent_fwd(x, y, scale):
    "raw sgmcmc_softmax_xent_fwd into guarded outputs -> (probs, total)"
    B, K = x.shape
    (probs, pw), (loss, lw) = guarded((B, K)), guarded((1,))
    _hip.check(_hip.lib().sgmcmc_softmax_xent_fwd(x.data_ptr(), y.data_ptr(), probs.data_ptr(), loss.data_ptr(), B, K,
                                                  float(scale), _stream()), "sgmcmc_softmax_xent_fwd")
    torch.cuda.synchronize()
    assert_guard(pw, probs, "probs")
    assert_guard(lw, loss, "loss")
    return probs, loss


def _xent_fwd_grad(x, y, scale, gscale):
    B, K = x.shape
    (d, dw), (loss, lw) = guarded((B, K)), guarded((1,))
    _hip.check(_hip.lib().sgmcmc_softmax_xent_fwd_grad(x.data_ptr(), y.data_ptr(), loss.data_ptr(), d.data_ptr(), B, K,
                                                       float(scale), float(gscale), _stream()), "sgmcmc_softmax_xent_fwd_grad")
    torch.cuda.synchronize()
    assert_guard(dw, d, "dlogits")
    assert_guard(lw, loss, "loss")
    return d, loss


def _xent_bwd(probs, y, g, scale):
    B, K = probs.shape
    d, dw = guarded((B, K))
    gout = torch.tensor([g], dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().sgmcmc_softmax_xent_bwd(probs.data_ptr(), y.data_ptr(), gout.data_ptr(), d.data_ptr(), B, K,
                                                  float(scale), _stream()), "sgmcmc_softmax_xent_bwd")
    torch.cuda.synchronize()
    assert_guard(dw, d, "dlogits of the backward")
    return d


def _linear_loss(x, y, gscale):
    """sgmcmc_linear_fwd_loss with J = K and the identity as weight: every product is x_k * 1 or x_j * 0, so the logits
    ARE x (asserted) and the likelihood is tested on known logits -> (loss_rows, dlogits)"""
    B, K = x.shape
    w = torch.eye(K, device="cuda")
    (logits, gw), (d, dw), (rows, rw) = guarded((B, K)), guarded((B, K)), guarded((B,))
    _hip.check(_hip.lib().sgmcmc_linear_fwd_loss(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), logits.data_ptr(),
                                                 d.data_ptr(), rows.data_ptr(), B, K, K, float(gscale), _stream()),
               "sgmcmc_linear_fwd_loss")
    torch.cuda.synchronize()
    for whole, out, what in ((gw, logits, "logits"), (dw, d, "dlogits"), (rw, rows, "loss_rows")):
        assert_guard(whole, out, "sgmcmc_linear_fwd_loss " + what)
    assert torch.equal(logits, x)
    return rows, d


def _head_loss(x, y, gscale):
    """sgmcmc_pool_linear_loss with C = K channels, 4 x 4 planes constant per channel and the identity as weight: the mean
    of 16 equal numbers and the products with 1 and 0 are exact, so pooled and logits ARE x -> (loss_rows, dlogits)"""
    B, K = x.shape
    h = x[:, :, None].expand(B, K, 16).contiguous()
    w = torch.eye(K, device="cuda")
    outs = {name: guarded(shape) for name, shape in (("pooled", (B, K)), ("logits", (B, K)), ("dlogits", (B, K)),
                                                     ("loss_rows", (B,)), ("dh", (B, K, 16)), ("slab_w", (B, K * K)),
                                                     ("slab_b", (B, K)))}
    o = {k: v[0] for k, v in outs.items()}
    _hip.check(_hip.lib().sgmcmc_pool_linear_loss(
        h.data_ptr(), w.data_ptr(), None, y.data_ptr(), o["pooled"].data_ptr(), o["logits"].data_ptr(),
        o["dlogits"].data_ptr(), o["loss_rows"].data_ptr(), o["dh"].data_ptr(), o["slab_w"].data_ptr(),
        o["slab_b"].data_ptr(), None, None, None, None, None, 0, None, 0, B, K, 16, K, float(gscale), _stream()),
        "sgmcmc_pool_linear_loss")
    torch.cuda.synchronize()
    for name, (out, whole) in outs.items():
        assert_guard(whole, out, "sgmcmc_pool_linear_loss " + name)
    assert torch.equal(o["pooled"], x) and torch.equal(o["logits"], x) and torch.equal(o["slab_b"], o["dlogits"])
    return o["loss_rows"], o["dlogits"]


def _g32(B, seed=1.0):
    "the float32 gradient scale of a batch mean, as the callers form it"
    return np.float32(seed) * np.float32(1.0 / B)


@GPU
@pytest.mark.parametrize("family,K", GROUPS, ids=GROUP_IDS)
def test_cross_entropy_through_autograd(family, K):
    "pool.cross_entropy (mean; backward through a factor 0.37) and pool.cross_entropy_backward (sum / 50000)"
    t = Tally("autograd", f"{family} K={K}")
    for B in ROWS:
        x, y = _dev_case(family, K, B)
        (loss, p, d), (loss32, p32, d32) = reference(family, K, B)
        lg = x.clone().requires_grad_()
        out = pool.cross_entropy(lg, y, "mean")
        (out * 0.37).backward()
        t.add("mean loss", out.detach().reshape(1), total32(loss32, 1.0 / B).reshape(1), (loss.sum() / B).reshape(1))
        t.add("d of 0.37 * mean", lg.grad, (_g32(B, 0.37) * d32).astype(np.float32), d * (LD(0.37) / B))
        lg2 = x.clone().requires_grad_()
        out2 = pool.cross_entropy_backward(lg2, y, "sum", divide_by=50000.0)
        t.add("sum loss / 50000", out2.reshape(1), (total32(loss32, 1.0) / np.float32(50000.0)).reshape(1),
              (loss.sum() / 50000).reshape(1))
        seed = np.float32(1.0) / np.float32(50000.0)
        t.add("d of sum / 50000", lg2.grad, (seed * d32).astype(np.float32), d / LD(50000))
    t.check()


@GPU
@pytest.mark.parametrize("family,K", GROUPS, ids=GROUP_IDS)
def test_raw_softmax_cross_entropy_entry_points(family, K):
    "sgmcmc_softmax_xent_fwd (probabilities, total), _fwd_grad (gradient, total) and _bwd (gradient from the probabilities)"
    t = Tally("raw xent", f"{family} K={K}")
    for B in ROWS:
        x, y = _dev_case(family, K, B)
        (loss, p, d), (loss32, p32, d32) = reference(family, K, B)
        probs, tot = _xent_fwd(x, y, 1.0 / B)
        t.add("p", probs, p32, p)
        t.add("total (fwd)", tot, total32(loss32, 1.0 / B).reshape(1), (loss.sum() / B).reshape(1))
        g = _g32(B)
        dg, tot2 = _xent_fwd_grad(x, y, 1.0 / B, g)
        assert torch.equal(tot2, tot)
        t.add("d (fwd_grad)", dg, (g * d32).astype(np.float32), d / B)
        db = _xent_bwd(probs, y, 1.0, 1.0 / B)
        assert torch.equal(db, dg)          # the header's promise: the same bits when grad_out * scale == grad_scale
        t.add("d (bwd)", db, (g * d32).astype(np.float32), d / B)
    t.check()


@GPU
@pytest.mark.parametrize("family,K", GROUPS, ids=GROUP_IDS)
def test_the_likelihood_inside_the_last_layers_launch(family, K):
    """loss_rows and dlogits of sgmcmc_linear_fwd_loss and sgmcmc_pool_linear_loss on logits that are the chosen numbers
    exactly, per row against longdouble -- and the same bits as sgmcmc_softmax_xent_fwd_grad, as the header says"""
    tl, th = Tally("linear_fwd_loss", f"{family} K={K}"), Tally("pool_linear_loss", f"{family} K={K}")
    for B in ROWS:
        x, y = _dev_case(family, K, B)
        (loss, p, d), (loss32, p32, d32) = reference(family, K, B)
        g = _g32(B)
        dg, _ = _xent_fwd_grad(x, y, 1.0, g)
        for tally, route in ((tl, _linear_loss), (th, _head_loss)):
            rows, dl = route(x, y, g)
            tally.add("loss_rows", rows, loss32, loss)
            tally.add("dlogits", dl, (g * d32).astype(np.float32), d / B)
            assert torch.equal(dl, dg), tally.route
    tl.check()
    th.check()


@GPU
def test_the_kernels_are_exact_where_the_restatement_is():
    """K = 1 (loss 0, p 1, d 0), underflowed rows (loss == x_max - x_t, p one-hot: expf(-200) is 0) and all-equal rows of
    K = 2 and 16 (p == 1 / K): no rounding happens in float32, so none is allowed"""
    for family in FAMILIES:
        x, y = _dev_case(family, 1, 65)
        probs, tot = _xent_fwd(x, y, 1.0)
        assert (probs == 1).all() and tot.item() == 0
        for route in (_linear_loss, _head_loss):
            rows, dl = route(x, y, 0.5)
            assert (rows == 0).all() and (dl == 0).all()
    for K in CLASSES:
        x, y = _dev_case("underflow200", K, 128)
        want = (x.max(dim=1).values.double() - x.double()[torch.arange(128), y]).float()
        hot = F.one_hot(x.argmax(dim=1), K).float()
        probs, tot = _xent_fwd(x, y, 1.0)
        assert torch.equal(probs, hot)
        if K > 1:
            assert tot.item() > 0
        for route in (_linear_loss, _head_loss):
            rows, dl = route(x, y, 0.5)
            assert torch.equal(rows, want) and torch.equal(dl, 0.5 * (hot - F.one_hot(y, K).float()))
    for K in (2, 16):
        x = torch.arange(-3, 4, dtype=torch.float32, device="cuda")[:, None].expand(7, K).contiguous()
        y = (torch.arange(7, device="cuda") % K).long()
        probs, _ = _xent_fwd(x, y, 1.0)
        assert (probs == 1.0 / K).all()
        for route in (_linear_loss, _head_loss):
            _, dl = route(x, y, 0.5)
            assert torch.equal(dl, 0.5 * (1.0 / K - F.one_hot(y, K).float()))


# ---------------------------------------------------------------------------------------------------------------------
# labels outside [0, K)

def _all_routes(x, y, g):
    "every per-row output of every route, by name: loss rows (or totals) and gradient rows"
    B = x.shape[0]
    probs, tot = _xent_fwd(x, y, 1.0 / B)
    dg, tot2 = _xent_fwd_grad(x, y, 1.0 / B, g)
    db = _xent_bwd(probs, y, 1.0, 1.0 / B)
    rl, dl = _linear_loss(x, y, g)
    rh, dh = _head_loss(x, y, g)
    return dict(totals=(tot, tot2), probs=probs, loss_rows=(rl, rh), d=(dg, db, dl, dh))


@GPU
@pytest.mark.parametrize("B", [1, 65, 128])
@pytest.mark.parametrize("bad", [10, -1, 2 ** 32 + 1], ids=["K", "minus_one", "two_to_32_plus_1"])
def test_a_label_outside_the_range(bad, B):
    """the label rule of include/sgmcmc_hip.h on every route: that row's loss is NaN (so is every total), its gradient row
    is gscale * p, every other row has the bits it has beside a valid label, nothing outside the outputs is written
    (guard tails, inside the helpers).  2^32 + 1 is class 1 after a cast to int: the comparison is 64-bit."""
    K = 10
    x, y = _dev_case("randn4", K, B)
    xh, yh = case("randn4", K, B)
    g = _g32(B)
    good = _all_routes(x, y, g)
    # the tolerance of this group, from the restatement on valid labels
    (loss, p, d), (loss32, p32, d32) = reference("randn4", K, B)
    for r in sorted({0, B // 2, B - 1}):
        y2h = yh.copy()
        y2h[r] = bad
        y2 = torch.from_numpy(y2h).cuda()
        _, p64, d64 = rows64(xh, y2h)
        _, _, d32b = rows32(xh, y2h)
        tol = 4 * dev((g * d32b).astype(np.float32), d64 / B)
        got = _all_routes(x, y2, g)
        keep = torch.arange(B, device="cuda") != r
        assert all(torch.isnan(t).all() for t in got["totals"]), (bad, B, r)
        assert torch.equal(got["probs"], good["probs"])
        for a, b in zip(got["loss_rows"], good["loss_rows"]):
            assert torch.isnan(a[r]) and torch.equal(a[keep], b[keep]), (bad, B, r)
        for a, b in zip(got["d"], good["d"]):
            assert torch.equal(a[keep], b[keep]), (bad, B, r)
            assert dev(a[r].cpu().numpy(), (p64[r] / B)) <= tol, (bad, B, r, dev(a[r].cpu().numpy(), p64[r] / B), tol)
            assert torch.equal(a[r], got["d"][0][r])
        # ... and through the module: NaN total, the same gradient rows
        lg = x.clone().requires_grad_()
        out = pool.cross_entropy(lg, y2, "mean")
        out.backward()
        assert torch.isnan(out) and torch.equal(lg.grad, got["d"][0])
        lg2 = x.clone().requires_grad_()
        assert torch.isnan(pool.cross_entropy_backward(lg2, y2, "mean")) and torch.equal(lg2.grad, got["d"][0])
