"""numpy restatement of the model-averaging weights (include/sgmcmc_hip.h "Model averaging"; Yao, Vehtari, Simpson &
Gelman 2018): pseudo-BMA, pseudo-BMA+ with the Bayesian bootstrap, stacking by the EM update of mixture proportions,
and the log density of a weighted mixture.  TEST INFRASTRUCTURE: the device path (csrc/weights_hip.inc) is compared
with this.

Every function takes ``sums``: how sums over observations and over replicates are taken --
``DEVICE`` (the header's order: slices of 1,024, 256 partial sums, a fixed tree, slices ascending), ``NUMPY``
(numpy's pairwise sums) or ``FSUM`` (exactly rounded, ``math.fsum``).  The three differ by rounding only; the test of
the summation order bounds by how much."""
import collections
import math

import numpy as np

from oracle import noise

SLICE, PARTIALS, MAX_MODELS, PURPOSE = 1024, 256, 32, 4

StackingRef = collections.namedtuple("StackingRef", "weights r gap iterations converged lpd")
BootstrapRef = collections.namedtuple("BootstrapRef", "weights se z w")


def _tree(acc):
    "[..., 256] -> [...]: partial t += partial t + w for w = 128, 64, ..., 1"
    w = PARTIALS // 2
    while w:
        acc = acc[..., :w] + acc[..., w:2 * w]
        w //= 2
    return acc[..., 0]


class _Device:
    name = "device"

    @staticmethod
    def obs(x, quads=False):
        "sum over the last axis (observations) in the header's order; ``quads``: partial t owns elements 4t .. 4t + 3"
        x = np.asarray(x, dtype=np.float64)
        N, S = x.shape[-1], -(-x.shape[-1] // SLICE)
        pad = np.zeros(x.shape[:-1] + (S * SLICE,))
        pad[..., :N] = x
        pad = pad.reshape(x.shape[:-1] + ((S, PARTIALS, 4) if quads else (S, 4, PARTIALS)))
        acc = np.zeros(x.shape[:-1] + (S, PARTIALS))
        for j in range(4):
            acc = acc + (pad[..., j] if quads else pad[..., j, :])
        per_slice = _tree(acc)
        out = np.zeros(x.shape[:-1])
        for s in range(S):
            out = out + per_slice[..., s]
        return out

    @staticmethod
    def reps(x):
        "sum over the last axis (replicates): 256 interleaved partial sums in ascending order, then the tree"
        x = np.asarray(x, dtype=np.float64)
        B, R = x.shape[-1], -(-x.shape[-1] // PARTIALS)
        pad = np.zeros(x.shape[:-1] + (R * PARTIALS,))
        pad[..., :B] = x
        pad = pad.reshape(x.shape[:-1] + (R, PARTIALS))
        acc = np.zeros(x.shape[:-1] + (PARTIALS,))
        for j in range(R):
            acc = acc + pad[..., j, :]
        return _tree(acc)


class _Numpy:
    name = "numpy"

    @staticmethod
    def obs(x, quads=False):
        return np.asarray(x, dtype=np.float64).sum(-1)

    reps = obs


class _Fsum:
    name = "fsum"

    @staticmethod
    def obs(x, quads=False):
        x = np.asarray(x, dtype=np.float64)
        flat = x.reshape(-1, x.shape[-1])
        out = np.array([math.fsum(row) if np.isfinite(row).all() else row.sum() for row in flat])
        return out.reshape(x.shape[:-1])

    reps = obs


DEVICE, NUMPY, FSUM = _Device, _Numpy, _Fsum


def _softmax(z):
    "z [..., K] -> exp(z - max) / sum_k exp(z - max), the sum over ascending k"
    e = np.exp(z - z.max(-1, keepdims=True))
    den = np.zeros(z.shape[:-1])
    for k in range(z.shape[-1]):
        den = den + e[..., k]
    return e / den[..., None]


def _check(P):
    P = np.asarray(P, dtype=np.float64)
    assert P.ndim == 2 and 1 <= P.shape[0] <= MAX_MODELS and P.shape[1] >= 1
    return P, P.shape[0], P.shape[1]


def _mq(P):
    "m [N] (NaN where the column has a non-finite entry), q [K, N] = exp(P - m)"
    with np.errstate(invalid="ignore"):
        m = np.where(np.isfinite(P).all(0), P.max(0), np.nan)
        return m, np.exp(P - m)


def _mix(w, q):
    mix = np.zeros(q.shape[1])
    for k in range(q.shape[0]):
        mix = mix + w[k] * q[k]
    return mix


def pseudo_bma(P, sums=DEVICE):
    "-> (weights [K], elpd [K])"
    P, K, N = _check(P)
    if not np.isfinite(P).all():
        return np.full(K, np.nan), np.full(K, np.nan)
    elpd = sums.obs(P)
    return _softmax(elpd), elpd


def bootstrap_g(N, B, seed=0, stream=0):
    "g [B, N] = -log u, u the Philox uniform of word i & 3 of counter (quad = i >> 2, draw = b, stream, purpose 4)"
    quads = np.arange(-(-N // 4), dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    g = np.empty((B, N))
    for b in range(B):
        x = noise.philox4x32_10_np(noise.noise_counter_np(quads, b, stream, PURPOSE), key)
        g[b] = -np.log(noise.uniform_np(x).reshape(-1)[:N])
    return g


def bb_pseudo_bma(P, B=1000, seed=0, stream=0, sums=DEVICE):
    P, K, N = _check(P)
    if not np.isfinite(P).all():
        return BootstrapRef(np.full(K, np.nan), np.full(K, np.nan), np.full((B, K), np.nan), np.full((B, K), np.nan))
    g = bootstrap_g(N, B, seed, stream)
    G = sums.obs(g, quads=True)
    X = sums.obs(g[:, None, :] * P[None], quads=True)
    z = (N * X) / G[:, None]
    w = _softmax(z)
    mz = sums.reps(z.T) / B
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt(sums.reps((z.T - mz[:, None]) ** 2) / (B - 1.0))
    return BootstrapRef(sums.reps(w.T) / B, se, z, w)


def stacking(P, tol=1e-8, max_iter=100_000, sums=DEVICE, trace=None):
    """The EM iteration of the header.  ``trace``: a list that receives (w, gap, lpd) of every iterate, the returned one
    included."""
    P, K, N = _check(P)
    if not np.isfinite(P).all():
        nan = np.full(K, np.nan)
        return StackingRef(nan, nan, np.nan, 0, False, np.nan)
    m, q = _mq(P)
    w, it = np.full(K, 1.0 / K), 0
    while True:
        mix = _mix(w, q)
        r = sums.obs(q / mix) / N
        lpd = float(sums.obs(m + np.log(mix)))
        gap = float(r.max() - 1.0)
        if trace is not None:
            trace.append((w.copy(), gap, lpd))
        converged = gap <= tol
        if converged or it >= max_iter:
            return StackingRef(w, r, gap, it, converged, lpd)
        w = w * r
        it += 1


def mixture_lpd(P, w, sums=DEVICE):
    "-> (total, pointwise [N])"
    P, K, N = _check(P)
    m, q = _mq(P)
    with np.errstate(invalid="ignore", divide="ignore"):
        pointwise = m + np.log(_mix(np.asarray(w, dtype=np.float64), q))
    return float(sums.obs(pointwise)), pointwise


def objective(P, w):
    "f(w) = (1/N) sum_i log sum_k w_k exp(P[k, i]), exactly rounded sum"
    return mixture_lpd(P, w, FSUM)[0] / np.asarray(P).shape[1]


def slsqp(P):
    "an independent optimiser of f over the simplex -> (w, f(w))"
    import scipy.optimize
    P, K, N = _check(P)
    m, q = _mq(P)

    def neg(w):
        mix = w @ q
        return -float(np.mean(m + np.log(mix))), -(q / mix).mean(1)

    res = scipy.optimize.minimize(neg, np.full(K, 1.0 / K), jac=True, method="SLSQP", bounds=[(0.0, 1.0)] * K,
                                  constraints=[{"type": "eq", "fun": lambda w: w.sum() - 1.0,
                                                "jac": lambda w: np.ones(K)}],
                                  options={"ftol": 1e-15, "maxiter": 2000})
    w = np.clip(res.x, 0.0, None)
    w /= w.sum()
    return w, objective(P, w)
