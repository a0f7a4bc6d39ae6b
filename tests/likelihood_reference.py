"""The softmax cross-entropy of one row, twice: in ``numpy.longdouble`` (the reference) and restated in ``numpy.float32``
in the kernels' own operation order (csrc/pool_hip.inc, xent::row) -- so that the tolerance of a GPU comparison is the
MEASURED rounding of that order on the test's own inputs, not a constant somebody picked.

The label rule (include/sgmcmc_hip.h, "Labels"): a label outside [0, K) gives its row a NaN loss and no one-hot term
(``d = p``); labels are compared as 64-bit integers.

Also the shared case list of tests/test_likelihood.py and tests/test_pool.py: row counts at the wave edges and the
shuffle tree's last wave, class counts from 1 to 16, and the logit families where a likelihood goes wrong."""
import functools

import numpy as np

LD = np.longdouble
EPS32 = float(np.finfo(np.float32).eps)

ROWS = [1, 63, 64, 65, 128, 1023, 1024]
CLASSES = [1, 2, 3, 10, 16]
FAMILIES = ["randn4", "ties", "spread30", "underflow200", "offset1e4"]


def _onehot(y, K):
    "[B, K] bool; a label outside [0, K) matches no class (int64 comparison: 2^32 + 1 is not class 1)"
    return np.arange(K, dtype=np.int64)[None, :] == np.asarray(y, dtype=np.int64)[:, None]


def rows64(logits, y):
    """(loss [B], p [B, K], d = p - onehot [B, K]) in longdouble from float32 logits and int64 labels; a label outside
    [0, K): NaN loss, d = p"""
    x = np.asarray(logits, dtype=np.float32).astype(LD)
    K = x.shape[1]
    hot = _onehot(y, K)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    valid = hot.any(axis=1)
    xt = np.where(hot, x, LD(0)).sum(axis=1)
    loss = np.where(valid, np.log(s[:, 0]) - (xt - m[:, 0]), LD("nan"))
    return loss, p, p - hot.astype(LD)


def rows32(logits, y):
    """the same three arrays in float32, operation by operation as xent::row: m = max; e_k = exp(x_k - m); s = the sum of
    e_k IN ORDER; inv = 1 / s; p_k = e_k * inv; d_k = p_k - [k == t]; loss = log(s) - (x_t - m)"""
    x = np.asarray(logits, dtype=np.float32)
    B, K = x.shape
    hot = _onehot(y, K)
    m = x.max(axis=1)
    e = np.exp(x - m[:, None]).astype(np.float32)
    s = np.zeros(B, dtype=np.float32)
    for k in range(K):
        s = (s + e[:, k]).astype(np.float32)
    inv = (np.float32(1) / s).astype(np.float32)
    p = (e * inv[:, None]).astype(np.float32)
    d = (p - hot.astype(np.float32)).astype(np.float32)
    xt = np.where(hot, x, np.float32(0)).sum(axis=1, dtype=np.float32)          # (one nonzero term: exact)
    loss = (np.log(s).astype(np.float32) - (xt - m).astype(np.float32)).astype(np.float32)
    loss = np.where(hot.any(axis=1), loss, np.float32("nan")).astype(np.float32)
    return loss, p, d


def total32(loss_rows, scale):
    """the batch total as xent::fwd_kernel forms it, in float32: a shuffle tree inside every wave of 64 rows (rows past
    the batch count 0), the waves' sums added in order, times the float32 ``scale``"""
    l = np.asarray(loss_rows, dtype=np.float32)
    waves = -(-l.shape[0] // 64)
    v = np.zeros(waves * 64, dtype=np.float32)
    v[:l.shape[0]] = l
    v = v.reshape(waves, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v[:, :off] + v[:, off:2 * off]).astype(np.float32)
    tot = np.float32(0)
    for w in range(waves):
        tot = np.float32(tot + v[w, 0])
    return np.float32(tot * np.float32(scale))


def dev(got, ref):
    "largest |got - ref| in longdouble (0.0 for identical arrays; NaN in both at the same place counts as equal)"
    g, r = np.asarray(got).astype(LD), np.asarray(ref).astype(LD)
    assert g.shape == r.shape, (g.shape, r.shape)
    both_nan = np.isnan(g) & np.isnan(r)
    diff = np.where(both_nan, LD(0), np.abs(g - r))
    return float(diff.max()) if not np.isnan(diff).any() else float("nan")


@functools.lru_cache(maxsize=None)
def case(family, K, B):
    """(logits float32 [B, K], labels int64 [B]) of one family; deterministic.  No infinities, no NaN.

    randn4        4 * standard normal logits, uniform labels
    ties          a third of the rows all equal (at a different constant each); the others have TWO tied maxima and the
                  rest up to 2 below; the label alternates between a tied class and (K >= 3) one off the tie
    spread30      one logit 30 above the smallest, the rest between; the label is the argmax on even rows, the argmin on odd
    underflow200  one logit 200 above every other: expf of the others underflows to 0 in float32 -- the loss is exactly
                  x_max - x_t and p is one-hot
    offset1e4     a common offset of +1e4 (even rows) or -1e4 (odd rows) plus a spread below 2: shift invariance"""
    rng = np.random.RandomState(1000 * FAMILIES.index(family) + 37 * K + B)
    rows = np.arange(B)
    y = rng.randint(0, K, size=B).astype(np.int64)
    if family == "randn4":
        x = 4 * rng.randn(B, K)
    elif family == "ties":
        x = -2 * rng.rand(B, K)
        a = rng.randint(0, K, size=B)
        b = (a + 1 + rng.randint(0, max(K - 1, 1), size=B)) % K                 # another class than a (K >= 2)
        x[rows, a] = 0
        x[rows, b] = 0
        off = np.where((a != 0) & (b != 0), 0, np.where((a != 1) & (b != 1), 1, 2))     # the first class off the tie
        y = np.where((rows % 2 == 0) | (K < 3), a, off).astype(np.int64)
        x += rng.randint(-3, 4, size=(B, 1))
        x[rows % 3 == 0] = rng.randint(-5, 6, size=(B, 1))[rows % 3 == 0]       # all-equal rows
    elif family == "spread30":
        x = 30 * rng.rand(B, K)
        hi = rng.randint(0, K, size=B)
        lo = (hi + 1 + rng.randint(0, max(K - 1, 1), size=B)) % K
        x[rows, lo] = 0
        x[rows, hi] = 30
        y = np.where(rows % 2 == 0, hi, lo).astype(np.int64)
    elif family == "underflow200":
        x = rng.randint(0, 5 * 1024, size=(B, K)) / 1024.0                      # (multiples of 2^-10: 205 - x is an fp32 number)
        hi = rng.randint(0, K, size=B)
        x[rows, hi] = 205
    elif family == "offset1e4":
        x = 2 * rng.rand(B, K) + np.where(rows % 2 == 0, 1e4, -1e4)[:, None]
    else:
        raise KeyError(family)
    x = x.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def reference(family, K, B):
    "(rows64, rows32) of ``case(family, K, B)``: computed once, shared by every test, read-only"
    x, y = case(family, K, B)
    out = rows64(x, y), rows32(x, y)
    for t in out:
        for a in t:
            a.setflags(write=False)
    return out
