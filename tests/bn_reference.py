"""What tests/test_bn_exact.py needs to hold the BatchNorm kernels (csrc/bn_hip.inc) to exact results: a Python
restatement of ``bn::geo`` with a classifier of the run-time branches a geometry takes, inputs on which the kernels owe
exact results, exact references (Python integers / ``Fraction``), and fp32 / fp64 NumPy restatements of the kernels'
own expressions in the kernels' order, used on the CPU only to justify the bounds the GPU tests apply.

Nothing here touches a GPU."""
import collections
import functools
from fractions import Fraction

import numpy as np
import torch

from exact_inputs import assert_budget, ints

kT = 256                                   # bn::kT, threads per block
Geo = collections.namedtuple("Geo", "N C P S NB G")

# (n, C, H, W, G): n images of the launch = G groups of n / G.  What each case reaches: ``classify``.
TABLE = [
    (256, 16, 32, 32, 1),      # V == kT, count 8: a full second quad, x4 on every slice, XCD order
    (13, 256, 32, 32, 1),      # V == kT, counts 7 and 6: partial quads, no x4
    (17, 256, 32, 32, 1),      # counts 9 and 8: x4 on one slice of two
    (8, 512, 32, 32, 1),       # S = 1, count 8
    (80, 16, 32, 32, 1),       # ragged last slice (3, 3, ..., 2), plain order
    (23, 64, 32, 32, 1),       # S = 8 (XCD order) with a ragged last slice
    (11, 600, 16, 32, 1),      # V < kT (2 images per pass), counts 6 and 5, C > 512
    (120, 600, 6, 6, 1),       # V = 9: 4 idle threads, counts 5 and 4
    (3, 8, 64, 64, 1),         # V > kT, 4 float4 per thread and plane
    (2, 4, 32, 36, 1),         # V > kT with a V % 256 tail
    (18, 8, 40, 40, 2),        # ... and with groups
    (9, 5, 2, 2, 1),           # P = 4
    (1, 1, 2, 2, 1),
    (600, 1, 4, 4, 1),         # C = 1 with S = 300: more slices than threads
    (7, 513, 4, 4, 1),         # C just above 512
    (5, 1024, 8, 8, 1),        # C far above 512
    (48, 64, 32, 32, 3),       # XCD order with groups
    (64, 16, 32, 32, 2),
    (33, 16, 32, 32, 3),       # plain order with groups
    (10, 256, 8, 8, 2),        # plain order with groups AND a ragged last slice
    (46, 64, 8, 8, 2),         # XCD order with groups and a ragged last slice
    (128, 16, 32, 32, 1),      # the three trunk shapes: anchors to the workload
    (128, 32, 16, 16, 1),
    (128, 64, 8, 8, 1),
]


def case_id(case):
    n, C, H, W, G = case
    return f"{n}x{C}x{H}x{W}" + (f"-G{G}" if G > 1 else "")


def geo(n, C, P, G=1):
    "bn::geo: None where the kernels refuse the shape"
    if n <= 0 or C <= 0 or P <= 0 or P % 4 or G <= 0 or n % G:
        return None
    N = n // G
    S = min(max(512 // C, 1), N)
    NB = (N + S - 1) // S
    return Geo(N, C, P, (N + NB - 1) // NB, NB, G)


def slice_images(g):
    "images of every slice of one group (bn::decode: n1 - n0)"
    return [min(g.N, (s + 1) * g.NB) - s * g.NB for s in range(g.S)]


def thread_counts(g, ns):
    "bn::walk_of: the ``count`` of every working thread class of a slice of ``ns`` images (empty: V > kT, no walk)"
    V = g.P // 4
    if V == kT:
        return [ns]
    if V < kT:
        ipp = kT // V
        return [(ns - j + ipp - 1) // ipp if ns - j > 0 else 0 for j in range(ipp)]
    return []


def classify(n, C, P, G=1):
    "the branch class of a case: which of the kernels' run-time arms it takes"
    g = geo(n, C, P, G)
    V = P // 4
    ns = slice_images(g)
    if V > kT:
        walk = "V>kT,tail" if V % kT else "V>kT"
    elif V == kT:
        walk = "V==kT"
    else:
        walk = "V<kT,idle" if kT % V else "V<kT"
    counts = [c for k in ns for c in thread_counts(g, k)]
    second = {("partial" if c % 4 else "full") for c in counts if c > 4}      # walk_finish's second loop
    x4 = [V == kT and k % 4 == 0 for k in ns]                                  # for_each_vec_x4 per slice
    return dict(geo=g, walk=walk, float4_per_thread=(V + kT - 1) // kT, count_max=max(counts, default=0),
                count_min=min(counts, default=0), second_loop=second or {"none"},
                x4="all" if all(x4) else "some" if any(x4) else "none",
                order="xcd" if g.S % 8 == 0 else "plain", ragged=g.N % g.NB != 0, single_slice=g.S == 1,
                slices_beyond_block=g.S > kT, groups=G > 1, wide=C > 512)


def tags(info):
    "the classes of ``classify``'s answer as names"
    t = {"walk:" + info["walk"], "x4:" + info["x4"], "order:" + info["order"],
         "ragged:" + ("yes" if info["ragged"] else "no"), "S==1:" + ("yes" if info["single_slice"] else "no")}
    t |= {"second-loop:" + s for s in info["second_loop"]}
    if info["groups"]:
        t.add("groups:" + info["order"] + ("+ragged" if info["ragged"] else ""))
    if info["wide"]:
        t.add("C>512")
    if info["slices_beyond_block"]:
        t.add("S>kT")
    return frozenset(t)


# every class the classifier can return
ALL_TAGS = frozenset(
    ["walk:" + w for w in ("V>kT", "V>kT,tail", "V==kT", "V<kT", "V<kT,idle")]
    + ["x4:" + w for w in ("all", "some", "none")] + ["order:xcd", "order:plain", "ragged:yes", "ragged:no",
                                                       "S==1:yes", "S==1:no"]
    + ["second-loop:" + w for w in ("none", "full", "partial")]
    + ["groups:xcd", "groups:plain", "groups:xcd+ragged", "groups:plain+ragged", "C>512", "S>kT"])


def fingerprint(case):
    "a case's class as one tuple: two cases with the same fingerprint take the same arms with the same trip counts"
    n, C, H, W, G = case
    i = classify(n, C, H * W, G)
    return (i["walk"], i["float4_per_thread"], i["count_max"], i["count_min"], i["x4"], i["order"], i["ragged"],
            i["single_slice"], i["slices_beyond_block"], i["groups"], i["wide"])


# ---------------------------------------------------------------------------------------------------------------------
# integer inputs: every fp32 per-thread sum of the statistics kernel is exact

def int_input(case):
    n, C, H, W, G = case
    return ints((n, C, H, W), -8, 8, 7 + n * 1009 + C * 13 + H)


def grouped_view(x, G):
    "[n, C, H, W] -> [G, N, C, P]"
    n, C, H, W = x.shape
    return x.reshape(G, n // G, C, H * W)


def stats_budget(x, g):
    """The condition under which the statistics kernel owes exact sums: per slice, sum |x - K| and sum (x - K)^2 (K: the
    slice's first element, as the kernel) -- bounds of every thread's fp32 sums -- are within 2^24.  Returns the slices'
    (sum of x - K, sum of (x - K)^2, K, elements) as float64 [G, C, S] for ``chan_order``."""
    xg = grouped_view(x, g.G).long()
    a, b, k, cnt, wa = [], [], [], [], []
    for s, ns in enumerate(slice_images(g)):
        part = xg[:, s * g.NB:s * g.NB + ns]
        K = part[:, 0, :, 0]
        d = part - K[:, None, :, None]
        a.append(d.sum((1, 3))); b.append((d * d).sum((1, 3))); wa.append(d.abs().sum((1, 3)))
        k.append(K); cnt.append(torch.full_like(K, ns * g.P))
    a, b, k, cnt, wa = (torch.stack(t, -1).double() for t in (a, b, k, cnt, wa))
    assert_budget(wa, b)
    return a, b, k, cnt


def exact_stats(x, G):
    """Exact batch statistics of integer-valued ``x`` per (group, channel): the mean as ONE correctly rounded division of
    the exact sum, the biased and the unbiased variance as exact rationals rounded once.  float64 [G, C] each."""
    xg = grouped_view(x, G).long()
    M = xg.shape[1] * xg.shape[3]
    s, q = xg.sum((1, 3)), (xg * xg).sum((1, 3))
    mean = s.double() / float(M)
    var_b, var_u = torch.empty_like(mean), torch.empty_like(mean)
    for i, (si, qi) in enumerate(zip(s.flatten().tolist(), q.flatten().tolist())):
        m2 = Fraction(M * qi - si * si, M)                      # sum of squared deviations from the mean
        var_b.view(-1)[i] = float(m2 / M)
        var_u.view(-1)[i] = float(m2 / (M - 1)) if M > 1 else float(m2)
    return mean, var_b, var_u


def block_sum(v):
    "bn::block_sum2 on [..., 256] float64: the shuffle tree of every wave, then (w0 + w1) + (w2 + w3)"
    w = v.reshape(v.shape[:-1] + (4, 64)).copy()
    off = 32
    while off:
        w[..., :off] = w[..., :off] + w[..., off:2 * off]
        off >>= 1
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _by_thread(p):
    "[..., Q] -> thread t's running sum of elements t, t + 256, ... -> block tree"
    Q = p.shape[-1]
    pad = (-Q) % kT
    p = np.concatenate([p, np.zeros(p.shape[:-1] + (pad,))], -1).reshape(p.shape[:-1] + (-1, kT))
    acc = np.zeros(p.shape[:-2] + (kT,))
    for r in range(p.shape[-2]):
        acc = acc + p[..., r, :]
    return block_sum(acc)


def chan_from_partials(p_sum, p_m2, cnt, M):
    """apply_kernel's prologue in float64 NumPy, in its order (no FMA): mean = (sum of the partial sums) / M, then
    M2 = sum_q [M2_q + cnt_q (sum_q / cnt_q - mean)^2].  p_*: [..., Q]; cnt: [Q] or a scalar.  -> mean, var, unbiased"""
    p_sum, p_m2 = np.asarray(p_sum, np.float64), np.asarray(p_m2, np.float64)
    mean = _by_thread(p_sum) / M
    dm = p_sum / cnt - mean[..., None]
    var = np.maximum(_by_thread(p_m2 + cnt * dm * dm) / M, 0.0)
    return mean, var, (var * (M / (M - 1.0)) if M > 1 else var)


def chan_order(x, g):
    "stats_kernel + apply_kernel's prologue on integer ``x``: the slice-then-Chan order in float64 NumPy"
    a, b, K, cnt = (t.numpy() for t in stats_budget(x, g))
    return chan_from_partials(a + cnt * K, b - a * a / cnt, cnt[0, 0], float(g.N * g.P))


def equal_parts(x, G, parts):
    "caller-side partials of integer ``x``: float64 [C, G * parts, 2] (sum, M2 around the part's mean) of equal parts"
    xg = grouped_view(x, G).long().permute(0, 2, 1, 3)
    _, C, N, P = xg.shape
    assert (N * P) % parts == 0
    cnt = N * P // parts
    v = xg.reshape(G, C, parts, cnt)
    s, q = v.sum(-1).double(), (v * v).sum(-1).double()
    assert_budget(q)                                               # (integers far inside 2^53: s, q are exact)
    return torch.stack([s, q - s * s / cnt], -1).permute(1, 0, 2, 3).reshape(C, G * parts, 2).contiguous()


def random_parts(x, G, parts):
    "the same for any float ``x``, computed in float64"
    xg = grouped_view(x, G).double().permute(0, 2, 1, 3)
    _, C, N, P = xg.shape
    assert (N * P) % parts == 0
    v = xg.reshape(G, C, parts, N * P // parts)
    s = v.sum(-1)
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([s, m2], -1).permute(1, 0, 2, 3).reshape(C, G * parts, 2).contiguous()


def ulp32(v):
    "the fp32 spacing at |v| (v: float64 array-like of fp32-representable or rounded values)"
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# two-valued inputs: mean exactly 0, invstd exactly 2^-k, xhat = +-1

@functools.lru_cache(maxsize=2)
def two_valued(case):
    """x = +-2^k (k by channel) with exactly M / 2 of each sign per (group, channel) at shuffled positions; gamma a power
    of two of either sign, beta / residual / dy small integers (tensors [n, C, H, W] / [C], float32, CPU)"""
    n, C, H, W, G = case
    N, P = n // G, H * W
    M = N * P
    rng = np.random.default_rng(1000 * n + C)
    sign = np.tile(np.repeat(np.float32([1, -1]), M // 2), (G, C, 1))
    sign = rng.permuted(sign, axis=2)
    c = np.arange(C)
    k = c % 5 - 2
    x = sign * np.exp2(k).astype(np.float32)[None, :, None]
    x = torch.from_numpy(np.ascontiguousarray(x.reshape(G, C, N, P).transpose(0, 2, 1, 3))).reshape(n, C, H, W)
    gamma = torch.from_numpy((np.exp2((c + 1) % 3 - 1) * np.where((c // 2) % 2, -1.0, 1.0)).astype(np.float32))
    seed = 31 * n + C
    return dict(x=x, k=torch.from_numpy(k), gamma=gamma, beta=ints((C,), -3, 3, seed, nonzero=False),
                res=ints((n, C, H, W), -4, 4, seed + 1, nonzero=False), dy=ints((n, C, H, W), -3, 3, seed + 2), G=G, M=M)


# fp32 roundings of a dx element as bwd_dx_body writes it (a fused multiply-add only removes one):
#   mdb = (float)(a / M)                 1
#   mdg = (float)(b / M)                 2
#   k = gamma[c] * invstd                3
#   q - mean                             4
#   (q - mean) * invstd                  5
#   ... * mdg                            6
#   d - mdb                              7
#   (d - mdb) - ...                      8
#   k * (...)                            9
# each of relative size 2^-24 of a quantity that |k| (|d| + |mdb| + |xhat| |mdg|) bounds, and |xhat| = 1 here.
DX_ROUNDINGS = 9


def two_valued_ref(d, relu, residual, res=None):
    """float64 evaluation of forward and backward on ``two_valued`` data, with the exactness owed asserted: y, the ReLU
    mask's dz, dbeta and dgamma are fp32 numbers (and the sums' absolute terms stay within 2^24); dx gets a bound.
    ``res``: another residual than d["res"] (the shortcut BatchNorm's output)"""
    G, M = d["G"], d["M"]
    x = grouped_view(d["x"], G).double()
    cv = lambda t: t.double()[None, None, :, None]
    xhat = x * cv(torch.exp2(-d["k"].double()))
    assert bool((xhat.abs() == 1).all()) and bool((xhat.sum((1, 3)) == 0).all())       # mean 0, variance 4^k: exactly
    pre = cv(d["gamma"]) * xhat + cv(d["beta"])
    if residual:
        pre = pre + grouped_view(d["res"] if res is None else res, G).double()
    y = pre.clamp_min(0) if relu else pre
    dy = grouped_view(d["dy"], G).double()
    dz = dy * (y > 0) if relu else dy
    assert torch.equal(y.float().double(), y)
    kk = cv(d["gamma"]) * cv(torch.exp2(-d["k"].double()))
    dbeta, dgamma, dx, bound = bwd64(dz, xhat, kk, M)
    back = lambda t: t.reshape(d["x"].shape)
    return dict(y=back(y), dz=back(dz), dbeta=dbeta, dgamma=dgamma, dx=back(dx), bound=back(bound), xhat=xhat)


def bwd64(dz, xhat, kk, M):
    """float64 BatchNorm backward of [G, N, C, P] operands with xhat = +-1: (dbeta, dgamma) [G, C] -- asserted to be
    sums of integers within 2^24, so that every partial sum in any order is an fp32 number -- dx and its bound"""
    assert bool((xhat.abs() == 1).all()) and torch.equal(dz, dz.round())
    assert_budget(dz.abs().sum((1, 3)))
    dbeta, dgamma = dz.sum((1, 3)), (dz * xhat).sum((1, 3))
    mdb, mdg = dbeta[:, None, :, None] / M, dgamma[:, None, :, None] / M
    dx = kk * (dz - mdb - xhat * mdg)
    return dbeta, dgamma, dx, DX_ROUNDINGS * 2.0 ** -24 * kk.abs() * (dz.abs() + mdb.abs() + mdg.abs())


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' element-wise expressions in fp32 NumPy, operation by operation (NumPy never fuses a multiply-add)

def apply32(x, mean, scale, shift, r=None, relu=False):
    "apply_kernel: (x - mean) * scale + shift [+ r], max with 0 (arrays broadcastable, float32)"
    f = np.float32
    o = (x.astype(f) - f(mean)) * f(scale) + f(shift)
    if r is not None:
        o = o + r.astype(f)
    return np.maximum(o, f(0)) if relu else o


def bwd_dx32(d, q, mean, invstd, gamma, dbeta, dgamma, M):
    "bwd_dx_body: k * (d - mdb - ((q - mean) * invstd) * mdg) with mdb, mdg the float roundings of the fp64 means"
    f = np.float32
    mean, invstd = np.asarray(mean, f), np.asarray(invstd, f)
    mdb, mdg = (np.asarray(dbeta, np.float64) / M).astype(f), (np.asarray(dgamma, np.float64) / M).astype(f)
    k = np.asarray(gamma, f) * invstd
    return k * (d.astype(f) - mdb - ((q.astype(f) - mean) * invstd) * mdg)


def replay_reference(log, momentum, rm, rv):
    """the running-statistics recurrence as the kernels write it -- float storage, double update, no FMA:
    r <- (float)((1 - m) * (double) r + m * e) for every logged entry in order.  log [n, C, 2] float64"""
    rm, rv = rm.astype(np.float32).copy(), rv.astype(np.float32).copy()
    for e in np.asarray(log, np.float64):
        rm = ((1.0 - momentum) * rm.astype(np.float64) + momentum * e[:, 0]).astype(np.float32)
        rv = ((1.0 - momentum) * rv.astype(np.float64) + momentum * e[:, 1]).astype(np.float32)
    return rm, rv
