"""Fitting the data-driven priors to stacks of weight samples on the device (``csrc/fit_hip.inc``; C ABI
``sgmcmc_fit_moments`` / ``sgmcmc_fit_mvt_init`` / ``sgmcmc_fit_mvt_iterate`` / ``sgmcmc_fit_abs_stats``, definitions in
``include/sgmcmc_hip.h``) -- what the reference's authors did offline with numpy and scipy, and what ``storage.py``'s
``[S, *shape]`` stacks are the input of:

    moments         mean, covariance, skewness and excess kurtosis of the P-position vectors (filters) of a stack
    fit_mvt         maximum likelihood of ``distributions.MultivariateT`` by EM (Liu & Rubin 1995; the parameter-expanded
                    scatter update of Kent, Tyler & Vardi 1994): ``MVTFit.prior(shape)`` is the ``prior.MultivariateT``
    fit_marginal    element-wise maximum likelihood of norm / laplace / t / gennorm / dgamma, parameters in scipy's order
    fit_prior_data  the two tables the ``DataDriven*ClassificationConvNet``s read (``prior_data=``)

A stack is read in place through its strides (fp32 or fp64, any view), never copied into a permuted layout.  Everything
runs in fp64 in an order fixed by the sizes (counts in integers), so two calls give the same bits.  ``moments`` does not
synchronise with the host; ``fit_mvt`` reads a flag every ``check_every`` iterations (its result does not depend on it).
"""
import collections
import math

import numpy as np
import torch

from . import _hip
from .calibration import _stream

__all__ = ("Moments", "MVTFit", "moments", "fit_mvt", "fit_marginal", "fit_prior_data", "abs_stats", "tile_events",
           "FAMILIES")

MAX_P = _hip.FILTER_MAX_P                # positions of a vector (SGMCMC_FILTER_MAX_P)
MAX_F = _hip.FIT_TILE_ROWS               # vectors of an event
TILE_DOUBLES = _hip.FIT_TILE_DOUBLES     # an event's F (P | 1) doubles must fit one LDS tile
MAX_VECTORS = 2 ** 31 - 1
MAX_EVENT_DIMS = 4
FAMILIES = ("norm", "laplace", "t", "gennorm", "dgamma")

Moments = collections.namedtuple("Moments", "n mean cov skew kurt var pooled_mean pooled_var pooled_skew pooled_kurt "
                                            "zero_variance")
Moments.__doc__ = ("n: the number of vectors (int); fp64 tensors on the device: mean [P], cov [P, P] (divided by n - "
                   "ddof), skew, kurt, var [P] (population definitions; excess kurtosis) and their pooled values over "
                   "all n P elements (0-d); zero_variance [P] (bool): columns whose variance is 0, whose skew and kurt "
                   "are NaN")


class MVTFit(collections.namedtuple("MVTFit", "loc scale_tril df loglik trace iterations converged df_at_bound "
                                              "event_dim permute")):
    """loc [P], scale_tril [P, P] = chol(S df / (df - 2)) (the covariance's factor, ``distributions.MultivariateT``'s
    parametrisation) and trace [iterations] (the log-likelihood before each iteration): fp64 tensors on the host; df and
    loglik (the total at the returned parameters): floats; iterations: int; converged, df_at_bound: bools."""
    __slots__ = ()

    def prior(self, shape):
        "the fitted ``prior.MultivariateT`` of a parameter of this shape"
        from . import prior
        if self.event_dim is None:
            raise ValueError("an element-wise fit (P = 1, event_dim = None) has no multivariate event: pass event_dim")
        dt = torch.get_default_dtype()
        return prior.MultivariateT(shape, self.loc.to(dt), self.scale_tril.to(dt), self.df, self.event_dim, self.permute)


def tile_events(P, F):
    "events of one LDS tile (``fit::tile_events``: a function of the sizes alone)"
    return max(1, min(TILE_DOUBLES // (F * (P | 1)), MAX_F // F))


def _collapse(dims):
    "drop dimensions of size 1 and merge neighbours that one stride walks"
    out = []
    for size, stride in dims:
        if size == 1:
            continue
        if out and out[-1][1] == size * stride:
            out[-1] = (out[-1][0] * size, stride)
        else:
            out.append((size, stride))
    return out


def _geometry(w, P, event_dim, permute):
    "(sgmcmc_fit_geometry, event_dim, permute) of the stack w [S, *shape]; every limit is checked here"
    if not isinstance(w, torch.Tensor) or w.dim() < 2 or w.dtype not in (torch.float32, torch.float64):
        raise ValueError("w must be a float32 or float64 [S, *shape] tensor")
    if w.numel() == 0:
        raise ValueError("w is empty")
    if not isinstance(P, int) or not 1 <= P <= MAX_P:
        raise ValueError(f"P = {P}: 1 .. {MAX_P} positions are supported")
    shape = tuple(w.shape[1:])
    nd = len(shape)
    ident = tuple(range(nd))
    permute = ident if permute is None else tuple(int(i) for i in permute)
    if sorted(permute) != list(ident):
        raise ValueError(f"permute {permute} is not a permutation of the {nd} dimensions")
    if permute != ident and not (nd == 4 and permute == (1, 0, 2, 3) and event_dim == 3):
        raise ValueError(f"unsupported permutation {permute} with event_dim = {event_dim}: the identity, or (1, 0, 2, 3) "
                         "with event_dim = 3 on a 4-D shape, are supported")
    dims = [(shape[p], w.stride(1 + p)) for p in permute]
    if event_dim is None:                                   # the trailing dimensions that hold P elements: F = 1
        k, prod = 0, 1
        while prod < P and k < nd:
            k += 1
            prod *= dims[nd - k][0]
        if prod != P:
            raise ValueError(f"P = {P} does not divide the event: no trailing dimensions of {shape} hold {P} elements")
        n_event = k
    else:
        if not isinstance(event_dim, int) or not 1 <= event_dim <= nd:
            raise ValueError(f"event_dim must be in [1, {nd}], not {event_dim}")
        n_event = event_dim
    batch, event = [(w.shape[0], w.stride(0))] + dims[:nd - n_event], dims[nd - n_event:]
    D = math.prod(s for s, _ in event)
    if D % P:
        raise ValueError(f"P = {P} does not divide the event of {D} elements")
    # the trailing P elements of the event are a vector's positions; a dimension may be cut in two
    pos, prod = [], 1
    while prod < P:
        size, stride = event.pop()
        if (prod * size) <= P and P % (prod * size) == 0:
            pos.insert(0, (size, stride))
            prod *= size
        else:
            inner = P // prod
            if P % prod or size % inner:
                raise ValueError(f"P = {P} does not divide the event: its trailing dimensions do not split into vectors "
                                 f"of {P} elements")
            pos.insert(0, (inner, stride))
            event.append((size // inner, stride * inner))
            prod *= inner
    F = D // P
    if F > MAX_F or F * (P | 1) > TILE_DOUBLES:
        raise ValueError(f"{F} vectors of {P} positions per event: at most {MAX_F} vectors and {TILE_DOUBLES} "
                         "= F (P | 1) staged numbers are supported")
    fdims = _collapse(event)
    if len(fdims) > 1:
        raise ValueError("the vectors of an event must lie at one stride (a view that breaks it is not supported)")
    batch = _collapse(batch)
    if len(batch) > MAX_EVENT_DIMS:
        raise ValueError(f"the events span {len(batch)} strided dimensions: at most {MAX_EVENT_DIMS} are supported")
    events = math.prod(s for s, _ in batch)
    if events * F > MAX_VECTORS:
        raise ValueError(f"{events * F} vectors: at most {MAX_VECTORS} are supported")
    g = _hip.FitGeometry()
    g.P, g.F, g.events = P, F, events
    g.f_stride = fdims[0][1] if fdims else 0
    g.f_major = int(bool(fdims) and bool(batch) and g.f_stride > batch[-1][1])
    batch = [(1, 0)] * (MAX_EVENT_DIMS - len(batch)) + batch
    for k, (size, stride) in enumerate(batch):
        g.size[k], g.stride[k] = size, stride
    offsets = [0]
    for size, stride in pos:
        offsets = [o + i * stride for o in offsets for i in range(size)]
    for a, o in enumerate(offsets):
        g.pos[a] = o
    return g, (n_event if n_event else None), permute


def _on_device(w):
    if not w.is_cuda:
        raise ValueError("w must be a CUDA tensor (there is no CPU path)")
    return w.device


class _Workspace:
    "the buffers of the entry points for one geometry"

    def __init__(self, g, dev):
        self.blocks = _hip.lib().sgmcmc_fit_blocks(g.P, g.F, g.events)
        if self.blocks < 1:
            raise ValueError("sgmcmc_fit_blocks refused the shape")
        self.part = torch.empty((self.blocks + 1) * _hip.FIT_PART, dtype=torch.float64, device=dev)
        self.counts = torch.empty(self.blocks, dtype=torch.int64, device=dev)


def _dtype(w):
    return _hip.F32 if w.dtype == torch.float32 else _hip.F64


def _moments_table(w, g, ddof, work):
    P = g.P
    out = torch.empty(P * P + 4 * P + 4, dtype=torch.float64, device=w.device)
    bad = torch.empty(1, dtype=torch.int64, device=w.device)
    _hip.check(_hip.lib().sgmcmc_fit_moments(w.data_ptr(), _dtype(w), g, ddof, work.part.data_ptr(),
                                             work.counts.data_ptr(), out.data_ptr(), bad.data_ptr(), _stream()),
               "sgmcmc_fit_moments")
    return out, bad


def moments(w, P, event_dim=None, permute=None, ddof=1):
    """w [S, *shape] -> ``Moments`` of its n vectors of P positions (``event_dim`` / ``permute`` as ``fit_mvt``; they only
    name which elements form a vector).  The second to fourth moments are centred on a shift taken from the data, so a
    column whose mean is far from 0 keeps its digits.  A NaN or Inf anywhere makes every output NaN.  One pass and one
    workgroup that adds its partial sums; no host synchronisation.  For more than 25 positions -- the rows, columns or
    channels of a layer -- ``weight_correlation.covariance`` forms the covariance and correlation of up to 1,024 variables."""
    g, _, _ = _geometry(w, P, event_dim, permute)
    n = g.events * g.F
    if not isinstance(ddof, int) or not 0 <= ddof < n:
        raise ValueError(f"ddof = {ddof}: 0 .. n - 1 = {n - 1} is supported")
    dev = _on_device(w)
    with torch.cuda.device(dev):
        out, _ = _moments_table(w, g, ddof, _Workspace(g, dev))
    mean, cov, skew, kurt, var, pooled = out.split([P, P * P, P, P, P, 4])
    return Moments(n, mean, cov.reshape(P, P), skew, kurt, var, *pooled, var == 0)


def _check_fit_args(df_init, df_bounds, max_iter, tol, check_every):
    lo, hi = (float(b) for b in df_bounds)
    if not 2.0 < lo <= hi or not math.isfinite(hi):
        raise ValueError(f"df_bounds = {tuple(df_bounds)}: 2 < lower <= upper is needed (the covariance-parametrised t "
                         "needs df > 2)")
    if not lo <= float(df_init) <= hi:
        raise ValueError(f"df_init = {df_init} lies outside df_bounds = ({lo}, {hi})")
    if not isinstance(max_iter, int) or not 1 <= max_iter <= 2 ** 30:
        raise ValueError(f"max_iter = {max_iter}: 1 .. 2^30 is supported")
    if not float(tol) >= 0.0:
        raise ValueError("tol must be >= 0")
    if not isinstance(check_every, int) or check_every < 1:
        raise ValueError("check_every must be a positive integer")
    return lo, hi


def fit_mvt(w, P, event_dim=None, permute=None, df_init=5., df_bounds=(2.01, 1e4), max_iter=500, tol=1e-10,
            check_every=8):
    """Maximum likelihood of ``distributions.MultivariateT`` on the stack w [S, *shape] -> ``MVTFit``.

    ``permute`` and ``event_dim`` mean what they mean for ``prior.MultivariateT``: after permuting ``shape`` the trailing
    ``event_dim`` dimensions form one event of F vectors of P consecutive positions that share one mixing variable; the
    S samples multiply the events.  ``event_dim=None`` takes the trailing dimensions that hold P elements (F = 1).
    Supported: unpermuted trailing events, and ``permute=(1, 0, 2, 3)`` with ``event_dim=3``.

    EM in the standard parametrisation (include/sgmcmc_hip.h, definition 2): one pass over the stack and one
    single-workgroup update per iteration, until (loc, scatter, df) move by at most ``tol`` relative, or ``max_iter``.
    A device flag turns the launches after that into no-ops; the host reads it every ``check_every`` iterations."""
    g, event_dim, permute = _geometry(w, P, event_dim, permute)
    lo, hi = _check_fit_args(df_init, df_bounds, max_iter, tol, check_every)
    dev = _on_device(w)
    lib = _hip.lib()
    with torch.cuda.device(dev):
        work = _Workspace(g, dev)
        mom, _ = _moments_table(w, g, 0, work)
        state = torch.empty(_hip.FIT_STATE, dtype=torch.float64, device=dev)
        trace = torch.zeros(max_iter, dtype=torch.float64, device=dev)
        _hip.check(lib.sgmcmc_fit_mvt_init(P, mom.data_ptr(), mom[P:].data_ptr(), float(df_init), state.data_ptr(),
                                           _stream()), "sgmcmc_fit_mvt_init")
        left = max_iter + 1                                  # the last pair writes loglik at the returned parameters
        while left > 0:
            k = min(check_every, left)
            _hip.check(lib.sgmcmc_fit_mvt_iterate(w.data_ptr(), _dtype(w), g, k, max_iter, float(tol), lo, hi,
                                                  work.part.data_ptr(), work.counts.data_ptr(), state.data_ptr(),
                                                  trace.data_ptr(), _stream()), "sgmcmc_fit_mvt_iterate")
            left -= k
            if state[0].item() == 2.0:
                break
        rec, trace = state.cpu(), trace.cpu()
    iterations, df = int(rec[1]), float(rec[3])
    loc = rec[8:8 + P].clone()
    S = rec[8 + MAX_P + MAX_P * MAX_P:][:P * P].reshape(P, P)
    if math.isfinite(df) and bool(torch.isfinite(S).all()):
        scale_tril = torch.linalg.cholesky(S * (df / (df - 2.0)))
    else:
        scale_tril = torch.full((P, P), math.nan, dtype=torch.float64)
    return MVTFit(loc, scale_tril, df, float(rec[5]), trace[:iterations].clone(), iterations, bool(rec[2]), bool(rec[6]),
                  event_dim, permute)


def abs_stats(w, loc=0., beta=1.):
    """(n, zeros, sums): over the elements of w with d = |x - loc| > 0 the fp64 sums [d, log d, d^beta, d^beta log d,
    d^beta log^2 d] (a host tensor) and the integer count of d == 0.  Two launches, one host synchronisation."""
    if not float(beta) > 0.0 or not math.isfinite(float(loc)):
        raise ValueError("beta must be > 0 and loc finite")
    if isinstance(w, torch.Tensor) and w.dim() == 1:
        w = w.unsqueeze(0)
    g, _, _ = _geometry(w, 1, None, None)
    dev = _on_device(w)
    with torch.cuda.device(dev):
        work = _Workspace(g, dev)
        out = torch.empty(5, dtype=torch.float64, device=dev)
        zeros = torch.empty(1, dtype=torch.int64, device=dev)
        _hip.check(_hip.lib().sgmcmc_fit_abs_stats(w.data_ptr(), _dtype(w), g, float(loc), float(beta),
                                                   work.part.data_ptr(), work.counts.data_ptr(), out.data_ptr(),
                                                   zeros.data_ptr(), _stream()), "sgmcmc_fit_abs_stats")
        return g.events, int(zeros.item()), out.cpu()


def _digamma(x):
    "the kernels' digamma on the host: recurrence up to x >= 10, then the asymptotic series through B_14"
    r = 0.0
    while x < 10.0:
        r -= 1.0 / x
        x += 1.0
    f = 1.0 / (x * x)
    t = f * (1 / 12 - f * (1 / 120 - f * (1 / 252 - f * (1 / 240 - f * (1 / 132 - f * (691 / 32760 - f * (1 / 12)))))))
    return r + (math.log(x) - 0.5 / x - t)


def _trigamma(x):
    r = 0.0
    while x < 10.0:
        r += 1.0 / (x * x)
        x += 1.0
    f = 1.0 / (x * x)
    t = (f / x) * (1 / 6 - f * (1 / 30 - f * (1 / 42 - f * (1 / 30 - f * (5 / 66 - f * (691 / 2730 - f * (7 / 6)))))))
    return r + (1.0 / x + 0.5 * f + t)


def _laplace_params(n, sums, loc):
    b = float(sums[0]) / n
    return (loc, b), -math.log(2.0 * b) - 1.0


def _dgamma_params(n, zeros, sums, loc):
    """the double-Gamma at a given loc: log a - psi(a) = log mean|d| - mean log|d| (Minka's start and generalised Newton
    step), scale = mean|d| / a.  An element equal to loc has no log|d|: refused."""
    if zeros:
        raise ValueError(f"dgamma: {zeros} of the {n} elements equal loc = {loc}, where log|x - loc| is undefined; at most 0 "
                         "such elements are supported (fit the other families, or drop them)")
    m1, ml = float(sums[0]) / n, float(sums[1]) / n
    s = math.log(m1) - ml
    a = (3.0 - s + math.sqrt((s - 3.0) * (s - 3.0) + 24.0 * s)) / (12.0 * s)
    for _ in range(100):
        an = 1.0 / (1.0 / a + ((math.log(a) - _digamma(a)) - s) / (a * a * (1.0 / a - _trigamma(a))))
        done = abs(an - a) <= 1e-14 * an
        a = an
        if done:
            break
    scale = m1 / a
    return (a, loc, scale), (((a - 1.0) * ml - m1 / scale) - math.log(2.0)) - math.lgamma(a) - a * math.log(scale)


def _gennorm_profile(beta, n, sums):
    "the profile score g(beta) of the generalised normal at a given location, and g'(beta)"
    sp, spl, spll = (float(v) for v in sums[2:5])
    r, inv = spl / sp, 1.0 / beta
    la = math.log(beta * sp / n)
    g = ((1.0 + _digamma(inv) * inv) - r) + la * inv
    dg = (((-_digamma(inv) * inv * inv - _trigamma(inv) * inv * inv * inv) - (spll / sp - r * r))
          + (inv + r) * inv) - la * inv * inv
    return g, dg


def _gennorm_params(stats_at, n, loc):
    "Newton on the profile score from beta = 1, one ``stats_at(beta)`` (one launch) per evaluation; steps kept in [b/2, 2b]"
    beta = 1.0
    for _ in range(100):
        g, dg = _gennorm_profile(beta, n, stats_at(beta))
        bn = beta - g / dg
        if not bn > beta / 2:
            bn = beta / 2
        elif bn > 2 * beta:
            bn = 2 * beta
        done = abs(bn - beta) <= 1e-12 * bn
        beta = bn
        if done:
            break
    sp = float(stats_at(beta)[2])
    alpha = math.exp(math.log(beta * sp / n) / beta)
    return (beta, loc, alpha), ((math.log(beta) - math.log(2.0 * alpha)) - math.lgamma(1.0 / beta)) - 1.0 / beta


def fit_marginal(w, families=FAMILIES, loc=0.):
    """Element-wise maximum likelihood over every element of w -> ``{family: (params, mean_loglik)}``, params in
    ``scipy.stats``' order: norm (loc, scale), laplace (loc, scale), t (df, loc, scale), gennorm (beta, loc, scale),
    dgamma (a, loc, scale).  norm and t have a free location; laplace, gennorm and dgamma are fitted at the GIVEN
    ``loc`` (a free location makes the double-Gamma likelihood unbounded for a < 1).  Elements equal to ``loc`` have no
    ``log|d|``: with any, dgamma raises a ``ValueError`` that says how many; laplace and gennorm (0^beta log 0 = 0)
    proceed."""
    families = tuple(families)
    unknown = [f for f in families if f not in FAMILIES]
    if unknown:
        raise ValueError(f"unknown families {unknown}: {FAMILIES} are supported")
    loc = float(loc)
    if isinstance(w, torch.Tensor) and w.dim() == 1:
        w = w.unsqueeze(0)
    out = {}
    base = None
    for fam in families:
        if fam == "norm":
            m = moments(w, 1, ddof=0)
            mean, var = float(m.mean[0]), float(m.var[0])
            out[fam] = ((mean, math.sqrt(var)), -(math.log(2.0 * math.pi * var) + 1.0) / 2.0 if var > 0 else math.nan)
        elif fam == "t":
            f = fit_mvt(w, 1)
            scale = float(f.scale_tril[0, 0]) * math.sqrt((f.df - 2.0) / f.df) if math.isfinite(f.df) else math.nan
            out[fam] = ((f.df, float(f.loc[0]), scale), f.loglik / w.numel())
        else:
            if base is None:
                base = abs_stats(w, loc, 1.0)
            n, zeros, sums = base
            if fam == "laplace":
                out[fam] = _laplace_params(n, sums, loc)
            elif fam == "dgamma":
                out[fam] = _dgamma_params(n, zeros, sums, loc)
            else:
                out[fam] = _gennorm_params(lambda b: abs_stats(w, loc, b)[2], n, loc)
    return out


def fit_prior_data(stacks, families=("norm", "laplace", "dgamma")):
    """stacks: ``"<module>.weight_prior.p"`` / ``"<module>.bias_prior.p"`` -> [S, *shape] (what ``storage.load_samples``
    returns, minus its bookkeeping keys) -> ``{MEAN_COVS_FILE: ..., FITS_FILE: ...}`` in the layout of the reference's
    tables, i.e. a ``prior_data=`` of the ``DataDriven*ClassificationConvNet``s: convolution weights [S, Cout, Cin, kh,
    kw] -> (mean [kh kw] float32, cov [kh kw, kh kw] float64, as ``numpy.cov``); everything else -> (mean, var) scalars;
    the fits table -> {key: {family: params}} at loc = 0."""
    from .models.data_driven import FITS_FILE, MEAN_COVS_FILE
    mean_covs, fits = {}, {}
    for key, w in stacks.items():
        if isinstance(w, torch.Tensor) and w.dim() == 5:
            m = moments(w, w.shape[-1] * w.shape[-2])
            mean_covs[key] = (m.mean.cpu().numpy().astype(np.float32), m.cov.cpu().numpy())
        else:
            if isinstance(w, torch.Tensor) and w.dim() == 1:
                w = w.unsqueeze(0)
            m = moments(w, 1)
            mean_covs[key] = (np.float64(m.mean[0].item()), np.float64(m.cov[0, 0].item()))
        fits[key] = {fam: tuple(float(v) for v in params) for fam, (params, _) in fit_marginal(w, families).items()}
    return {MEAN_COVS_FILE: mean_covs, FITS_FILE: fits}
