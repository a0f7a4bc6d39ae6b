"""Goodness of fit of the element-wise families that ``prior_fit.fit_marginal`` fits, on the device
(``csrc/gof_hip.inc``; C ABI ``sgmcmc_gof_cdf`` / ``sgmcmc_gof_statistics`` / ``sgmcmc_gof_ppf``, definitions in
``include/sgmcmc_hip.h``): which family the weights follow, and where a family fails -- what the reference's authors read
off Q-Q plots and distribution-function distances computed offline with scipy:

    cdf               F, 1 - F or their logarithms of norm / laplace / t / gennorm / dgamma (and uniform), formed in log
                      space: finite where scipy's ``logsf`` is ``-inf`` (``gennorm.logsf(30, 2)``, ``dgamma.logsf(800, 1)``)
    goodness_of_fit   per family the Kolmogorov-Smirnov distance (and where it is attained), the Cramer-von Mises W^2 and
                      the Anderson-Darling A^2 of the pooled elements of a stack, AIC / BIC, and the two sides of a Q-Q plot
    compare_families  the same per key of a ``storage.load_samples``-style mapping, with the families ranked

NO P-VALUES are returned: with parameters estimated from the same data (what ``fit_marginal`` does) the classical null
distributions of these statistics do not apply -- the fitted statistic is stochastically smaller, by an amount that
depends on the family and on the estimator.  The statistics RANK families on the same data and LOCATE misfit (KS and W^2
weigh the body, A^2 the tails, ``ks_at`` says where the largest gap is); they are not tests.

The ascending order comes from ``torch.sort`` of the flattened values; everything after it is fp64 in an order fixed by
the number of values, so two calls, or two permutations of the input, give the same bits.  One host synchronisation per
call; all families are scored in one launch that loads every value once.
"""
import collections
import ctypes
import math

import torch

from . import _hip, prior_fit
from .calibration import _stream

__all__ = ("GOF", "FAMILIES", "CRITERIA", "MAX_QQ_POINTS", "PARAMETER_RANGES", "cdf", "goodness_of_fit",
           "compare_families")

FAMILIES = ("uniform",) + prior_fit.FAMILIES
CRITERIA = ("ad", "cvm", "ks", "aic", "bic")
MAX_QQ_POINTS = _hip.GOF_MAX_QUANTILES
MAX_N = 2 ** 31 - 1
_CODE = {"uniform": _hip.GOF_UNIFORM, "norm": _hip.GOF_NORM, "laplace": _hip.GOF_LAPLACE, "t": _hip.GOF_T,
         "gennorm": _hip.GOF_GENNORM, "dgamma": _hip.GOF_DGAMMA}
# the accepted range of a family's shape parameter (SGMCMC_GOF_*_MIN / _MAX); loc finite, scale finite and > 0
PARAMETER_RANGES = {"t": _hip.GOF_DF_RANGE, "gennorm": _hip.GOF_BETA_RANGE, "dgamma": _hip.GOF_A_RANGE}

GOF = collections.namedtuple("GOF", "params n mean_loglik aic bic ks ks_plus ks_minus ks_at cvm ad qq")
GOF.__doc__ = ("params: the family's parameters in scipy's order; n: the number of values; mean_loglik, aic = 2 k - 2 n "
               "mean_loglik, bic = k log n - 2 n mean_loglik with k = len(params): floats, or None when no log-likelihood "
               "was given; ks = max(ks_plus, ks_minus), ks_at the value of x where it is attained, cvm = W^2, ad = A^2: "
               "floats; qq: None, or (probabilities (j - 1/2) / K, model quantiles, empirical quantiles), fp64 host tensors")


def _record(family, params):
    "the sgmcmc_gof_record of (family, params); every range is checked here, without touching the device"
    if family not in _CODE:
        raise ValueError(f"unknown family {family!r}: {FAMILIES} are supported")
    params = tuple(float(v) for v in params)
    want = 3 if family in PARAMETER_RANGES else 2
    if len(params) != want:
        raise ValueError(f"{family} takes {want} parameters in scipy's order, not {len(params)}")
    shape = params[0] if want == 3 else 0.0
    loc, scale = params[-2:]
    if not math.isfinite(loc) or not math.isfinite(scale) or not scale > 0.0:
        raise ValueError(f"{family}: loc = {loc} must be finite and scale = {scale} finite and > 0")
    if want == 3:
        lo, hi = PARAMETER_RANGES[family]
        if not lo <= shape <= hi:
            raise ValueError(f"{family}: shape parameter {shape} outside the accepted range [{lo}, {hi}]")
    rec = _hip.GofRecord()
    rec.family, rec.reserved, rec.shape, rec.loc, rec.scale = _CODE[family], 0, shape, loc, scale
    return rec, params


def _device_values(x, what):
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be a float32 or float64 tensor")
    if not x.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor (there is no CPU path)")
    if not 1 <= x.numel() <= MAX_N:
        raise ValueError(f"{what} has {x.numel()} elements: 1 .. {MAX_N} are supported")
    return x


def _is_f64(x):
    return _hip.F64 if x.dtype == torch.float64 else _hip.F32


def cdf(x, family, params, upper=False, log=False):
    """The distribution function F of ``family`` (``FAMILIES``) with ``params`` in scipy's order at the points x (any
    fp32 / fp64 device tensor or view) -> an fp64 device tensor of x's shape: F, or 1 - F (``upper``), or their
    logarithm (``log``).  The small side of ``loc`` is evaluated in log space and the large side derived from it, so
    ``log=True`` stays finite where the plain value underflows.  No host synchronisation."""
    rec, _ = _record(family, params)
    x = _device_values(x, "x")
    with torch.cuda.device(x.device):
        flat = x.reshape(-1).contiguous()
        out = torch.empty((4, flat.numel()), dtype=torch.float64, device=x.device)
        _hip.check(_hip.lib().sgmcmc_gof_cdf(flat.data_ptr(), _is_f64(flat), flat.numel(), ctypes.byref(rec),
                                             out.data_ptr(), _stream()), "sgmcmc_gof_cdf")
    return out[(2 if log else 0) + (1 if upper else 0)].reshape(x.shape)


def _non_finite(bad, n):
    return f"w has {bad} non-finite elements of {n}: the statistics are defined for finite values only"


def _normalise_fits(fits):
    "{family: params | (params, mean_loglik)} -> [(family, record, params, mean_loglik or None)]"
    out = []
    for fam, entry in fits.items():
        entry = tuple(entry)
        loglik = None
        if len(entry) == 2 and isinstance(entry[0], (tuple, list)):
            entry, loglik = tuple(entry[0]), None if entry[1] is None else float(entry[1])
        rec, params = _record(fam, entry)
        out.append((fam, rec, params, loglik))
    if not 1 <= len(out) <= _hip.GOF_MAX_RECORDS:
        raise ValueError(f"{len(out)} families: 1 .. {_hip.GOF_MAX_RECORDS} are scored in one call")
    return out


def goodness_of_fit(w, fits=None, families=prior_fit.FAMILIES, loc=0., qq_points=0):
    """w: any fp32 / fp64 device tensor or view; all its elements are pooled -> ``{family: GOF}``.

    ``fits`` defaults to ``prior_fit.fit_marginal(w, families, loc)``; a ``{family: params}`` or ``{family: (params,
    mean_loglik)}`` mapping scores hand-chosen parameters (and ``"uniform"``: (loc, scale)).  ``qq_points = K > 0`` adds the
    Q-Q plot at the probabilities (j - 1/2) / K.  A non-finite element raises a ``ValueError`` that says how many there are.

    With parameters estimated from the same data the classical p-values of these statistics do not apply, and none are
    returned (see the module's docstring): the statistics rank families and locate misfit."""
    if not isinstance(qq_points, int) or not 0 <= qq_points <= MAX_QQ_POINTS:
        raise ValueError(f"qq_points = {qq_points}: 0 .. {MAX_QQ_POINTS} are supported")
    if fits is None:
        families = tuple(families)
        unknown = [f for f in families if f not in prior_fit.FAMILIES]
        if unknown:
            raise ValueError(f"unknown families {unknown}: {prior_fit.FAMILIES} are fitted (pass fits= for {FAMILIES})")
        w = _device_values(w, "w")
        stack = w.reshape(1, -1) if w.dim() < 2 else w
        problem = None
        try:
            fits = prior_fit.fit_marginal(stack, families, loc)
        except (ValueError, ArithmeticError) as e:            # a fit that a NaN or a constant stack sent astray
            problem = e
        if problem is None:
            for fam, (params, _) in fits.items():
                if not all(math.isfinite(float(v)) for v in params) or not float(params[-1]) > 0.0:
                    problem = ValueError(f"the fitted {fam} is degenerate, params = {tuple(float(v) for v in params)}: "
                                         "w has no spread")
                    break
        if problem is not None:
            bad = int((~torch.isfinite(w)).sum().item())
            if bad:
                raise ValueError(_non_finite(bad, w.numel())) from problem
            if isinstance(problem, ValueError):
                raise problem
            raise ValueError(f"fit_marginal failed on w: {problem!r}") from problem
    entries = _normalise_fits(fits)
    w = _device_values(w, "w")
    n, count, K = w.numel(), len(entries), qq_points
    lib = _hip.lib()
    records = (_hip.GofRecord * count)(*[rec for _, rec, _, _ in entries])
    with torch.cuda.device(w.device):
        ordered, _ = torch.sort(w.reshape(-1))
        work = torch.empty(lib.sgmcmc_gof_workspace_doubles(n), dtype=torch.float64, device=w.device)
        out = torch.empty(count * _hip.GOF_OUT + (count + 1) * K, dtype=torch.float64, device=w.device)
        _hip.check(lib.sgmcmc_gof_statistics(ordered.data_ptr(), _is_f64(ordered), n, records, count, work.data_ptr(),
                                             out.data_ptr(), _stream()), "sgmcmc_gof_statistics")
        if K:
            model = out[count * _hip.GOF_OUT:]
            _hip.check(lib.sgmcmc_gof_ppf(ordered.data_ptr(), _is_f64(ordered), n, records, count, K, model.data_ptr(),
                                          model[count * K:].data_ptr(), _stream()), "sgmcmc_gof_ppf")
        host = out.cpu()                                     # the call's one synchronisation
    stats = host[:count * _hip.GOF_OUT].reshape(count, _hip.GOF_OUT)
    bad = int(stats[0, 7])
    if bad:
        raise ValueError(_non_finite(bad, n))
    result = {}
    if K:
        probs = (2.0 * torch.arange(1, K + 1, dtype=torch.float64) - 1.0) / (2.0 * K)
        quantiles = host[count * _hip.GOF_OUT:].reshape(count + 1, K)
    for f, (fam, _, params, loglik) in enumerate(entries):
        D, Dp, Dm, _, at, W2, A2, _ = (float(v) for v in stats[f])
        aic = bic = None
        if loglik is not None:
            aic = 2.0 * len(params) - 2.0 * n * loglik
            bic = len(params) * math.log(n) - 2.0 * n * loglik
        qq = (probs, quantiles[f].clone(), quantiles[count].clone()) if K else None
        result[fam] = GOF(params, n, loglik, aic, bic, D, Dp, Dm, at, W2, A2, qq)
    return result


def compare_families(stacks, families=("norm", "laplace", "dgamma"), criterion="ad"):
    """stacks: ``"<module>.weight_prior.p"`` -> [S, *shape], what ``prior_fit.fit_prior_data`` takes -> ``{key: (table,
    ranking)}`` with ``table = goodness_of_fit(stack, families=families)`` and ``ranking`` the families from the best
    (smallest ``criterion``: "ad", "cvm", "ks", "aic" or "bic") to the worst.  The keys are those of ``fit_prior_data``'s
    fits table.  The ranking compares families on the same data; it is not a test (no p-values: module docstring)."""
    if criterion not in CRITERIA:
        raise ValueError(f"criterion = {criterion!r}: one of {CRITERIA}")
    families = tuple(families)
    unknown = [f for f in families if f not in prior_fit.FAMILIES]
    if unknown:
        raise ValueError(f"unknown families {unknown}: {prior_fit.FAMILIES} are supported")
    out = {}
    for key, w in stacks.items():
        table = goodness_of_fit(w, families=families)
        out[key] = (table, tuple(sorted(table, key=lambda fam: getattr(table[fam], criterion))))
    return out
