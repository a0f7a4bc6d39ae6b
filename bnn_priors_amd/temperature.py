"""Does a chain sample at the temperature it claims?  The diagnostics that the reference reads off plots
(``bnn_priors/plot.py:14-141``: ``_gamma_confidence``, ``kinetic_temperature_intervals``, ``weighted_var_se``,
``temperature_stderr``, ``ewma``), computed on the device from the columns every runner logs -- ``est_temperature/<name>``,
``est_config_temp/<name>``, ``temperature`` (``csrc/temper_hip.inc``; C ABI ``sgmcmc_temper_*``, definitions in
``include/sgmcmc_hip.h``):

    chi2_interval         per tensor and confidence level the central interval of T^ / T ~ chi^2_d / d, d the tensor's size
    chi2_quantile         the r at which a tail of chi^2_d / d has a given probability, given plainly or as a logarithm
    chi2_tails            P(chi^2_d / d <= r), its complement, or their logarithms, at any d in [1, 2^31 - 1]
    kinetic_coverage      per metrics step the share of tensors inside their intervals (and its EWMA), per tensor the number
                          of steps inside: at the target temperature the share at level c is c
    weighted_temperature  the size-weighted mean temperature per step with Cochran's (1977) standard error
    ewma                  y_0 = x_0, y_t = (1 - alpha) x_t + alpha y_(t-1) along the last dimension
    temperature_report    all of it from a ``MemoryMetrics``, an ``HDF5Metrics`` file or a dict of columns

A tensor with d elements has a = d / 2 up to 1e9, far beyond where a series or a continued fraction of the incomplete gamma
function ends: the kernel switches to Temme's uniform expansion there (the switch points and the measured error on each
side are in ``csrc/temper_hip.inc``; 32 eps of the log-tail are held against a 50-digit restatement in
``tests/test_temperature.py``).  Everything is fp64 and deterministic: no floating-point atomics, sums in an order fixed by
the shapes, the per-tensor coverage as integer counts.  Arguments are checked on the host before anything is launched;
CPU tensors are refused -- there is no CPU path.
"""
import numpy as np
import torch

from . import _hip
from .calibration import _stream

__all__ = ("CONFIDENCES", "MAX_LEVELS", "MAX_SIZE", "get_sizes", "chi2_interval", "chi2_quantile", "chi2_tails",
           "kinetic_coverage", "weighted_temperature", "ewma", "temperature_report")

CONFIDENCES = (.05, .25, .5, .75, .95)
MAX_LEVELS = _hip.TEMPER_MAX_LEVELS
MAX_SIZE = 2 ** 31 - 1
_KINETIC, _CONFIG = "est_temperature", "est_config_temp"


def get_sizes(model):
    "``{name: numel}`` of the model's state dict (plot.py:14): the d of every tensor's chi^2_d law"
    return {k: p.numel() for k, p in model.state_dict().items()}


def _device(device):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError(f"device = {device}: a CUDA device is needed (there is no CPU path)")
    return device


def _sizes(sizes):
    "a sequence (or mapping's values, or tensor) of tensor sizes -> list of ints, each in [1, 2^31 - 1]"
    if isinstance(sizes, dict):
        sizes = list(sizes.values())
    if isinstance(sizes, torch.Tensor):
        sizes = sizes.detach().cpu().reshape(-1).tolist()
    if isinstance(sizes, (int, np.integer)):
        sizes = [sizes]
    out = []
    for d in sizes:
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) and not (isinstance(d, float) and d == int(d)):
            raise ValueError(f"sizes must be integers, not {d!r}")
        d = int(d)
        if not 1 <= d <= MAX_SIZE:
            raise ValueError(f"size {d} outside [1, {MAX_SIZE}]")
        out.append(d)
    if not out:
        raise ValueError("sizes is empty")
    return out


def _sizes_tensor(sizes, device):
    return torch.tensor(_sizes(sizes), dtype=torch.int64, device=device)


def _confidences(confidences):
    c = [float(v) for v in (confidences if isinstance(confidences, (tuple, list, np.ndarray)) else [confidences])]
    if not 1 <= len(c) <= MAX_LEVELS:
        raise ValueError(f"{len(c)} confidence levels: 1 .. {MAX_LEVELS} are supported")
    if not all(0.0 < v < 1.0 for v in c):
        raise ValueError(f"confidences = {c}: each must lie in (0, 1)")
    return c


def _table(x, what, dim):
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be a float32 or float64 tensor")
    if not x.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor (there is no CPU path)")
    if x.dim() != dim:
        raise ValueError(f"{what} must have {dim} dimensions, not {x.dim()}")
    if not 1 <= x.numel() <= MAX_SIZE:
        raise ValueError(f"{what} has {x.numel()} elements: 1 .. {MAX_SIZE} are supported")
    return x


def _is_f64(x):
    return _hip.F64 if x.dtype == torch.float64 else _hip.F32


def _temperature(temperature, S, device):
    "-> (fp64 device tensor, element stride): [S] or one value"
    if isinstance(temperature, torch.Tensor):
        if not temperature.is_cuda:
            raise ValueError("temperature must be a CUDA tensor or a number (there is no CPU path)")
        t = temperature.to(torch.float64).reshape(-1).contiguous()
    else:
        t = torch.tensor([float(temperature)], dtype=torch.float64, device=device)
    if t.numel() not in (1, S):
        raise ValueError(f"temperature has {t.numel()} elements: 1 or {S} (one per step) are accepted")
    return t, (1 if t.numel() == S and S > 1 else 0)


def chi2_interval(sizes, confidences=CONFIDENCES, device=None):
    """``[K, C, 2]`` fp64 on the device: (lower, upper) of the central interval of chi^2_d / d with mass ``confidences[c]``
    for d = ``sizes[k]`` -- plot.py's ``_gamma_confidence``, i.e. ``chi2.ppf((1 -+ c) / 2, df=d, scale=1 / d)``, for any d
    in [1, 2^31 - 1].  The upper end is solved on the upper tail 1 - (1 + c) / 2, which is exact.  No synchronisation."""
    device = _device(device)
    c = np.asarray(_confidences(confidences), dtype=np.float64)
    value = np.stack([(1.0 - c) / 2.0, 1.0 - (1.0 + c) / 2.0], axis=1).reshape(-1)      # entry 2 c + side
    upper = np.tile(np.array([0, 1], dtype=np.int32), len(c))
    with torch.cuda.device(device):
        d = _sizes_tensor(sizes, device)
        v = torch.from_numpy(value).to(device)
        u = torch.from_numpy(upper).to(device)
        out = torch.empty((d.numel(), len(c), 2), dtype=torch.float64, device=device)
        _hip.check(_hip.lib().sgmcmc_temper_quantile(d.data_ptr(), d.numel(), v.data_ptr(), u.data_ptr(), v.numel(), 0,
                                                     out.data_ptr(), _stream()), "sgmcmc_temper_quantile")
    return out


def chi2_quantile(sizes, value, upper=False, log=False, device=None):
    """``[K, M]`` fp64: the r = chi^2_d / d at which the lower tail P (``upper``: the upper tail Q) of d = ``sizes[k]``
    equals ``value[m]`` (``log``: its logarithm, for tails below the smallest double)."""
    device = _device(device)
    value = np.atleast_1d(np.asarray(value, dtype=np.float64)).reshape(-1)
    if value.size < 1 or np.isnan(value).any() or ((value > 0).any() if log else ((value < 0) | (value > 1)).any()):
        raise ValueError("value must hold probabilities in [0, 1] (log: their logarithms, <= 0)")
    with torch.cuda.device(device):
        d = _sizes_tensor(sizes, device)
        v = torch.from_numpy(value).to(device)
        u = torch.full((value.size,), 1 if upper else 0, dtype=torch.int32, device=device)
        out = torch.empty((d.numel(), value.size), dtype=torch.float64, device=device)
        _hip.check(_hip.lib().sgmcmc_temper_quantile(d.data_ptr(), d.numel(), v.data_ptr(), u.data_ptr(), value.size,
                                                     1 if log else 0, out.data_ptr(), _stream()),
                   "sgmcmc_temper_quantile")
    return out


def _tails(est, temperature, sizes):
    est = _table(est, "ratio", 2)
    S, K = est.shape
    with torch.cuda.device(est.device):
        d = _sizes_tensor(sizes, est.device)
        if d.numel() != K:
            raise ValueError(f"{d.numel()} sizes for {K} columns")
        t, ts = (None, 0) if temperature is None else _temperature(temperature, S, est.device)
        out = torch.empty((4, S, K), dtype=torch.float64, device=est.device)
        _hip.check(_hip.lib().sgmcmc_temper_tails(est.data_ptr(), _is_f64(est), S, K, est.stride(0), est.stride(1),
                                                  None if t is None else t.data_ptr(), ts, d.data_ptr(), out.data_ptr(),
                                                  _stream()), "sgmcmc_temper_tails")
    return out


def chi2_tails(ratio, sizes, log=True, temperature=None):
    """ratio: ``[S, K]`` (or ``[K]``) fp32 / fp64 device tensor or view of T^ / T, column k a tensor with ``sizes[k]``
    elements -> ``(lower, upper)``, each of ratio's shape in fp64: log P(chi^2_d / d <= r) and log P(chi^2_d / d > r), or the
    plain probabilities (``log=False``).  The smaller tail is evaluated in log space, so the logarithm stays finite where
    the probability underflows.  ``temperature`` ([S] or a number) divides ratio first.  ``lower`` with ``log=False`` is
    the probability integral transform u = P(d / 2, d r / 2): uniform on [0, 1] at the target temperature, and accepted by
    ``goodness_of_fit.goodness_of_fit(u, fits={"uniform": (0., 1.)})`` as it stands (that module fits no uniform law, so
    the family is named with its parameters)."""
    flat = isinstance(ratio, torch.Tensor) and ratio.dim() == 1
    out = _tails(ratio.unsqueeze(0) if flat else ratio, temperature, sizes)
    lower, upper = (out[2], out[3]) if log else (out[0], out[1])
    return (lower[0], upper[0]) if flat else (lower, upper)


def _steps(est, temperature, sizes, bounds, want_mean):
    est = _table(est, "est", 2)
    S, K = est.shape
    lib = _hip.lib()
    with torch.cuda.device(est.device):
        d = _sizes_tensor(sizes, est.device)
        if d.numel() != K:
            raise ValueError(f"{d.numel()} sizes for {K} columns of est")
        share = totals = mean = se = t = None
        C, ts = 0, 0
        if bounds is not None:
            if bounds.shape[0] != K or bounds.dim() != 3 or bounds.shape[2] != 2 or bounds.dtype != torch.float64:
                raise ValueError(f"bounds must be [K = {K}, C, 2] float64, not {tuple(bounds.shape)} {bounds.dtype}")
            bounds = bounds.to(est.device).contiguous()
            C = bounds.shape[1]
            if not 1 <= C <= MAX_LEVELS:
                raise ValueError(f"{C} levels: 1 .. {MAX_LEVELS} are supported")
            t, ts = _temperature(temperature, S, est.device)
            share = torch.empty((C, S), dtype=torch.float64, device=est.device)
            totals = torch.empty(K * C + 1, dtype=torch.int64, device=est.device)
        if want_mean:
            mean = torch.empty(S, dtype=torch.float64, device=est.device)
            se = torch.empty(S, dtype=torch.float64, device=est.device)
        ptr = lambda v: None if v is None else v.data_ptr()
        _hip.check(lib.sgmcmc_temper_steps(est.data_ptr(), _is_f64(est), S, K, est.stride(0), est.stride(1), ptr(t), ts,
                                           d.data_ptr(), ptr(bounds), C, ptr(share), ptr(mean), ptr(se), ptr(totals),
                                           _stream()), "sgmcmc_temper_steps")
    return share, totals, mean, se


def ewma(x, alpha):
    """Exponentially weighted moving average along the LAST dimension of an fp32 / fp64 device tensor or view -> fp64 of
    x's shape: y_0 = x_0, y_t = (1 - alpha) x_t + alpha y_(t-1) -- what plot.py's ``lfiltic`` / ``lfilter`` pair computes --
    as a scan of affine maps, every row at once.  ``alpha = 0`` returns the input's values bit for bit; a NaN poisons
    what follows it in its own row only.  No synchronisation."""
    alpha = float(alpha)
    if not 0.0 <= alpha < 1.0:
        raise ValueError(f"alpha = {alpha}: 0 <= alpha < 1")
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise ValueError("x must be a tensor with at least one dimension")
    rows = _table(x.unsqueeze(0) if x.dim() == 1 else x.reshape(-1, x.shape[-1]) if x.dim() > 2 else x, "x", 2)
    R, S = rows.shape
    with torch.cuda.device(rows.device):
        y = torch.empty((R, S), dtype=torch.float64, device=rows.device)
        _hip.check(_hip.lib().sgmcmc_temper_ewma(rows.data_ptr(), _is_f64(rows), R, S, rows.stride(0), rows.stride(1),
                                                 alpha, y.data_ptr(), _stream()), "sgmcmc_temper_ewma")
    return y.reshape(x.shape)


def kinetic_coverage(est, temperature, sizes, confidences=CONFIDENCES, ewma_alpha=0., bounds=None):
    """est: ``[S, K]`` fp32 / fp64 device tensor or view, row s the K tensors' kinetic temperature estimates at metrics
    step s; temperature: ``[S]`` or a number, the target; sizes: the K tensors' element counts ->

        share      [C, S] fp64: the share of the K tensors with lower <= est / temperature <= upper (both ends included, as
                   in plot.py's ``kinetic_temperature_intervals``; NaN and the inf of a zero temperature are outside)
        smoothed   [C, S]: ``ewma(share, ewma_alpha)``
        per_tensor [K, C] int64: the number of steps at which tensor k was inside level c (exact counts)
        finite     0-dim int64: the number of finite est / temperature

    ``bounds`` [K, C, 2] defaults to ``chi2_interval(sizes, confidences)``.  At the target temperature row c of share
    fluctuates about ``confidences[c]``.  No synchronisation."""
    est = _table(est, "est", 2)
    if bounds is None:
        bounds = chi2_interval(sizes, confidences, device=est.device)
    elif not isinstance(bounds, torch.Tensor) or not bounds.is_cuda:
        raise ValueError("bounds must be a CUDA tensor")
    alpha = float(ewma_alpha)
    if not 0.0 <= alpha < 1.0:
        raise ValueError(f"ewma_alpha = {alpha}: 0 <= alpha < 1")
    share, totals, _, _ = _steps(est, temperature, sizes, bounds, False)
    K, C = bounds.shape[0], bounds.shape[1]
    return share, ewma(share, alpha), totals[:K * C].reshape(K, C), totals[K * C]


def weighted_temperature(est, sizes):
    """``(mean [S], se [S])`` fp64 of est ``[S, K]``: the mean of the K tensors' temperatures weighted by their sizes and
    the variance of that weighted mean after Cochran (1977) -- plot.py's ``weighted_var_se``, the band that
    ``temperature_stderr`` draws.  K = 1 has no such variance (NaN).  No synchronisation."""
    _, _, mean, se = _steps(est, None, sizes, None, True)
    return mean, se


def _columns(metrics):
    "a MemoryMetrics, the path of an HDF5Metrics file, or a dict of columns -> {name: fp64 numpy column}"
    if isinstance(metrics, dict):
        return {k: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in metrics.items()}
    if isinstance(metrics, (str, bytes)) or hasattr(metrics, "__fspath__"):
        # HDF5Metrics keeps "est_temperature/<name>" as a dataset inside the group "est_temperature": every dataset is read,
        # nested groups included, under its slash-joined path (a file still being written is fine: SWMR read)
        from . import _h5
        with _h5.File(metrics, "r", swmr=True) as f:
            return {k: np.asarray(f[k][slice(None)]) for k in f.dataset_names()}
    if hasattr(metrics, "column") and hasattr(metrics, "names"):
        names = metrics.names()
        cols = {k: metrics.column(k)[1] for k in names}
        cols["steps"] = metrics.column(names[0])[0] if names else np.zeros(0, dtype=np.int64)
        return cols
    raise ValueError("metrics must be a MemoryMetrics, the path of an HDF5Metrics file, or a dict of columns")


def temperature_report(metrics, sizes_or_model, mask=slice(None), confidences=CONFIDENCES, ewma_alpha=0., pit=False,
                       device=None):
    """The temperature diagnostics of one run.  metrics: a ``storage.MemoryMetrics``, the path of an ``HDF5Metrics`` file,
    or a dict of equally long columns; sizes_or_model: ``{name: numel}`` or the model (``get_sizes``); mask: a slice or
    index array over the metrics rows (plot.py's ``mask``).  Every ``est_temperature/<name>`` column is paired with
    ``sizes[name]`` (the ``/all`` rows are left out, a column without a size raises).  Returns a dict:

        steps [S] int64 (host), names (the K tensors, alphabetical: the columns' order below), sizes [K], temperature [S], confidences,
        intervals [K, C, 2], coverage [C, S], coverage_smoothed [C, S], coverage_per_tensor [K, C], finite,
        kinetic_mean [S], kinetic_se [S]        -- ``kinetic_coverage`` and ``weighted_temperature`` of the kinetic group
        config_mean [S], config_se [S]          -- ``weighted_temperature`` of ``est_config_temp/<name>``, which has no
                                                   chi^2 law and hence no intervals; absent if the run logged none
        pit, log_lower, log_upper [S, K]        -- with ``pit=True``: ``chi2_tails`` of est / temperature

    all device tensors in fp64 but ``steps``.  ``pit`` is what ``goodness_of_fit.goodness_of_fit(pit, fits={"uniform":
    (0., 1.)})`` scores against the uniform law."""
    device = _device(device)
    sizes = get_sizes(sizes_or_model) if isinstance(sizes_or_model, torch.nn.Module) else dict(sizes_or_model)
    cols = _columns(metrics)
    if "temperature" not in cols or "steps" not in cols:
        raise ValueError("metrics has no 'temperature' / 'steps' column")

    def group(prefix):
        # alphabetical, the order in which an HDF5 file lists them: the same report whatever the source
        names = sorted(k[len(prefix) + 1:] for k in cols if k.startswith(prefix + "/") and k != prefix + "/all")
        missing = [n for n in names if n not in sizes]
        if missing:
            raise ValueError(f"no size for {missing}: sizes must name every tensor of {prefix}/")
        if not names:
            return names, None
        table = np.stack([np.asarray(cols[f"{prefix}/{n}"], dtype=np.float64)[mask] for n in names], axis=1)
        return names, torch.from_numpy(np.ascontiguousarray(table)).to(device)

    names, kinetic = group(_KINETIC)
    if kinetic is None:
        raise ValueError(f"metrics has no '{_KINETIC}/<name>' column")
    if kinetic.shape[0] < 1:
        raise ValueError("mask selects no row")
    d = [sizes[n] for n in names]
    temperature = torch.from_numpy(np.ascontiguousarray(np.asarray(cols["temperature"], dtype=np.float64)[mask])).to(device)
    conf = _confidences(confidences)
    intervals = chi2_interval(d, conf, device=device)
    share, smoothed, per_tensor, finite = kinetic_coverage(kinetic, temperature, d, conf, ewma_alpha, bounds=intervals)
    mean, se = weighted_temperature(kinetic, d)
    out = dict(steps=torch.from_numpy(np.asarray(cols["steps"])[mask].astype(np.int64)), names=tuple(names),
               sizes=torch.tensor(_sizes(d), dtype=torch.int64, device=device), temperature=temperature,
               confidences=tuple(conf), intervals=intervals, coverage=share, coverage_smoothed=smoothed,
               coverage_per_tensor=per_tensor, finite=finite, kinetic_mean=mean, kinetic_se=se)
    cnames, config = group(_CONFIG)
    if config is not None:
        out["config_mean"], out["config_se"] = weighted_temperature(config, [sizes[n] for n in cnames])
    if pit:
        tails = _tails(kinetic, temperature, d)
        out["pit"], out["log_lower"], out["log_upper"] = tails[0], tails[2], tails[3]
    return out
