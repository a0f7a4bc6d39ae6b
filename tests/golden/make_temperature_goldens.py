"""Writes tests/golden/temperature.npz: what the REFERENCE's temperature diagnostics compute (bnn_priors/plot.py:14-141), on
the CPU with scipy, for tests/test_temperature.py.

    python tests/golden/make_temperature_goldens.py

plot.py imports ``gpytorch.lazy.DiagLazyTensor`` at module scope (for ``gp_posterior``, which is not called here): a stub
is put in its place before the import.  Nothing of the reference is changed.  Recorded:

    _gamma_confidence            on the synthetic table's sizes at the default confidences, and on the quantile test's
                                 grid of sizes at (.05, .25, .5, .75, .95, .999)
    kinetic_temperature_intervals   what it hands to ``ax.plot`` (a recording stand-in for the axes), at ewma_alpha 0 and 0.7
    weighted_var_se, ewma        on the same table

The table is synthetic and seeded: S = 37 metrics rows, K = 5 tensors of sizes (1, 2, 10, 640, 36864), est = temperature *
chi^2_d / d draws, a target temperature that changes half way, one row of NaN estimates and one row with temperature 0.
Every est / temperature keeps a relative distance of 1e-9 from every interval end (checked here with scipy's ends, and
again in the test with the 50-digit ones), so that no rounding decides a count.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

ref_stubs.install()
lazy = types.ModuleType("gpytorch.lazy")
lazy.DiagLazyTensor = object
sys.modules.setdefault("gpytorch.lazy", lazy)

from bnn_priors import plot  # noqa: E402

NAMES = ("scale", "bias.b", "head.bias", "head.weight", "conv.weight")
SIZES = (1, 2, 10, 640, 36864)
CONFIDENCES = (.05, .25, .5, .75, .95)
GRID_SIZES = (1, 2, 3, 7, 100, 19999, 20000, 20002, 36864, 78400, 10 ** 6, 10 ** 7, 2 ** 31 - 1)
GRID_CONFIDENCES = (.05, .25, .5, .75, .95, .999)
S, NAN_ROW, ZERO_ROW = 37, 11, 23


class Line:
    def get_color(self):
        return "k"


class Axes:
    "keeps what is passed to ax.plot"
    def __init__(self):
        self.plotted = []

    def axhline(self, *a, **kw):
        return Line()

    def plot(self, x, y, **kw):
        self.plotted.append((np.asarray(x).copy(), np.asarray(y).copy()))
        return [Line()]

    def legend(self):
        pass


def main():
    rng = np.random.default_rng(20240611)
    sizes = dict(zip(NAMES, SIZES))
    temperature = np.where(np.arange(S) < 18, 1.0, 0.25)
    est = np.stack([temperature * rng.chisquare(d, size=S) / d for d in SIZES], axis=1)
    est[5, 0] *= 40.0                    # far outside every interval
    est[NAN_ROW] = np.nan
    temperature[ZERO_ROW] = 0.0
    config = np.stack([temperature * (1.0 + 0.1 * rng.standard_normal(S)) for _ in SIZES], axis=1)
    steps = np.arange(S, dtype=np.int64) * 10

    intervals = plot._gamma_confidence(sizes, np.array(CONFIDENCES))
    lower = np.stack([intervals[k][0] for k in NAMES])
    upper = np.stack([intervals[k][1] for k in NAMES])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = est / temperature[:, None]
    for k in range(len(SIZES)):
        for end in (lower[k], upper[k]):
            gap = np.abs(ratio[:, k, None] - end[None, :]) / end[None, :]
            assert not (gap < 1e-9).any(), "an estimate sits on an interval end: change the seed"

    metrics = {"steps": steps, "temperature": temperature,
               "est_temperature": dict({k: est[:, i] for i, k in enumerate(NAMES)},
                                       all=est @ np.array(SIZES, dtype=float) / sum(SIZES))}
    out = dict(names=np.array(NAMES), sizes=np.array(SIZES, dtype=np.int64), confidences=np.array(CONFIDENCES),
               steps=steps, temperature=temperature, est=est, config=config, lower=lower, upper=upper)
    cmap = lambda c: [(0., 0., 0., 1.)] * len(c)
    for tag, alpha in (("a0", 0.0), ("a07", 0.7)):
        ax = Axes()
        plot.kinetic_temperature_intervals(ax, metrics, sizes, ewma_alpha=alpha, confidences=list(CONFIDENCES),
                                           cmap=cmap, legend=False)
        assert len(ax.plotted) == len(CONFIDENCES) and all((x == steps).all() for x, _ in ax.plotted)
        out["coverage_" + tag] = np.stack([y for _, y in ax.plotted])
    ax = Axes()
    plot.kinetic_temperature_intervals(ax, metrics, sizes, mask=slice(3, 30, 2), ewma_alpha=0.0,
                                       confidences=list(CONFIDENCES), cmap=cmap, legend=False)
    out["coverage_masked"] = np.stack([y for _, y in ax.plotted])

    w = np.array(SIZES, dtype=float)
    for tag, table in (("kinetic", est), ("config", config)):
        mean, se = plot.weighted_var_se(w, table)
        out[tag + "_mean"], out[tag + "_se"] = mean, se
    finite = np.delete(est, NAN_ROW, axis=0).T.copy()            # [K, S - 1]: rows to smooth
    for tag, alpha in (("a0", 0.0), ("a05", 0.5), ("a0999", 0.999)):
        out["ewma_" + tag] = np.stack([plot.ewma(row, alpha) for row in finite])
    out["ewma_input"] = finite

    grid = plot._gamma_confidence({str(d): d for d in GRID_SIZES}, np.array(GRID_CONFIDENCES))
    out["grid_sizes"] = np.array(GRID_SIZES, dtype=np.int64)
    out["grid_confidences"] = np.array(GRID_CONFIDENCES)
    out["grid_lower"] = np.stack([grid[str(d)][0] for d in GRID_SIZES])
    out["grid_upper"] = np.stack([grid[str(d)][1] for d in GRID_SIZES])
    path = os.path.join(HERE, "temperature.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
