"""The paper's data-driven MNIST convnets (reference: models/data_driven_conv_nets.py:15-109, exp_utils.py:130-152).

The BASELINE convnet at depth 3 (same layers, widths and kernels, the same ``net.module.1/4/8`` indices and RNG
consumption order) whose priors are fitted to SGD-trained weights:

* ``DataDrivenGaussianClassificationConvNet``: ``FixedCovNormal`` on both convolutions, Normal head -- every prior is in
  the HIP hook, so the step is captured;
* ``DataDrivenDoubleGammaClassificationConvNet``: ``FixedCovLaplace`` / ``FixedCovDoubleGamma`` on the convolutions (in
  the hook), the element-wise ``DoubleGamma`` head (autograd, ``Potential.leftover``: the step runs eagerly).

Biases are ``Normal(0, sqrt(var))`` (the fitted mean is ignored, as ``Conv2dPrior`` ignores ``loc_b``).  No scaling by
fan-in.  ``prior_w`` / ``loc_w`` / ``std_w`` / ``scaling_fn`` and the bias arguments are accepted and ignored, as in the
reference.

The fitted tables are the reference's data files ``mean_covs_mnist_classification.pkl.gz`` and
``fits_mnist_classification.pkl.gz`` (gzip'd pickles of dicts of numpy values).  ``prior_data`` is a directory that holds
them, or a mapping from those two file names to what the files hold; None looks next to an installed reference package.
"""
import gzip
import importlib.util
import os
import pickle
from collections.abc import Mapping

import torch
from torch import nn

from .. import prior
from .base import ClassificationModel
from .nets import Conv2dPrior, LinearPrior, Reshape, _ConvPoolTrunk

__all__ = ("DataDrivenGaussianClassificationConvNet", "DataDrivenDoubleGammaClassificationConvNet",
           "load_prior_data", "MEAN_COVS_FILE", "FITS_FILE")

MEAN_COVS_FILE = "mean_covs_mnist_classification.pkl.gz"
FITS_FILE = "fits_mnist_classification.pkl.gz"


def _reference_models_dir():
    "the ``models`` directory of an installed reference package (found without importing it), or None"
    try:
        spec = importlib.util.find_spec("bnn_priors")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.submodule_search_locations:
        return None
    return os.path.join(list(spec.submodule_search_locations)[0], "models")


def load_prior_data(prior_data=None, fits=True):
    """(mean_covs, fits) of the data-driven convnets; ``fits`` (the per-module fit dict, the second element of the
    reference's pickled pair) is None unless asked for.  ``prior_data``: a directory holding both files, a mapping
    {MEAN_COVS_FILE: ..., FITS_FILE: ...} of their contents, or None (the reference package's own copies)."""
    if isinstance(prior_data, Mapping):
        mean_covs = prior_data[MEAN_COVS_FILE]
        table = prior_data[FITS_FILE] if fits else None
    else:
        where = prior_data if prior_data is not None else _reference_models_dir()
        paths = [os.path.join(where, f) for f in (MEAN_COVS_FILE, FITS_FILE)] if where is not None else []
        if not paths or not all(os.path.isfile(p) for p in paths[:2 if fits else 1]):
            raise FileNotFoundError(
                f"the data-driven convnets need {MEAN_COVS_FILE} and {FITS_FILE}: "
                + (f"not found in {where}" if where is not None else "pass prior_data= (no reference package installed)"))
        with gzip.open(paths[0], "rb") as f:
            mean_covs = pickle.load(f)
        table = None
        if fits:
            with gzip.open(paths[1], "rb") as f:
                table = pickle.load(f)
    if table is not None and not isinstance(table, Mapping):
        _, table = table                       # the file holds a pair; the reference reads its second element
    return mean_covs, table


def _normal_bias(mean_covs, idx):
    return dict(prior_b=prior.Normal, loc_b=mean_covs[f"net.module.{idx}.bias_prior.p"][0],
                std_b=mean_covs[f"net.module.{idx}.bias_prior.p"][1] ** .5)


def _fixed_cov(mean_covs, idx):
    loc, cov = mean_covs[f"net.module.{idx}.weight_prior.p"]
    return dict(loc_w=torch.from_numpy(loc), std_w=torch.from_numpy(cov))


def _no_scaling(std, dim):
    return std


def _net(in_channels, img_height, out_features, width, depth, softmax_temp, conv_1, conv_2, head):
    assert depth == 3, "That's what we have data"
    reshaped_size = width * (img_height // 2 ** (depth - 1)) ** 2        # 2**(depth-1): the max-pools
    layers = [Reshape(-1, in_channels, img_height, img_height),
              Conv2dPrior(in_channels, width, kernel_size=3, padding=1, scaling_fn=_no_scaling, **conv_1),
              nn.ReLU(), nn.MaxPool2d(2),
              Conv2dPrior(width, width, kernel_size=3, padding=1, scaling_fn=_no_scaling, **conv_2),
              nn.ReLU(), nn.MaxPool2d(2),
              nn.Flatten(),
              LinearPrior(reshaped_size, out_features, scaling_fn=_no_scaling, **head)]
    return ClassificationModel(_ConvPoolTrunk(*layers), softmax_temp)


def DataDrivenGaussianClassificationConvNet(in_channels, img_height, out_features, width, depth=3, softmax_temp=1.,
                                            prior_w=prior.Normal, loc_w=0., std_w=2 ** .5, prior_b=prior.Normal,
                                            loc_b=0., std_b=1., scaling_fn=None, weight_prior_params={},
                                            bias_prior_params={}, *, prior_data=None):
    "``FixedCovNormal`` convolutions, Normal head (reference: models/data_driven_conv_nets.py:15-58)"
    assert depth == 3, "That's what we have data"
    mc, _ = load_prior_data(prior_data, fits=False)
    head_w = mc["net.module.8.weight_prior.p"]
    return _net(in_channels, img_height, out_features, width, depth, softmax_temp,
                dict(prior_w=prior.FixedCovNormal, **_fixed_cov(mc, 1), **_normal_bias(mc, 1)),
                dict(prior_w=prior.FixedCovNormal, **_fixed_cov(mc, 4), **_normal_bias(mc, 4)),
                dict(prior_w=prior.Normal, loc_w=head_w[0], std_w=head_w[1] ** .5, **_normal_bias(mc, 8)))


def DataDrivenDoubleGammaClassificationConvNet(in_channels, img_height, out_features, width, depth=3, softmax_temp=1.,
                                               prior_w=prior.Normal, loc_w=0., std_w=2 ** .5, prior_b=prior.Normal,
                                               loc_b=0., std_b=1., scaling_fn=None, weight_prior_params={},
                                               bias_prior_params={}, *, prior_data=None):
    """``FixedCovLaplace`` first convolution, ``FixedCovDoubleGamma`` second, element-wise ``DoubleGamma`` head
    (reference: models/data_driven_conv_nets.py:61-109)"""
    assert depth == 3, "That's what we have data"
    mc, fits = load_prior_data(prior_data)
    dg_4, dg_8 = fits["net.module.4.weight_prior.p"]["dgamma"], fits["net.module.8.weight_prior.p"]["dgamma"]
    return _net(in_channels, img_height, out_features, width, depth, softmax_temp,
                dict(prior_w=prior.FixedCovLaplace, **_fixed_cov(mc, 1), **_normal_bias(mc, 1)),
                dict(prior_w=prior.FixedCovDoubleGamma, **_fixed_cov(mc, 4), **_normal_bias(mc, 4),
                     weight_prior_params=dict(concentration=dg_4[0])),
                dict(prior_w=prior.DoubleGamma, loc_w=dg_8[1], std_w=dg_8[2], **_normal_bias(mc, 8),
                     weight_prior_params=dict(concentration=dg_8[0])))
