"""Model construction by name for the BASELINE configs.

Restates the on-path part of ``bnn_priors/exp_utils.py:63-69,99-105,108-234``:
``get_model`` for classificationdensenet / classificationconvnet / googleresnet /
densenet, the correlated nets correlatedclassificationconvnet / correlatedgoogleresnet, decreasing_mvt_googleresnet and
the data-driven MNIST convnets datadrivengaussconv / datadrivendoublegammaconv, the Rao-Blackwellised regression models
raobdensenet / raob_linear, ``he_initialize``, and the ``net.module.`` wrapper that gives stored
samples the reference's key prefix.  (The reference wraps GPU models in
``nn.DataParallel``; here one chain owns one GPU, so the wrapper is always the
plain ``DummyModule`` -- the keys are identical.)
"""
import math

import torch
from torch import nn

from ..prior import LogNormal, get_prior
from .data_driven import DataDrivenDoubleGammaClassificationConvNet, DataDrivenGaussianClassificationConvNet
from .nets import (ClassificationConvNet, ClassificationDenseNet, CorrelatedClassificationConvNet, CorrelatedResNet,
                   DecreasingMVTGoogleResNet, DenseNet, RaoBDenseNet, RaoBLinearRegression, ResNet)

__all__ = ("get_model", "he_initialize", "DummyModule")


class DummyModule(nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *a, **kw):
        return self.module(*a, **kw)


def he_initialize(model):
    "Kaiming-normal weights, U(-1/sqrt(n_out), 1/sqrt(n_out)) biases (exp_utils.py:63-69)"
    for name, param in model.named_parameters():
        if "weight_prior.p" in name:
            nn.init.kaiming_normal_(param.data, mode='fan_in', nonlinearity='relu')
        elif "bias_prior.p" in name:
            bound = 1 / math.sqrt(param.size(0))
            nn.init.uniform_(param.data, -bound, bound)


def get_model(x_train, y_train, model, width=50, depth=3, weight_prior="gaussian", weight_loc=0.,
              weight_scale=2 ** .5, bias_prior="gaussian", bias_loc=0., bias_scale=1.,
              batchnorm=True, weight_prior_params={}, bias_prior_params={}, *, prior_data=None):
    """``prior_data``: the fitted tables of datadrivengaussconv / datadrivendoublegammaconv (models/data_driven.py: a
    directory holding the reference's two data files, a mapping of their contents, or None for the installed reference
    package's copies); unused by the other models"""
    scaling_fn = (lambda std, dim: std / dim) if weight_prior == "cauchy" \
        else (lambda std, dim: std / dim ** 0.5)
    common = dict(prior_w=get_prior(weight_prior), loc_w=weight_loc, std_w=weight_scale,
                  prior_b=get_prior(bias_prior), loc_b=bias_loc, std_b=bias_scale,
                  scaling_fn=scaling_fn, weight_prior_params=weight_prior_params,
                  bias_prior_params=bias_prior_params)
    if model == "classificationdensenet":
        net = ClassificationDenseNet(x_train.size(-1), int(y_train.max()) + 1, width, depth,
                                     softmax_temp=1., **common)
    elif model in ("classificationconvnet", "correlatedclassificationconvnet", "datadrivengaussconv",
                   "datadrivendoublegammaconv"):
        if x_train.dim() == 4:
            in_channels, img_height = x_train.shape[1], x_train.shape[-2]
        else:
            in_channels, img_height = 1, int(math.sqrt(x_train.shape[-1]))
        extra = {}
        if model == "classificationconvnet":
            cls = ClassificationConvNet
        elif model == "correlatedclassificationconvnet":
            cls = CorrelatedClassificationConvNet
        else:
            # the fitted priors replace weight_prior / weight_scale / scaling_fn (exp_utils.py:130-152)
            cls = (DataDrivenGaussianClassificationConvNet if model == "datadrivengaussconv"
                   else DataDrivenDoubleGammaClassificationConvNet)
            extra["prior_data"] = prior_data
        net = cls(in_channels, img_height, int(y_train.max()) + 1, width, depth, softmax_temp=1., **common, **extra)
    elif model == "googleresnet":
        # NB: conv_prior_w is not forwarded, so convolutions stay Gaussian whatever
        # weight_prior says (reference quirk, exp_utils.py:186-190).
        net = ResNet(depth=20, bn=batchnorm, softmax_temp=1., **common)
    elif model == "correlatedgoogleresnet":
        # weight_prior is the CONVOLUTIONS' prior, the head is Normal (exp_utils.py:201-207); weight_prior_params go to
        # the convolutions only (the reference also hands them to the head's Normal, which raises TypeError there)
        net = CorrelatedResNet(depth=20, bn=batchnorm, softmax_temp=1., **common)
    elif model == "decreasing_mvt_googleresnet":
        # weight_prior goes to the convolutions and the head; the first blocks become MultivariateT (exp_utils.py:194-200)
        net = DecreasingMVTGoogleResNet(depth=20, bn=batchnorm, softmax_temp=1., **common)
    elif model == "densenet":
        net = DenseNet(x_train.size(-1), y_train.size(-1), width, depth, noise_std=1., **common)
    elif model == "raobdensenet":
        # default priors and a learned noise level, whatever the prior arguments say (exp_utils.py:123-124)
        net = RaoBDenseNet(x_train, y_train, width, noise_std=LogNormal((), -1., 0.2)).to(x_train)
    elif model == "raob_linear":
        net = RaoBLinearRegression(x_train, y_train, noise_std=0.5)           # (exp_utils.py:219-220)
    else:
        raise ValueError(f"model='{model}' is outside the accelerated path")
    net = net.to(x_train.device if isinstance(x_train, torch.Tensor) else "cpu")
    inner = net.net
    del net.net
    net.net = DummyModule(inner)
    return net
