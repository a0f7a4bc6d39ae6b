"""Writes tests/golden/raob.npz: what the REFERENCE's Rao-Blackwellised models compute (bnn_priors/models/base.py:194-311),
on the CPU, in float64 and in float32, for tests/test_raob.py.

    python tests/golden/make_raob_goldens.py

The reference calls ``torch.cholesky``, which current torch no longer has; ``torch.linalg.cholesky`` is the same
factorisation (lower triangle), so it is put in its place before the reference is imported.  Nothing else is changed.

Two cases, the same numbers in both dtypes (drawn in float64, rounded for float32):
    dense   RaoBDenseNet(x, y, 40, noise_std=0.8), N = 10, 3 inputs: the reference's own test (testing/test_models.py)
    linear  RaoBLinearRegression(x, y, noise_std=0.5), N = 10, 3 inputs
Per case and dtype: the state_dict, x_test, log_likelihood and its gradient per parameter, posterior_w() and the mean and
scale of model(x_test).  Also the state_dict keys of get_model("raobdensenet") and get_model("raob_linear").
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

ref_stubs.install()
torch.cholesky = torch.linalg.cholesky

from bnn_priors import exp_utils  # noqa: E402
from bnn_priors.models import RaoBDenseNet, RaoBLinearRegression  # noqa: E402


def build(case, x, y):
    if case == "dense":
        return RaoBDenseNet(x, y, 40, noise_std=0.8)
    return RaoBLinearRegression(x, y, noise_std=0.5)


def main():
    out = {}
    torch.manual_seed(1)
    torch.set_default_dtype(torch.float64)
    x = torch.randn(10, 3) * 2
    y = torch.randn(10, 1) * 2
    x_test = torch.randn(7, 3) * 2
    for case in ("dense", "linear"):
        torch.manual_seed(2)
        torch.set_default_dtype(torch.float64)
        weights = {k: v.clone() for k, v in build(case, x, y).state_dict().items()}
        for dtype in (torch.float64, torch.float32):
            tag = f"{case}.{str(dtype).split('.')[1]}"
            torch.set_default_dtype(dtype)
            model = build(case, x.to(dtype), y.to(dtype))
            model.load_state_dict({k: v.to(dtype) for k, v in weights.items()})
            ll = model.log_likelihood(None, None, 10)
            params = dict(model.named_parameters())
            grads = torch.autograd.grad(ll, list(params.values())) if params else ()
            with torch.no_grad():
                mean, root = model.posterior_w()
                pred = model(x_test.to(dtype))
            for k, v in model.state_dict().items():
                out[f"{tag}.state.{k}"] = v.numpy()
            out[f"{tag}.x_test"] = x_test.to(dtype).numpy()
            out[f"{tag}.ll"] = ll.detach().numpy()
            for k, g in zip(params, grads):
                out[f"{tag}.grad.{k}"] = g.numpy()
            out[f"{tag}.w_mean"] = mean.numpy()
            out[f"{tag}.w_root"] = root.numpy()
            out[f"{tag}.pred_mean"] = pred.mean.numpy()
            out[f"{tag}.pred_scale"] = pred.scale.numpy()
    torch.set_default_dtype(torch.float32)
    for name in ("raobdensenet", "raob_linear"):
        m = exp_utils.get_model(x.float(), y.float(), name, 50, 3, "gaussian", 0., 2 ** .5, "gaussian", 0., 1., True, {}, {})
        out[f"keys.{name}"] = np.array(sorted(m.state_dict().keys()))
    np.savez_compressed(os.path.join(HERE, "raob.npz"), **out)
    print("wrote raob.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
