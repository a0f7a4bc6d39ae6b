"""Posterior-predictive evaluation (SURVEY.md section 8 row f1 / e).

``evaluate_model`` restates ``bnn_priors/exp_utils.py:250-340`` for the
likelihood / accuracy outputs: for every stored sample load it, run the test
set, keep log p(y|x) ``lps[E,N]`` and the normalised logits ``acc[E,N,C]`` in
float64 ON THE DEVICE, then

    lp_ensemble  = mean_n( logsumexp_e lps - log E )
    ensemble logits = logsumexp_e acc - log E ,  acc = argmax == y

``ensemble_across_chains`` is the one exchange step of the multi-chain path:
each rank reduces its own samples to (max_e, sum_e exp(x - max)) and two small
all-reduces (MAX, SUM) over RCCL combine the chains -- N_test*(C+1) doubles,
instead of gathering [E, N, C] from every GPU.
"""
import contextlib
import math
import os
import warnings
import weakref

import torch

from . import _capture

__all__ = ("evaluate_model", "evaluate_ood", "predictive_tables", "logit_tables", "ensemble_across_chains",
           "ensemble_metrics", "gather_samples", "evaluate_loo", "evaluate_marglik", "evaluate_uncertainty",
           "regression_tables", "evaluate_regression", "evaluate_stein", "evaluate_eff_dim",
           "evaluate_prior_sensitivity")


def _labels_of(dataloader):
    ds = dataloader.dataset
    if hasattr(ds, "tensors"):
        return ds.tensors[1]
    if hasattr(ds, "targets"):
        return torch.as_tensor(ds.targets)
    raise ValueError("I cannot find the labels in the dataloader.")


def _n_samples(samples):
    return min(len(v) for v in samples.values())


class _NotBatchable(Exception):
    "the grouped (vmap) evaluation cannot run this model / these samples: evaluate sample by sample instead"


# Stack the samples and run ONE grouped (vmap) forward per test batch on the library's batched layers.  OFF by default
# since round 4: once the test set is sliced instead of iterated (``_resident_tensors``) the sample-by-sample pass on
# this package's kernels -- a captured forward per 1,024 rows, ``load_state_dict`` per sample -- is 3-4x faster for all
# three BASELINE nets (10 samples x 10,000 rows, tools/eval_probe.py: googleresnet 141 vs 427 ms, convnet 24 vs 71,
# densenet 15 vs 58), needs no MIOpen kernel search (1.4-5 s on first use) and gives the per-epoch evaluation's bits.
BATCHED = False          # (module attribute, not an environment switch: tests set it)
SAMPLE_GROUP = 32       # samples per grouped forward: bounds the activation memory at E_group * batch images


@contextlib.contextmanager
def _plain_torch_layers():
    """torch.func.vmap batches ATen operators, not this package's custom-kernel autograd functions: inside the
    grouped forward the layers take their ATen route (the grouped evaluation is a throughput problem -- E samples x
    a test batch per launch -- that the library's batched convolutions / GEMMs handle well).
    The switch is process-wide but never observable by another chain: the block runs to completion inside ONE
    ``next()`` of a runner's generator (multichain.run_on_streams interleaves chains only at ``yield`` points, and
    nothing in here yields), on one Python thread."""
    from . import bn, conv, pool, resblock
    mods = (bn, conv, pool, resblock)
    old = [m.ENABLED for m in mods]
    for m in mods:
        m.ENABLED = False
    try:
        yield
    finally:
        for m, v in zip(mods, old):
            m.ENABLED = v


@torch.no_grad()
def _predictive_tables_batched(model, dataloader_test, samples, labels, E, C):
    """All samples at once (reference semantics: exp_utils.py:250-340, one load_state_dict + one pass over the test
    set PER SAMPLE): the stored samples stay stacked [E, ...], ``torch.func.functional_call`` under ``vmap`` runs the
    network once per test batch for a whole group of samples, and the normalisation (log-softmax), the gather of
    log p(y|x) and the fp64 tables are filled on the device without a Python loop over samples."""
    from torch.func import functional_call, vmap
    device = labels.device
    N = labels.shape[0]
    lps = torch.zeros((E, N), dtype=torch.float64, device=device)
    acc = torch.zeros((E, N, C), dtype=torch.float64, device=device)
    names = set(dict(model.named_parameters())) | set(dict(model.named_buffers()))
    state = {k: v[:E].to(device) for k, v in samples.items() if k in names}
    if set(state) != names:
        raise _NotBatchable("the samples do not cover the model's state")
    temp = model.softmax_temp
    if callable(temp) or isinstance(temp, torch.Tensor):
        raise _NotBatchable("the softmax temperature is not a plain number")

    def logits_of(st, x):
        return functional_call(model.net, {k[len("net."):]: v for k, v in st.items()}, (x,))
    grouped = vmap(logits_of, in_dims=(0, None), randomness="error")
    with _plain_torch_layers():
        i = 0
        for bx, by in dataloader_test:
            bx, by = bx.to(device), by.to(device)
            j = i + len(bx)
            for e0 in range(0, E, SAMPLE_GROUP):
                e1 = min(E, e0 + SAMPLE_GROUP)
                try:
                    f = grouped({k: v[e0:e1] for k, v in state.items()}, bx)           # [e, B, C]
                except RuntimeError as exc:
                    # only vmap's own refusals fall back (an operator without a batching rule, in-place writes to
                    # an unbatched tensor, data-dependent control flow); out-of-memory and real bugs propagate
                    msg = str(exc)
                    if any(t in msg for t in ("vmap", "batching rule", "Batching rule", "functorch")):
                        raise _NotBatchable(msg.splitlines()[0]) from exc
                    raise
                logp = torch.log_softmax(f / temp, dim=-1)        # Categorical(logits=...).logits, in the net's dtype
                acc[e0:e1, i:j] = logp
                lps[e0:e1, i:j] = logp.gather(-1, by.view(1, -1, 1).expand(e1 - e0, -1, 1)).squeeze(-1)
            i = j
    return lps, acc


# ---- sample-by-sample evaluation on a captured forward ---------------------------------------------------------
# The per-epoch evaluation (inference.py:199-213) and the stored samples' predictions (exp_utils.py:250-340) run the
# network once per test batch: ~80 kernels launched eagerly from Python, 1.7 ms per batch of which the GPU works 0.3.
# ``_GraphedLogits`` captures ``model.net(x)`` (eval mode: this package's convolution kernels, the running-statistics
# BatchNorm kernel, the fused head) on a static input batch once per (model, batch shape) and replays it per batch;
# ``load_state_dict`` writes into the parameters' own storage, so the graph sees every sample.
EVAL_GRAPH = True


# rows per evaluation forward (0: the loader's own batches)
EVAL_ROWS = 1024


def _resident_tensors(dataloader):
    """(x, y) when the loader is a plain in-order pass over a TensorDataset-like set (``.tensors``, SequentialSampler,
    default collation, no workers): its batches are consecutive slices of those tensors, so the evaluation can slice them
    itself instead of iterating the DataLoader -- which indexes the set item by item and stacks 128 views per batch,
    ~0.3 ms of host time each: 24 of the 28 ms a per-epoch evaluation of 10,000 rows took"""
    ds = getattr(dataloader, "dataset", None)
    t = getattr(ds, "tensors", None)
    if (t is None or len(t) != 2 or getattr(ds, "augment", None) is not None
            or not isinstance(getattr(dataloader, "sampler", None), torch.utils.data.SequentialSampler)
            or dataloader.batch_size is None or dataloader.num_workers != 0
            or dataloader.collate_fn is not torch.utils.data.default_collate):
        return None
    n = len(ds)
    if dataloader.drop_last:
        n -= n % dataloader.batch_size
    return t[0][:n], t[1][:n]


def _row_groups(dataloader, device, rows):
    "the loader's batches, consecutive ones concatenated up to ``rows`` rows (order kept; the last group is what is left)"
    if rows <= 0:
        yield from dataloader
        return
    res = _resident_tensors(dataloader)
    if res is not None:
        # the same groups: whole batches up to ``rows`` rows each, as slices of the set (moved once if it lives on the host)
        # DataLoader.__iter__ draws a worker base seed from the (global) generator before anything else
        # (torch/utils/data/dataloader.py, _BaseDataLoaderIter.__init__): a run that iterates the test loader -- the
        # reference's evaluate_model -- consumes it, and the plain runners seed their next shuffle from the same stream
        torch.empty((), dtype=torch.int64).random_(generator=dataloader.generator)
        bs = dataloader.batch_size
        per = max(bs, rows // bs * bs)
        x, y = _resident_on(dataloader, res, device)
        for i in range(0, x.shape[0], per):
            yield x[i:i + per], y[i:i + per]
        return
    xs, ys, have = [], [], 0
    for bx, by in dataloader:
        if xs and have + len(bx) > rows:
            yield (torch.cat(xs), torch.cat(ys)) if len(xs) > 1 else (xs[0], ys[0])
            xs, ys, have = [], [], 0
        xs.append(bx.to(device))
        ys.append(by.to(device))
        have += len(bx)
    if xs:
        yield (torch.cat(xs), torch.cat(ys)) if len(xs) > 1 else (xs[0], ys[0])


# loader -> (host x, host y, their versions, device, x on the device, y on the device): a host-resident test set is moved
# once per loader.  Weakly keyed by the loader OBJECT (an id() can be reused by the next loader of a loop that builds
# fresh ones) and holding the host tensors it was copied from, so neither their address nor the loader's can come
# back meaning other data; an in-place edit of the host tensors (normalisation after a first evaluation) bumps their
# version counters and invalidates the copy.  Tensors already on the device are never cached (nothing is copied).
_resident_cache = weakref.WeakKeyDictionary()


def _root(t):
    "the tensor a view was sliced from (views share its version counter), else the tensor itself"
    return t._base if t._base is not None else t


def _resident_on(dataloader, res, device):
    x, y = res
    device = torch.device(device)
    if x.device == device and y.device == device:
        return x, y
    c = _resident_cache.get(dataloader)
    if (c is not None and c[0] is _root(x) and c[1] is _root(y)
            and c[2] == (x._version, y._version, tuple(x.shape), tuple(y.shape)) and c[3] == device):
        return c[4], c[5]
    xd, yd = x.to(device), y.to(device)
    _resident_cache[dataloader] = (_root(x), _root(y), (x._version, y._version, tuple(x.shape), tuple(y.shape)),
                                   device, xd, yd)
    return xd, yd


class _GraphedLogits:
    def __init__(self, model, x):
        self.shape, self.dtype = tuple(x.shape), x.dtype
        self.x = torch.empty_like(x)
        self.x.copy_(x)
        dev = x.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                model.net(self.x)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with _capture.capture(self.graph):
            self.out = model.net(self.x)

    def __call__(self, x):
        self.x.copy_(x)
        self.graph.replay()
        return self.out


# model -> {key: _GraphedLogits}.  Kept OUTSIDE the module (a hipGraph is neither picklable nor deep-copyable: a cache
# in model.__dict__ broke copy.deepcopy(model) / torch.save(model) after the first evaluation) and weakly keyed, so the
# graphs and their private memory pools go when the model goes.
_eval_graphs = weakref.WeakKeyDictionary()


def _logits_fn(model, x):
    "model.net(x), through a captured graph when the model is on the GPU in eval mode (cached per batch shape)"
    if not (EVAL_GRAPH and x.is_cuda and not model.training and not torch.is_grad_enabled()):
        return model.net(x)
    cache = _eval_graphs.setdefault(model, {})
    # (the capture holds the storage addresses of the parameters AND of the buffers -- the running statistics the
    # BatchNorm kernels read: a model moved, re-built or given re-registered buffers since gets a new capture)
    key = (tuple(x.shape), x.dtype, tuple(p.data_ptr() for p in model.parameters()),
           tuple(b.data_ptr() for b in model.buffers()))
    g = cache.get(key)
    if g is None:
        if len(cache) >= 4:
            cache.clear()
        try:
            g = cache[key] = _GraphedLogits(model, x)
        except RuntimeError as exc:       # an operator that cannot be captured: stay eager for this model
            warnings.warn(f"evaluation forward not captured ({str(exc).splitlines()[0]}); running it eagerly")
            cache[key] = g = False
    return g(x) if g else model.net(x)


def _normalised_logits(model, x):
    """the normalised logits ``model(x)`` = Categorical(logits=net(x) / T) would hold, without building the distribution
    object (its argument validation synchronises with the host once per batch); the forward is replayed from a
    captured graph"""
    f = _logits_fn(model, x)
    f = f if model.softmax_temp == 1 else f / model.softmax_temp
    return f - f.logsumexp(dim=-1, keepdim=True)          # torch/distributions/categorical.py: logits


@torch.no_grad()
def predictive_tables(model, dataloader_test, samples):
    """lps [E, N] and acc_data [E, N, C] (float64, on the model's device)."""
    device = next(iter(model.parameters())).device
    labels = _labels_of(dataloader_test).to(device)
    N = labels.shape[0]
    C = int(labels.max().item()) + 1 if labels.dim() == 1 else labels.shape[1]
    E = _n_samples(samples)
    from .models.base import ClassificationModel
    if (BATCHED and E > 1 and isinstance(model, ClassificationModel) and labels.dim() == 1
            and not model.training and device.type == "cuda"):
        try:
            lps, acc = _predictive_tables_batched(model, dataloader_test, samples, labels, E, C)
        except _NotBatchable as exc:
            warnings.warn(f"grouped posterior-predictive evaluation unavailable ({exc}); evaluating sample by sample")
        else:
            # the reference leaves the model holding the LAST sample (exp_utils.py:262-264 loads each in turn)
            model.load_state_dict({k: v[E - 1] for k, v in samples.items()})
            return lps, acc, labels, "cat"
    lps = torch.zeros((E, N), dtype=torch.float64, device=device)
    acc = torch.zeros((E, N, C), dtype=torch.float64, device=device)
    kind = None
    graphed = (isinstance(model, ClassificationModel) and device.type == "cuda" and not model.training
               and labels.dim() == 1)
    plain_temp = graphed and isinstance(model.softmax_temp, (int, float))
    for e in range(E):
        model.load_state_dict({k: v[e] for k, v in samples.items()})
        i = 0
        # evaluation mode makes every row's prediction a function of that row alone, so the loader's batches are
        # evaluated several at a time (EVAL_ROWS rows per forward): 10 launch-bound forwards of 1,024 rows instead of
        # 79 of 128 for a CIFAR-10 test set -- same numbers row by row (the kernels' arithmetic is per image)
        for bx, by in (_row_groups(dataloader_test, device, EVAL_ROWS) if graphed and plain_temp else dataloader_test):
            bx, by = bx.to(device), by.to(device)
            if graphed and plain_temp:
                # the numbers ``model(bx)`` would hold -- normalised logits and log p(y|x) -- on a captured forward
                a = _normalised_logits(model, bx)
                lp = a.gather(-1, by.view(-1, 1)).squeeze(-1)
                kind = "cat"
                j = i + len(bx)
                lps[e, i:j] = lp
                acc[e, i:j] = a
                i = j
                continue
            preds = model(bx)
            if isinstance(preds, torch.distributions.Categorical):
                kind, a, lp = "cat", preds.logits, preds.log_prob(by)
            elif isinstance(preds, torch.distributions.Normal):
                kind, a, lp = "normal", preds.mean, preds.log_prob(by).sum(-1)
            else:
                raise ValueError(f"unknown likelihood {type(preds)}")
            j = i + len(bx)
            lps[e, i:j] = lp
            acc[e, i:j] = a
            i = j
    return lps, acc, labels, kind


def _log_mean_exp(t, dim):
    return t.logsumexp(dim) - math.log(t.size(dim))


def ensemble_metrics(model, lps, acc, labels, kind):
    lp_each = lps.mean(1)
    out = {"lp_ensemble": _log_mean_exp(lps, 0).mean().item(), "lp_last": lp_each[-1].item()}
    if kind == "cat":
        ens = torch.distributions.Categorical(logits=_log_mean_exp(acc, 0))
        last = torch.distributions.Categorical(logits=acc[-1])
    else:
        ens = torch.distributions.Normal(acc.mean(0), torch.ones_like(acc[0]))
        last = torch.distributions.Normal(acc[-1], ens.scale)
    out["acc_ensemble"] = model.acc_mse(ens, labels).double().mean(0).item()
    out["acc_last"] = model.acc_mse(last, labels).double().mean(0).item()
    return out


def evaluate_model(model, dataloader_test, samples, likelihood_eval=True, accuracy_eval=True,
                   calibration_eval=False):
    """exp_utils.py:250-340.  ``calibration_eval`` adds ``ece`` / ``ace`` / ``rmsce`` of the ensemble's mean
    probabilities (calibration.py: on the device, fp64); categorical likelihoods only, as in the reference."""
    lps, acc, labels, kind = predictive_tables(model, dataloader_test, samples)
    if calibration_eval and (kind != "cat" or labels.dim() != 1):
        raise ValueError(f"Cannot calculate calibration metrics for predictions of type {kind!r}")
    res = ensemble_metrics(model, lps, acc, labels, kind)
    keep = (["lp_ensemble", "lp_last"] if likelihood_eval else []) + \
           (["acc_ensemble", "acc_last"] if accuracy_eval else [])
    out = {k: res[k] for k in keep}
    if calibration_eval:
        from . import calibration
        out.update(calibration.calibration_metrics(labels, calibration.ensemble_probs(acc).probs))
    return out


def evaluate_loo(model, dataloader_train, samples, chains=None):
    """Model comparison on the rows the chains were fitted on (model_comparison.py: PSIS-LOO and WAIC, on the device,
    fp64): ``predictive_tables`` of ``dataloader_train``, then ``loo`` and ``waic`` of its ``lps [E, N]``.  Plain floats:
    ``elpd_loo``, ``elpd_loo_se``, ``p_loo``, ``elpd_waic``, ``p_waic``, ``pareto_k_max`` and ``pareto_k_bad`` (how many
    observations' Pareto-k exceed min(1 - 1 / log10(E), 0.7)).  ``chains=M``: ``samples`` hold M chains of equal length
    one after the other (``gather_samples``' layout); the table is viewed as [M, E / M, N] and
    ``model_comparison.relative_eff`` sets each observation's tail length.  The reference has no such function."""
    from . import model_comparison
    lps = predictive_tables(model, dataloader_train, samples)[0]
    r_eff = None
    if chains is not None:
        M = int(chains)
        if M < 1 or lps.shape[0] % M:
            raise ValueError(f"{lps.shape[0]} samples do not hold {chains} chains of equal length")
        r_eff = model_comparison.relative_eff(lps.unflatten(0, (M, lps.shape[0] // M)))
    res, wres = model_comparison.loo_waic(lps, r_eff)
    return {"elpd_loo": res.elpd_loo, "elpd_loo_se": res.se, "p_loo": res.p_loo, "elpd_waic": wres.elpd_waic,
            "p_waic": wres.p_waic, "pareto_k_max": res.k_max, "pareto_k_bad": float(res.n_bad)}


def evaluate_stein(model, samples, x_train, y_train, temperature=1., thin_to=None, **kw):
    """Do the stored samples target the (tempered) posterior?  (stein.py: the kernel Stein discrepancy with the inverse
    multiquadric kernel and Stein thinning, on the device, fp64.)  ``stein.scores`` differentiates the model's potential
    on (x_train, y_train) at every sample (``x_train = y_train = None`` for a ``PriorOnlyModel``), ``stein.kernel_matrix``
    -- which takes ``**kw``: c, beta, workspace_bytes -- forms the Stein matrix of the model's parameters, moved to the
    current device.  Plain floats ``ksd``, ``v_stat``, ``u_stat``; ``dimension`` and ``nonfinite`` (ints); with
    ``thin_to = m`` also ``kept`` (the list of the m sample indices Stein thinning keeps, in the order picked) and
    ``ksd_thinned`` (the KSD of those m).  The statistic loses power as the dimension grows: compare runs of the same
    model with it.  The reference has no such function."""
    from . import stein
    score = stein.scores(model, samples, x_train, y_train, temperature=temperature)
    x = {k: samples[k][:len(g)].to(device="cuda", dtype=g.dtype) for k, g in score.items()}
    k = stein.kernel_matrix(x, {name: g.to("cuda") for name, g in score.items()}, **kw)
    res = stein.ksd(k)
    out = {"ksd": res.ksd.item(), "v_stat": res.v_stat.item(), "u_stat": res.u_stat.item(), "dimension": k.d,
           "nonfinite": int(k.nonfinite)}
    if thin_to is not None:
        t = stein.thin(k, thin_to)
        out["kept"] = t.indices.tolist()
        out["ksd_thinned"] = t.ksd_path[-1].item()
    return out


def evaluate_eff_dim(model, dataloader_train, samples, n_eigs=20, n_steps=None, alpha=1.0, what="likelihood", **kw):
    """How many directions of weight space do the data determine at each stored sample?  (eff_dim.py: Lanczos with full
    reorthogonalisation, the tridiagonal eigensolver and N_eff = sum lambda / (lambda + alpha) on the device, fp64.)  For
    every sample: load it, run ``n_steps`` Lanczos steps (default 2 ``n_eigs``, at most D and ``eff_dim.MAX_M``; ``n_eigs =
    -1``: all D, for D <= MAX_M) on ``eff_dim.model_hvp(model, x, y, what)`` over the loader's rows, batch by batch, and keep
    the tridiagonal; then ONE batched launch solves all of them.  ``**kw`` goes to the Lanczos loop (seed,
    workspace_bytes, breakdown_rtol).  Plain floats and lists: ``eff_dim`` (per alpha: the mean over the samples),
    ``eff_dim_per_sample`` [S][A], ``eigenvalues`` [S][n_eigs] (the largest Ritz values, ascending), ``max_residual`` (the
    largest Ritz residual estimate among them); ints ``negative`` (Ritz values <= 0 among them), ``restarts``,
    ``dimension``.  N_eff from the largest Ritz values only is a LOWER bound of the Hessian's (every eigenvalue left out
    would add a positive term), and the values are only as accurate as the Hessian-vector product: fp32 for an fp32 model.
    The model's state and mode are left as found.  The reference has no such function."""
    from . import eff_dim
    xs, ys = zip(*((b[0], b[1]) for b in dataloader_train))
    batch = len(xs[0])
    params = [p for _, p in model.named_parameters()]
    dev = params[0].device
    x, y = torch.cat(xs).to(dev), torch.cat(ys).to(dev)
    D = sum(p.numel() for p in params)
    if n_eigs == -1:
        if D > eff_dim.MAX_M:
            raise ValueError(f"n_eigs = -1 needs D <= {eff_dim.MAX_M}; D = {D}")
        k = steps = D
    else:
        k = eff_dim._check_int(n_eigs, "n_eigs", 1, min(D, eff_dim.MAX_M))
        steps = min(2 * k if n_steps is None else eff_dim._check_int(n_steps, "n_steps", k), D, eff_dim.MAX_M)
    if not isinstance(samples, dict) or not samples:
        raise ValueError("samples must be a non-empty dict of [S, *shape] stacks")
    S = _n_samples(samples)
    state = model.state_dict()
    kept = {n: v.detach().clone() for n, v in state.items() if n in samples}
    hvp = eff_dim.model_hvp(model, x, y, what, batch_size=batch)
    if dev.type != "cuda":
        raise ValueError("the model must be on the device (there is no CPU path)")
    if set(kw) - {"seed", "workspace_bytes", "breakdown_rtol"}:
        raise TypeError(f"unexpected arguments {sorted(set(kw) - {'seed', 'workspace_bytes', 'breakdown_rtol'})}")
    seed = kw.get("seed", 0)
    workspace_bytes, rtol = kw.get("workspace_bytes", eff_dim.WORKSPACE_BYTES), kw.get("breakdown_rtol")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    v0 = torch.randn(D, generator=gen, device=dev, dtype=torch.float64)      # the same start vector for every sample
    alphas, betas, restarts = [], [], 0
    try:
        for s in range(S):
            model.load_state_dict({n: v[s] for n, v in samples.items()}, strict=False)
            step, m, r, bad = eff_dim._iterate(hvp, steps, v0, seed, workspace_bytes, rtol)
            if bad:
                raise ValueError(f"sample {s}: the Hessian-vector product has {bad} non-finite elements")
            alphas.append(step.alpha[:m].clone())
            betas.append(step.beta[:m].clone())
            restarts += r
    finally:
        model.load_state_dict(kept, strict=False)
    a, b = torch.stack(alphas), torch.stack(betas)
    theta, Y, _, failed = eff_dim.tridiag_eig(a, b)
    if int(failed.sum()):
        raise RuntimeError("sgmcmc_tridiag_eig: an eigenvalue was not deflated after 60 sweeps")
    m = a.shape[1]
    top = theta[:, m - k:]
    n_eff, nonpos, _ = eff_dim.effective_dimensionality(top, alpha)
    resid = (b[:, m - 1, None] * Y[:, m - 1, m - k:]).abs()
    return {"eff_dim": n_eff.mean(dim=0).tolist(), "eff_dim_per_sample": n_eff.tolist(), "eigenvalues": top.tolist(),
            "max_residual": resid.max().item(), "negative": int(nonpos.sum()), "restarts": restarts, "dimension": D}


def evaluate_prior_sensitivity(model, dataloader_train, dataloader_test, samples, chains=None, per_prior=False,
                               weights=False, alpha=1.01, threshold=0.05):
    """Does the prior matter for this posterior, and for which quantities?  (prior_sensitivity.py: power-scaling
    sensitivity from the stored samples -- a keyed column sort and the weighted-ECDF distance on the device, fp64, the
    weights by ``model_comparison.psis``.)  Every sample is loaded and ``model.log_prior()`` recorded in fp64: the
    component ``"prior"``; with ``per_prior=True`` every prior module's ``log_prob()`` is a component of its own,
    ``"prior:<module name>"`` (selective power-scaling).  The component ``"likelihood"`` is the row sum of
    ``predictive_tables(model, dataloader_train, samples)``' ``lps``.  The quantities are the test table
    ``lps [E, N_test]``; with ``weights=True`` also every stacked floating-point tensor of ``samples``.  ``chains=M``:
    ``samples`` hold M chains of equal length one after the other (``gather_samples``' layout).

    Plain floats and lists: ``components[name]`` = ``sensitive_fraction`` (the share of the quantities with psi >=
    threshold), ``psi_max``, ``psi_median``, ``pareto_k`` (of the powers 1 / alpha and alpha); ``diagnosis`` = how many
    quantities read ``none``, ``conflict`` (prior-data conflict) and ``strong_prior`` (strong prior or weak
    likelihood); ``quantities``; ``pareto_k_bad``: how many of the components' Pareto-k exceed
    ``model_comparison.k_threshold(E)`` -- there is no moment matching, so for those the chain has to be rerun under the
    scaled prior.  The model's state and mode are left as found.  The reference has no such function."""
    from . import model_comparison, prior, prior_sensitivity
    if not isinstance(samples, dict) or not samples:
        raise ValueError("samples must be a non-empty dict of [S, *shape] stacks")
    E = _n_samples(samples)
    M = 1 if chains is None else int(chains)
    if M < 1 or E % M:
        raise ValueError(f"{E} samples do not hold {chains} chains of equal length")
    dev = next(iter(model.parameters())).device
    if dev.type != "cuda":
        raise ValueError("the model must be on the device (there is no CPU path)")
    state = model.state_dict()
    kept = {n: v.detach().clone() for n, v in state.items() if n in samples}
    training = model.training
    parts = {"prior": torch.empty(E, dtype=torch.float64, device=dev)}
    if per_prior:
        parts.update({f"prior:{n}": torch.empty(E, dtype=torch.float64, device=dev) for n, _ in prior.named_priors(model)})
    try:
        with torch.no_grad():
            for s in range(E):
                model.load_state_dict({n: v[s] for n, v in samples.items()}, strict=False)
                parts["prior"][s] = model.log_prior().double()
                if per_prior:
                    for n, pr in prior.named_priors(model):
                        parts[f"prior:{n}"][s] = torch.as_tensor(pr.log_prob()).double()
        parts["likelihood"] = predictive_tables(model, dataloader_train, samples)[0][:E].sum(1)
        tables = [predictive_tables(model, dataloader_test, samples)[0][:E]]
    finally:
        model.load_state_dict(kept, strict=False)
        model.train(training)
    if weights:
        tables += [v[:E].to(dev) for v in samples.values() if v.is_floating_point() and v[0].numel()]
    results = [prior_sensitivity.power_scale_sensitivity(t.unflatten(0, (M, E // M)), parts, alpha, threshold)
               for t in tables]
    out = {"alpha": float(alpha), "threshold": float(threshold), "components": {}}
    for name in parts:
        psi = torch.cat([r.components[name].psi.reshape(-1) for r in results])
        out["components"][name] = {"sensitive_fraction": int((psi >= threshold).sum()) / psi.numel(),
                                   "psi_max": psi.max().item(), "psi_median": psi.median().item(),
                                   "pareto_k": results[0].components[name].pareto_k.tolist()}
    codes = torch.cat([r.diagnosis.reshape(-1) for r in results])
    out["diagnosis"] = {key: int((codes == code).sum()) for key, code in
                        (("none", prior_sensitivity.NONE), ("conflict", prior_sensitivity.CONFLICT),
                         ("strong_prior", prior_sensitivity.STRONG_PRIOR))}
    out["quantities"] = codes.numel()
    limit = model_comparison.k_threshold(E)
    out["pareto_k_bad"] = sum(k > limit for c in out["components"].values() for k in c["pareto_k"])
    return out


@torch.no_grad()
def evaluate_model_average(fits, dataloader_train, dataloader_test, method="stacking"):
    """Model averaging over several fits (model_comparison.py: stacking, pseudo-BMA or pseudo-BMA+ weights, on the
    device, fp64).  ``fits = {name: (model, samples)}``.  The weights come from the pointwise PSIS-LOO densities of
    ``dataloader_train``'s rows (what ``evaluate_loo`` sums); the score is on ``dataloader_test``: each model's pointwise
    lppd there (the log-mean-exp of ``predictive_tables``' ``lps`` over the samples) and ``mixture_lpd`` of those rows.
    -> ``weights`` {name: float}, ``lpd_average`` (the weighted mixture's test log density), ``best_single`` and
    ``lpd_best_single`` (the model with the largest test log density on its own) and ``lpd_uniform`` (equal weights).
    The reference has no such function."""
    from . import model_comparison
    if not isinstance(fits, dict) or not fits:
        raise ValueError("fits must be a non-empty dict {name: (model, samples)}")
    results, test = {}, {}
    for name, (model, samples) in fits.items():
        results[name] = model_comparison.loo(predictive_tables(model, dataloader_train, samples)[0])
        test[name] = _log_mean_exp(predictive_tables(model, dataloader_test, samples)[0], 0)
    weights = model_comparison.model_weights(results, method)
    names = list(weights)
    P = torch.stack([test[n] for n in names])
    K = len(names)
    single = P.sum(1).cpu().tolist()
    best = max(range(K), key=lambda k: -math.inf if math.isnan(single[k]) else single[k])
    return {"weights": weights, "lpd_average": model_comparison.mixture_lpd(P, [weights[n] for n in names])[0],
            "best_single": names[best], "lpd_best_single": single[best],
            "lpd_uniform": model_comparison.mixture_lpd(P, [1.0 / K] * K)[0]}


@torch.no_grad()
def evaluate_marglik(model, train_samples, eval_samples):
    """exp_utils.py:383-406: the model's ``log_prior()`` under every sample -- the parameters of ``train_samples``
    overwritten by those of ``eval_samples`` -- as ``simple_logmarglik`` (their log-mean-exp), ``mean_loglik`` (their
    mean) and ``simple_marglik`` (the mean of their exponentials), in the reference's float32.  Host-side and small."""
    n = _n_samples(train_samples)
    if n != _n_samples(eval_samples):
        raise ValueError(f"{n} train samples but {_n_samples(eval_samples)} eval samples")
    log_priors = []
    for e in range(n):
        model.load_state_dict({**{k: v[e] for k, v in train_samples.items()},
                               **{k: v[e] for k, v in eval_samples.items()}})
        log_priors.append(model.log_prior().item())
    log_priors = torch.tensor(log_priors)
    return {"simple_logmarglik": log_priors.logsumexp(dim=0).item() - math.log(n),
            "mean_loglik": log_priors.mean().item(),
            "simple_marglik": log_priors.exp().mean().item()}


@torch.no_grad()
def logit_tables(model, dataloaders, samples):
    """The normalised logits [E, N_l, C] of every sample on each loader of ``dataloaders`` (float64, on the model's
    device), C taken from the model's output: the loaders' labels are neither read nor needed to be in range.  Per
    sample, one pass over each loader in turn (exp_utils.py:349-362); the model is left holding the last sample."""
    from .models.base import ClassificationModel
    device = next(iter(model.parameters())).device
    E = _n_samples(samples)
    graphed = (isinstance(model, ClassificationModel) and device.type == "cuda" and not model.training
               and isinstance(model.softmax_temp, (int, float)))
    tables = [None] * len(dataloaders)
    for e in range(E):
        model.load_state_dict({k: v[e] for k, v in samples.items()})
        for li, loader in enumerate(dataloaders):
            parts = []
            for bx, _ in (_row_groups(loader, device, EVAL_ROWS) if graphed else loader):
                bx = bx.to(device)
                if graphed:
                    a = _normalised_logits(model, bx)
                else:
                    preds = model(bx)
                    if not isinstance(preds, torch.distributions.Categorical):
                        raise ValueError(f"out-of-distribution scores need a categorical likelihood, not {type(preds)}")
                    a = preds.logits
                parts.append(a)
            a = torch.cat(parts) if len(parts) > 1 else parts[0]
            if tables[li] is None:
                tables[li] = torch.empty((E,) + tuple(a.shape), dtype=torch.float64, device=device)
            elif tables[li].shape[1:] != a.shape:
                raise ValueError("a loader yielded a different number of rows or classes for another sample")
            tables[li][e] = a
    return tables


def evaluate_ood(model, dataloader_train, dataloader_test, samples):
    """exp_utils.py:343-380: AUROC / average precision of the ensemble's max-probability, the in-distribution set
    ``dataloader_train`` as the positive class against the out-of-distribution set ``dataloader_test`` (whose labels
    are ignored).  The score is max_c softmax(logsumexp_e logits - log E) in fp64, which equals the reference's
    mean over samples of ``pred.probs`` (there averaged in float32) -- calibration.py, on the device."""
    from . import calibration
    acc_in, acc_out = logit_tables(model, (dataloader_train, dataloader_test), samples)
    auroc, auprc = calibration.auroc_auprc(calibration.ensemble_probs(acc_in).conf,
                                           calibration.ensemble_probs(acc_out).conf)
    return {"auroc": auroc, "auprc": auprc}


def evaluate_uncertainty(model, dataloader_test, samples, dataloader_ood=None):
    """How uncertain the posterior ensemble is on ``dataloader_test``, and what that uncertainty is worth
    (uncertainty.py, on the device, fp64).  Plain floats.  Means over the rows: ``entropy`` (predictive),
    ``expected_entropy`` (aleatoric), ``mutual_info`` (epistemic, BALD), ``disagreement``, ``nll``, ``brier``, ``acc``.
    Selective prediction under the 0/1 loss: ``aurc`` / ``eaurc`` with the max-prob as the confidence,
    ``aurc_mutual_info`` with the negated mutual information; ``error_auroc``: the AUROC of the max-prob telling the
    correct rows (positive) from the wrong ones, NaN where there are none of either.  With ``dataloader_ood`` (its labels
    are ignored): ``ood_auroc_<s>`` / ``ood_auprc_<s>`` for the scores s = ``max_prob``, ``entropy``, ``mutual_info``,
    the test set being the positive class; ``ood_auroc_max_prob`` is ``evaluate_ood``'s ``auroc``.  The reference has no
    such function."""
    from . import calibration, uncertainty
    loaders = (dataloader_test,) if dataloader_ood is None else (dataloader_test, dataloader_ood)
    labels = _labels_of(dataloader_test)
    if labels.dim() != 1 or labels.dtype.is_floating_point:
        raise ValueError("uncertainty metrics need integer class labels")
    tables = logit_tables(model, loaders, samples)
    if tables[0].shape[1] != labels.shape[0]:
        raise ValueError(f"{labels.shape[0]} labels but the loader yielded {tables[0].shape[1]} rows")
    u = uncertainty.decompose(tables[0], labels.to(tables[0].device))
    means = torch.stack([u.entropy, u.expected_entropy, u.mutual_info, u.disagreement, u.nll, u.brier,
                         u.hit.to(torch.float64)]).mean(1).cpu().tolist()
    out = dict(zip(("entropy", "expected_entropy", "mutual_info", "disagreement", "nll", "brier", "acc"), means))
    wrong = 1 - u.hit
    rc = uncertainty.risk_coverage(u.max_prob, wrong)
    out["aurc"], out["eaurc"] = rc.aurc, rc.eaurc
    out["aurc_mutual_info"] = uncertainty.risk_coverage(-u.mutual_info, wrong).aurc
    right = u.hit.bool()
    conf_right, conf_wrong = u.max_prob[right], u.max_prob[~right]
    out["error_auroc"] = (calibration.auroc_auprc(conf_right, conf_wrong)[0]
                          if conf_right.shape[0] and conf_wrong.shape[0] else math.nan)
    if dataloader_ood is not None:
        s_in, s_out = uncertainty.ood_scores(u), uncertainty.ood_scores(uncertainty.decompose(tables[1]))
        for name in ("max_prob", "entropy", "mutual_info"):
            out[f"ood_auroc_{name}"], out[f"ood_auprc_{name}"] = calibration.auroc_auprc(s_in[name], s_out[name])
    return out


@torch.no_grad()
def regression_tables(model, dataloader, samples):
    """The Gaussian predictions of every sample on ``dataloader``: (mean [E, N, D], scale [E, N, D], y [N, D]), float64 on
    the model's device -- ``preds.mean`` / ``preds.scale`` of ``model(x)`` with each sample loaded in turn, as
    ``predictive_tables`` loads them; the model is left holding the last sample.  ``ValueError`` for a likelihood that
    is not Normal."""
    device = next(iter(model.parameters())).device
    E = _n_samples(samples)
    mean = scale = y = None
    for e in range(E):
        model.load_state_dict({k: v[e] for k, v in samples.items()})
        means, scales, ys = [], [], []
        for bx, by in dataloader:
            preds = model(bx.to(device))
            if not isinstance(preds, torch.distributions.Normal):
                raise ValueError(f"regression scores need a Normal likelihood, not {type(preds)}")
            m = preds.mean
            means.append(m.reshape(len(bx), -1))
            scales.append(preds.scale.expand_as(m).reshape(len(bx), -1))
            if e == 0:
                ys.append(by.to(device).reshape(len(bx), -1))
        m, s = torch.cat(means), torch.cat(scales)
        if e == 0:
            y = torch.cat(ys).to(torch.float64)
            if y.shape != m.shape:
                raise ValueError(f"targets of shape {tuple(y.shape)} but predictions of shape {tuple(m.shape)}")
            mean = torch.empty((E,) + tuple(m.shape), dtype=torch.float64, device=device)
            scale = torch.empty_like(mean)
        elif m.shape != mean.shape[1:]:
            raise ValueError("the loader yielded a different number of rows for another sample")
        mean[e], scale[e] = m, s
    return mean, scale, y


def evaluate_regression(model, dataloader_test, samples, central=(0.5, 0.9, 0.95)):
    """How good the posterior predictive of a regression model is on ``dataloader_test`` (regression.py, on the device,
    fp64): per row and output the equal-weight mixture of the samples' Gaussians.  Plain floats, means over rows and
    outputs: ``rmse`` (the root of the mean squared error of the mixture's mean), ``lpd``, ``crps``, ``var_aleatoric``,
    ``var_epistemic``; ``pit_ks`` and ``calibration_error`` (of the PIT values at ``regression.DEFAULT_LEVELS``) per
    output and then averaged; per level c of ``central`` the interval between the mixture's quantiles at (1 -+ c) / 2:
    ``coverage_<c>`` (the share of targets inside), ``width_<c>`` and ``interval_score_<c>`` (Winkler).  The reference
    has no such function."""
    from . import regression
    central = [float(c) for c in central]
    if not all(0.0 < c < 1.0 for c in central):
        raise ValueError("every central level must lie strictly between 0 and 1")
    mean, scale, y = regression_tables(model, dataloader_test, samples)
    g = regression.predictive(mean, scale, y)
    n = len(central)
    stats = [g.sq_err.mean(), g.lpd.mean(), g.crps.mean(), g.var_aleatoric.mean(), g.var_epistemic.mean()]
    if n:
        q = regression.quantiles(mean, scale, [(1.0 - c) / 2.0 for c in central] + [(1.0 + c) / 2.0 for c in central])
        for i, c in enumerate(central):
            lo, hi = q[i], q[n + i]
            stats += [((lo <= y) & (y <= hi)).sum().to(torch.float64), (hi - lo).mean(),      # (an integer count)
                      regression.interval_score(lo, hi, y, c).mean()]
    regression._check_pit(g.pit, 2)
    table = regression._pit_columns(g.pit, list(regression.DEFAULT_LEVELS), [])
    vals = torch.stack(stats).cpu().tolist()
    out = {"rmse": math.sqrt(vals[0]), "lpd": vals[1], "crps": vals[2], "pit_ks": table[:, 0].mean().item(),
           "calibration_error": table[:, 1].mean().item(), "var_aleatoric": vals[3], "var_epistemic": vals[4]}
    for i, c in enumerate(central):
        inside, width, score = vals[5 + 3 * i:8 + 3 * i]
        out[f"coverage_{c:g}"], out[f"width_{c:g}"], out[f"interval_score_{c:g}"] = inside / y.numel(), width, score
    return out


@torch.no_grad()
def ensemble_across_chains(lps, acc, group=None):
    """Combine the per-chain tables of all ranks into the ensemble over ALL chains'
    samples without gathering them: returns (log-mean-exp of lps [N], of acc [N, C]).

    Per rank: m = max_e x, s = sum_e exp(x - m).  all_reduce(MAX) gives the global
    max M; s * exp(m - M) summed with all_reduce(SUM), the sample counts likewise.
    Works on any backend (RCCL on the GPUs, gloo in the CPU tests)."""
    import torch.distributed as dist
    x = torch.cat([lps.unsqueeze(-1), acc], dim=-1)          # [E, N, C+1]
    m_local = x.max(dim=0).values
    s_local = (x - m_local).exp().sum(dim=0)
    if dist.is_available() and dist.is_initialized():
        m_glob = m_local.clone()
        dist.all_reduce(m_glob, op=dist.ReduceOp.MAX, group=group)
        packed = torch.cat([(s_local * (m_local - m_glob).exp()).reshape(-1),
                            torch.tensor([float(x.shape[0])], dtype=x.dtype, device=x.device)])
        dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
        s_glob, count = packed[:-1].reshape(s_local.shape), packed[-1]
    else:
        m_glob, s_glob, count = m_local, s_local, torch.tensor(float(x.shape[0]), dtype=x.dtype)
    lme = m_glob + s_glob.log() - count.log()
    return lme[..., 0], lme[..., 1:]


def gather_samples(samples, dst=0, group=None):
    """Collect every chain's stored samples (``runner.get_samples()``: name -> [E_c, ...]) on rank
    ``dst`` as name -> [sum_c E_c, ...], chain by chain -- what a single ``samples.pt`` of an
    8-chain run contains (reference: one file per chain, experiments/run_experiment.sh:15-34).
    One all_gather per tensor over RCCL (gloo in the CPU tests); returns None on other ranks."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return samples
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    out = {}
    for name in sorted(samples):
        t = samples[name].contiguous()
        n = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
        counts = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(counts, n, group=group)
        counts = [int(c.item()) for c in counts]
        pad = max(counts)
        buf = torch.zeros((pad,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        buf[:t.shape[0]] = t
        parts = [torch.zeros_like(buf) for _ in range(world)]
        dist.all_gather(parts, buf, group=group)
        if rank == dst:
            out[name] = torch.cat([p[:c] for p, c in zip(parts, counts)])
    return out if rank == dst else None
