"""What tests/test_dense_ladder.py and tests/test_dense_step_reference.py share: the builders of a begun runner of a tiny
dense classifier, and the two references a fused dense leapfrog step is held to -- neither of which is code under test:

* ``float64_reference``: the potential  mean cross-entropy - log_prior / N  of Linear-ReLU-Linear-ReLU-Linear written with
  ``F.linear`` / ``F.cross_entropy`` / ``torch.distributions`` on float64 clones of the parameters, differentiated by
  autograd on the CPU;
* ``oracle_transition``: the C oracle's flat-arena transition (oracle/csrc/sgmcmc_oracle.c through ``oracle.flat``), fed
  the gradient the kernel stored.

Everything here except ``_runner`` / ``_begun`` runs without a GPU.  ``python tests/dense_step_helpers.py`` walks every
case of ``CASES`` on the CPU (``dry_run``): the float64 reference, the 1e-3 logit-gap requirement on every row of every
checked step of every chain, and the ``FlatArena`` plumbing with a float32 torch gradient standing in for the kernel's;
``--search NAME`` looks for data seeds that meet the gap requirement."""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

DEV = "cuda:0"
IN, WIDTH, CLASSES = 16, 8, 4

GRAD_BAR = 2e-6          # max|g - ref| <= GRAD_BAR * max|ref| + GRAD_ABS (tests/test_fused_dense.py sets it for the
GRAD_ABS = 1e-9          # one-launch kernel: the same fp32 products in another summation order)
LOGIT_GAP = 1e-3         # no row's accuracy may hinge on fp32 tie-breaking


# ------------------------------------------------------------------ builders
def _problem(c, *, n=48, prior="gaussian", width=WIDTH, in_features=IN, classes=CLASSES, data_seed=None):
    """chain ``c``'s synthetic data set (n training + 8 test rows) and its He-initialised model, on the CPU"""
    from bnn_priors_amd import models
    g = torch.Generator().manual_seed(100 + c if data_seed is None else data_seed)
    x = torch.rand(n + 8, in_features, generator=g)
    y = torch.randint(0, classes, (n + 8,), generator=g)
    torch.manual_seed(10 + c)
    model = models.get_model(x[:2], torch.tensor([0, classes - 1]), "classificationdensenet", width=width, depth=3,
                             weight_prior=prior, weight_scale=2 ** .5, bias_prior="gaussian", bias_scale=1.)
    models.he_initialize(model)
    return x, y, model


def _runner(c, kind="VerletSGLDReject", *, T=1.0, lr=0.01, mom=0.9, n=48, batch=12, prior="gaussian", width=WIDTH,
            seed=None, loader_seed=None, in_features=IN, classes=CLASSES, data_seed=None, **kw):
    "runner ``c`` of the tiny dense classifier on its own synthetic device-resident set (not begun)"
    from bnn_priors_amd.inference_reject import runner_class
    from bnn_priors_amd.storage import MemoryMetrics, MemoryModelSaver
    x, y, model = _problem(c, n=n, prior=prior, width=width, in_features=in_features, classes=classes,
                           data_seed=data_seed)
    mk = torch.utils.data.TensorDataset
    lg = None if loader_seed is None else torch.Generator().manual_seed(loader_seed)
    train = torch.utils.data.DataLoader(mk(x[:n].to(DEV), y[:n].to(DEV)), batch_size=batch, shuffle=True, generator=lg)
    test = torch.utils.data.DataLoader(mk(x[n:].to(DEV), y[n:].to(DEV)), batch_size=8)
    run = dict(epochs_per_cycle=2, warmup_epochs=1, sample_epochs=1, skip=1, metrics_skip=10, cycles=1, precond_update=1,
               sampling_decay="cosine")
    run.update(kw)
    return runner_class(kind)(model=model.to(DEV), dataloader=train, dataloader_test=test, learning_rate=lr,
                              temperature=T, momentum=mom, metrics_saver=MemoryMetrics(), model_saver=MemoryModelSaver(),
                              seed=(99 + c) if seed is None else seed, chain_id=c, **run)


def _begun(*a, **kw):
    r = _runner(*a, **kw)
    r.begin()
    f = r._fused_dense()
    assert f is not None and f.direct and f.split
    return r, f


def _snapshot(runner):
    opt = runner.optimizer
    return ([p.detach().clone() for p in runner._params],
            [opt.state[p]["momentum_buffer"].clone() for p in runner._params],
            [opt.state[p]["square_avg"].clone() for p in runner._params])


class _Counting:
    "the library with every call counted (a thin wrapper around the bound ctypes functions)"

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] += 1
            return fn(*a)
        return call


# ------------------------------------------------------------------ the cases of tests/test_dense_step_reference.py
# name -> dims (in, width, classes), batch, per-chain data-set sizes ``n`` and sampler scalars ``chains`` (kind is one per
# case: it selects the kernel), the weights' prior, the number of consecutive steps and which of them are metric steps,
# the route switches, and the data seed of every chain (found with ``--search``: the gap requirement holds for them).
_B = dict(dims=(20, 8, 10), batch=17, n=(40,), kind="VerletSGLDReject", chains=(dict(T=0.75, mom=0.9),), prior="laplace")
LADDER = [dict(T=1.0, lr=0.01, mom=0.9), dict(T=0.1, lr=0.005, mom=0.5), dict(T=0.0, lr=0.02, mom=0.99)]
STEPS, METRIC = 3, (1,)      # step 0: nothing pending; step 1: a metric step that carries step 0's deferred finalize;
#                              step 2: deferred again, finalized by the flush of the state read that follows it
CASES = {
    "A": dict(dims=(4, 3, 2), batch=1, n=(5,), kind="VerletSGLDReject", chains=(dict(T=1.0, mom=0.9),), prior="gaussian"),
    "B": dict(_B),
    "C": dict(dims=(72, 50, 10), batch=16, n=(64,), kind="HMCReject", chains=(dict(T=1.0, mom=1.0),), prior="student-t"),
    "D": dict(dims=(832, 64, 16), batch=33, n=(70,), kind="SGLDReject", chains=(dict(T=1.0, mom=0.9),), prior="gaussian"),
    "E": dict(dims=(836, 64, 16), batch=33, n=(70,), kind="SGLDReject", chains=(dict(T=1.0, mom=0.9),), prior="gaussian"),
    "F": dict(dims=(784, 50, 10), batch=128, n=(300,), kind="VerletSGLDReject", chains=(dict(T=1.0, mom=0.994),),
              prior="gaussian"),
    "G": dict(_B, split=False),
    "H": dict(_B, direct=False, steps=10, metric=(0, 5)),
    "I": dict(_B, kind="SGLDReject", chains=(dict(T=0.75, mom=0.0),)),
    "J": dict(_B, chains=(dict(T=0.0, mom=0.994),)),
    "K": dict(_B, clamp=True),
    "L": dict(_B, batch=128, n=(200, 200), chains=(dict(T=0.75, mom=0.9, seed=99),) * 2),   # (one seed: one block)
    "Ln": dict(_B, batch=128, n=(200, 168), chains=(dict(T=0.75, mom=0.9),) * 2),
    "M": dict(dims=(16, 8, 4), batch=12, n=(48, 40, 56), kind="VerletSGLDReject", chains=tuple(LADDER), prior="gaussian"),
}
DATA_SEEDS = {"A": (100,), "B": (100,), "C": (100,), "D": (100,), "E": (102,), "F": (103,), "G": (100,), "H": (100,),
              "I": (100,), "J": (100,), "K": (100,), "L": (100, 124), "Ln": (100, 124), "M": (100, 101, 102)}
V_SCALE = (1.0, 0.3, 3.0, 0.1, 10.0, 0.03)     # per-tensor square_avg means: six distinct preconditioners
_KIND = {"VerletSGLDReject": "verlet", "HMCReject": "hmc", "SGLDReject": "sgld"}


def case_of(name):
    case = dict(steps=STEPS, metric=METRIC, split=True, direct=True, clamp=False)
    case.update(CASES[name])
    case["name"], case["seeds"], case["oracle_kind"] = name, DATA_SEEDS[name], _KIND[case["kind"]]
    return case


def runner_kwargs(case, c):
    IN_, W_, C_ = case["dims"]
    sp = dict(lr=0.01)
    sp.update(case["chains"][c])
    return dict(kind=case["kind"], n=case["n"][c], batch=case["batch"], prior=case["prior"], width=W_, in_features=IN_,
                classes=C_, data_seed=case["seeds"][c], **sp)


def row_indices(case, c):
    "per step, chain c's rows: a non-identity draw without replacement that includes row n - 1"
    n, batch = case["n"][c], case["batch"]
    rng = np.random.default_rng(7 + c)
    out = []
    for _ in range(case["steps"]):
        idx = rng.choice(n - 1, batch - 1, replace=False).astype(np.int64)
        idx = np.insert(idx, rng.integers(0, batch), n - 1)
        assert batch == 1 or not np.array_equal(idx, np.arange(batch))
        out.append(np.ascontiguousarray(idx))
    return out


def start_state(case, c, theta0):
    "the momentum and square_avg every chain's checked steps start from (theta: the model's initial values)"
    g = torch.Generator().manual_seed(1000 + c)
    m0 = [torch.randn(t.shape, generator=g) for t in theta0]
    v0 = [(torch.rand(t.shape, generator=g) + 0.5) * s for t, s in zip(theta0, V_SCALE)]
    return m0, v0


# ------------------------------------------------------------------ reference 1: float64
def prior_specs(model):
    "(family, loc, scale, df) of every parameter's prior, in parameter order, as Python floats"
    from bnn_priors_amd.prior import named_priors
    by_param = {id(pr.p): pr for _, pr in named_priors(model)}
    out = []
    for p in model.parameters():
        pr = by_param[id(p)]
        out.append((type(pr).__name__, float(pr.loc), float(pr.scale), float(getattr(pr, "df", 0.0))))
    return out


def _density(spec, dtype):
    family, loc, scale, df = spec
    t = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
    D = torch.distributions
    if family == "Normal":
        return D.Normal(t(loc), t(scale))
    if family == "Laplace":
        return D.Laplace(t(loc), t(scale))
    if family == "StudentT":
        return D.StudentT(t(df), t(loc), t(scale))
    raise ValueError(family)


def potential_and_grad(theta, x, y, softmax_temp, priors, N, dtype=torch.float64):
    """the step's potential on rows (x, y) at ``theta`` (six tensors W1, b1, W2, b2, W3, b3) in ``dtype`` on the CPU:
    dict(loss, acc, gap, log_prior, grads) -- gap: the smallest difference of a row's two largest logits"""
    th = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in theta]
    W1, b1, W2, b2, W3, b3 = th
    h = F.relu(F.linear(x.to(dtype), W1, b1))
    h = F.relu(F.linear(h, W2, b2))
    logits = F.linear(h, W3, b3) / softmax_temp
    loss = F.cross_entropy(logits, y)
    log_prior = sum(_density(sp, dtype).log_prob(t).sum() for sp, t in zip(priors, th))
    (loss - log_prior / N).backward()
    top = logits.detach().topk(2, dim=1).values
    return dict(loss=loss.item(), acc=(logits.argmax(1) == y).double().mean().item(),
                gap=(top[:, 0] - top[:, 1]).min().item(), log_prior=log_prior.item(), grads=[t.grad for t in th])


def float64_reference(theta, x, y, softmax_temp, priors, N):
    return potential_and_grad(theta, x, y, softmax_temp, priors, N, torch.float64)


def gradient_ratio(got, ref, clamp=0.0):
    """largest (max|got - ref| - GRAD_ABS) / max|ref| over the tensors (the bar is GRAD_BAR), ref clamped to +-clamp
    first when a clamp is set"""
    worst = 0.0
    for g, r in zip(got, ref):
        if clamp > 0:
            r = r.clamp(-clamp, clamp)
        err, scale = (g.double() - r).abs().max().item(), r.abs().max().item()
        worst = max(worst, (err - GRAD_ABS) / scale if scale > 0 else (0.0 if err <= GRAD_ABS else math.inf))
    return worst


# ------------------------------------------------------------------ reference 2: the C oracle
def oracle_scalars(kind, group):
    "the oracle's step parameters from an optimizer's param group AFTER the step (the step fills the derived keys in)"
    if kind == "sgld":
        return dict(grad_v=1.0, bhn=group["hn"], bh=group["h"], mom_decay=group["momentum"],
                    noise_std=group["noise_std"] if group["temperature"] > 0 else 0.0, alpha=group["rmsprop_alpha"])
    return dict(grad_v=group["grad_v"], bhn=group["bhn"], bh=group["bh"], mom_decay=group["mom_decay"],
                noise_std=group["noise_std"], alpha=group["rmsprop_alpha"])


def oracle_transition(kind, theta, m, v, g, M, scalars, seed, draw, stream):
    """one ordinary transition of the C oracle on a float32 arena loaded with the pre-step theta / m / v, the
    preconditioners M and the gradient g: (arena after the step, its six fp64 sums per tensor)"""
    from oracle.flat import FlatArena
    fa = FlatArena([t.numel() for t in theta], np.float32)
    for s, (t, mm, vv, gg) in enumerate(zip(theta, m, v, g)):
        for arr, src in ((fa.theta, t), (fa.m, mm), (fa.v, vv), (fa.g, gg)):
            a = src.detach().cpu()
            assert a.dtype == torch.float32
            fa.seg(arr, s)[:] = a.reshape(-1).numpy()
        fa.M[s] = M[s]
    sums = fa.step(kind, seed=seed, draw=draw, stream=stream, flags=0, **scalars).copy()
    return fa, sums


def arena_tensors(fa, arr, like):
    return [torch.from_numpy(fa.seg(arr, s).copy()).view(t.shape) for s, t in enumerate(like)]


# ------------------------------------------------------------------ the CPU walk through every case
def group_scalars(kind, lr, N, a, T):
    "the param-group keys the HIP samplers derive for an ordinary step (mcmc/sgld.py, mcmc/verlet_sgld.py), restated"
    g = dict(lr=lr, num_data=N, momentum=a, temperature=T, rmsprop_alpha=0.99)
    if kind == "sgld":
        g.update(hn=math.sqrt(lr * N), h=math.sqrt(lr / N), noise_std=math.sqrt(2 * (1 - a) * T))
    else:
        g.update(bh=math.sqrt(lr / N), bhn=math.sqrt(lr * N), mom_decay=a, grad_v=1 + a,
                 noise_std=math.sqrt((1 - a ** 2) * T))
    return g


def clamp_of(case, theta0, x, y, idx0, softmax_temp, priors, N):
    "case K's clamp: about the median |g| of the float64 reference of the first step"
    if not case["clamp"]:
        return 0.0
    ref = float64_reference(theta0, x[idx0], y[idx0], softmax_temp, priors, N)
    return float(torch.cat([g.abs().reshape(-1) for g in ref["grads"]]).median())


def dry_run(name, seeds=None, verbose=False, only=None):
    """every chain and checked step of case ``name`` without a GPU: float32 torch autograd stands in for the kernel's
    gradient, the oracle's arena after a step is the state the next one starts from.  Returns the smallest logit gap."""
    from bnn_priors_amd.schedule import get_cosine_schedule
    case = case_of(name)
    if seeds is not None:
        case["seeds"] = seeds
    kind, worst_gap = case["oracle_kind"], math.inf
    for c in range(len(case["n"])) if only is None else (only,):
        kw = runner_kwargs(case, c)
        N, batch = kw["n"], kw["batch"]
        x, y, model = _problem(c, n=N, prior=kw["prior"], width=kw["width"], in_features=kw["in_features"],
                               classes=kw["classes"], data_seed=kw["data_seed"])
        x, y = x[:N], y[:N]
        priors, st = prior_specs(model), float(model.softmax_temp)
        theta = [p.detach().clone() for p in model.parameters()]
        m, v = start_state(case, c, theta)
        means = [vv.double().mean().item() + 1e-8 for vv in v]
        M = [(s / min(means)) ** -0.25 for s in means]
        idx = row_indices(case, c)
        clamp = clamp_of(case, theta, x, y, idx[0], st, priors, N)
        schedule = get_cosine_schedule(-(-N // batch) * 2)
        for t in range(case["steps"]):
            rows = torch.from_numpy(idx[t])
            assert int(rows.max()) == N - 1 and len(set(idx[t].tolist())) == batch
            ref = float64_reference(theta, x[rows], y[rows], st, priors, N)
            assert ref["gap"] >= LOGIT_GAP, (name, c, t, ref["gap"])
            worst_gap = min(worst_gap, ref["gap"])
            g32 = potential_and_grad(theta, x[rows], y[rows], st, priors, N, torch.float32)["grads"]
            if clamp > 0:
                g32 = [g.clamp(-np.float32(clamp), np.float32(clamp)) for g in g32]
            ratio = gradient_ratio(g32, ref["grads"], clamp)
            assert ratio <= 50 * GRAD_BAR, (name, c, t, ratio)        # (torch's own fp32: a sanity check of the reference)
            sc = oracle_scalars(kind, group_scalars(kind, kw["lr"] * schedule(t), N, kw["mom"], kw["T"]))
            fa, sums = oracle_transition(kind, theta, m, v, g32, M, sc, seed=kw.get("seed", 99 + c), draw=2 + t, stream=c)
            assert np.isfinite(sums).all() and np.isfinite(fa.theta).all()
            if kw["mom"] == 0:
                assert all(torch.equal(a, b) for a, b in zip(arena_tensors(fa, fa.m, m), m))
            theta, m, v = (arena_tensors(fa, arr, theta) for arr in (fa.theta, fa.m, fa.v))
            if verbose:
                print(f"  {name} chain {c} step {t}: gap {ref['gap']:.2e} loss {ref['loss']:.4f} acc {ref['acc']:.3f} "
                      f"log_prior {ref['log_prior']:.3f} torch-fp32 ratio {ratio:.1e}")
    return worst_gap


def _search(name, margin=2 * LOGIT_GAP, tries=400):
    "data seeds, chain by chain, whose smallest gap over the checked steps is at least ``margin``"
    seeds = list(DATA_SEEDS[name])
    for c in range(len(seeds)):
        for seed in range(100 + c, 100 + c + tries):
            seeds[c] = seed
            try:
                if dry_run(name, seeds=tuple(seeds), only=c) >= margin:
                    break
            except AssertionError:
                pass
        else:
            raise SystemExit(f"{name}: no seed for chain {c}")
    return tuple(seeds)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) > 2 and sys.argv[1] == "--search":
        for name_ in sys.argv[2:]:
            print(name_, _search(name_), flush=True)
    else:
        for name_ in sys.argv[1:] or CASES:
            print(f"{name_}: smallest logit gap {dry_run(name_, verbose=True):.3e}", flush=True)
