"""The bits of the fused dense leapfrog step, route by route: sha256 digests of what every step of every case of
``dense_step_helpers.CASES`` leaves behind.  Needs the MI355X and the built library:

    python tests/golden/make_dense_step_bits.py     ->  tests/golden/dense_step_bits.json

Every chain of a case is put into the start state of tests/test_dense_step_reference.py and driven through the case's
steps exactly as ``_run_single`` / ``_run_multi`` drive it there (``FusedDenseLeapfrog.replay`` /
``MultiChainDense.step``, the same rows, the same metric steps, ``scheduler.step()`` after each).  After every step the
raw bytes of the per-slice partials of that batch size (``gpart``, ``loss_part``, ``corr_part``), of the assembled
gradient ``g_flat`` and of every tensor of theta, momentum and square_avg are hashed.  Nothing here flushes a pending
finalize: the tensors are read, the engine's state is not.

The file was recorded with the library of the commit BEFORE the forward / backward phases of csrc/mlp_hip.inc were
written once for both kernel families; the library is built with -ffp-contract=off, so a later library that performs
the same operations in the same order reproduces every digest (``test_every_route_reproduces_the_recorded_bits``).  The
recording carries the torch and ROCm versions it was made under.  Only tests/dense_step_helpers.py and the package's
public names are used."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import dense_step_helpers as H  # noqa: E402

PATH = os.path.join(HERE, "dense_step_bits.json")


def versions():
    return dict(torch=torch.__version__, rocm=str(torch.version.hip))


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _begin(case, c):
    "chain c of ``case``: a begun runner in the start state the CPU knows, its stepper and its rows per step"
    kw = H.runner_kwargs(case, c)
    r, f = H._begun(c, **kw)
    opt = r.optimizer
    _, _, model = H._problem(c, n=kw["n"], prior=kw["prior"], width=kw["width"], in_features=kw["in_features"],
                             classes=kw["classes"], data_seed=kw["data_seed"])
    theta0 = [p.detach().clone() for p in model.parameters()]
    m0, v0 = H.start_state(case, c, theta0)
    with torch.no_grad():
        for p, t, m, v in zip(r._params, theta0, m0, v0):
            p.copy_(t.to(H.DEV))
            opt.state[p]["momentum_buffer"].copy_(m.to(H.DEV))
            opt.state[p]["square_avg"].copy_(v.to(H.DEV))
    opt.update_preconditioner()
    if case["clamp"]:
        x, y, _ = H._problem(c, n=kw["n"], prior=kw["prior"], width=kw["width"], in_features=kw["in_features"],
                             classes=kw["classes"], data_seed=kw["data_seed"])
        idx0 = H.row_indices(case, c)[0]
        opt.grad_clamp = H.clamp_of(case, theta0, x[:kw["n"]], y[:kw["n"]], idx0, float(model.softmax_temp),
                                    H.prior_specs(model), kw["n"])
    return r, f, H.row_indices(case, c)


def _arrays(case, r, f):
    "name -> tensor of everything a step leaves behind, in a fixed order"
    st = f._by_batch[case["batch"]]
    out = [("gpart", st["gpart"]), ("loss_part", st["loss_part"]), ("corr_part", st["corr_part"]), ("g_flat", f.g_flat)]
    for part, tensors in zip(("theta", "momentum", "square_avg"), H._snapshot(r)):
        out += [(f"{part}{s}", t) for s, t in enumerate(tensors)]
    return out


def tensors_per_step(name, split=None, metric=None, steps=None):
    """drive case ``name`` (optionally with another ``split`` switch, metric steps or number of steps) and yield
    (chain, step, [(array name, tensor clone on the CPU)]) after every step"""
    case = H.case_of(name)
    for k, v in (("split", split), ("metric", metric), ("steps", steps)):
        if v is not None:
            case[k] = v
    chains = [_begin(case, c) for c in range(len(case["n"]))]
    multi = None
    if len(chains) > 1:
        from bnn_priors_amd.fused_dense import MultiChainDense
        multi = MultiChainDense([f for _, f, _ in chains])
    else:
        chains[0][1].split, chains[0][1].direct = case["split"], case["direct"]
    for t in range(case["steps"]):
        metric_step = t in case["metric"]
        if multi is None:
            r, f, idx = chains[0]
            f.replay(idx[t], metrics=metric_step)
        else:
            multi.step([idx[t] for _, _, idx in chains], metrics=metric_step)
        for c, (r, f, _) in enumerate(chains):
            yield c, t, [(n, a.detach().cpu().clone()) for n, a in _arrays(case, r, f)]
        for r, _, _ in chains:
            r.scheduler.step()


def digests(name):
    "case ``name``: [chain][step] -> {array name: sha256 of its bytes}"
    out = {}
    for c, t, arrays in tensors_per_step(name):
        steps = out.setdefault(c, [])
        assert len(steps) == t
        steps.append({n: _sha(a) for n, a in arrays})
    return [out[c] for c in sorted(out)]


def main():
    from bnn_priors_amd import _hip
    rec = dict(versions=versions(), library_sha=_hip.library_sha(), cases={n: digests(n) for n in H.CASES})
    out = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out, "from library", rec["library_sha"], rec["versions"])


if __name__ == "__main__":
    main()
