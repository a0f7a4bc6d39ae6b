"""The fused dense leapfrog step, through ``FusedDenseLeapfrog.replay`` / ``MultiChainDense.step``, held to two
references that are not code under test (tests/dense_step_helpers.py):

1. the GRADIENT the step assembled and consumed (``p.grad`` afterwards) against float64 autograd on the CPU of
   mean cross-entropy - log_prior / N written with ``F.linear`` / ``F.cross_entropy`` / ``torch.distributions``:
   ``max|g - ref| <= 2e-6 max|ref| + 1e-9`` per tensor (the bar tests/test_fused_dense.py sets for the one-launch kernel);
   on metric steps the returned loss (rel 2e-6, abs 1e-6), accuracy (abs 1e-7; every row's two largest float64 logits
   differ by at least 1e-3, asserted, so no accuracy hinges on an fp32 tie) and log-prior (rel 3e-6, the bar of
   tests/test_priors.py for the fused prior kernel on a float32 arena);
2. the TRANSITION against the C oracle, bit for bit: an ``oracle.flat.FlatArena`` loaded with the pre-step theta,
   momentum, square_avg, the six (distinct) preconditioners and the kernel's own stored gradient reproduces theta,
   momentum and square_avg exactly (``numpy.array_equal``) and the six fp64 sums per tensor to 1e-12.  This comparison
   is exact: nothing in it is a tolerance on the kernel's fp32 results.

Every case starts from a state the CPU knows (the model's initial values; momentum and square_avg from a seeded
generator, per-tensor square_avg means a factor 300 apart, then ``update_preconditioner``) and takes three consecutive
steps: step 0 with nothing pending, step 1 a metric step whose first launch carries step 0's deferred finalize (the
trailing workgroup), step 2 deferred again and settled by the state read that follows.  A step whose bookkeeping must
stay pending (step 0) is checked without anything that flushes it; its six sums are overwritten by the next transition
before they can be read, so they are held to the oracle through what the deferred finalize made of them: the Verlet
energy bookkeeping (``delta_energy`` / ``prev_new_momentum_delta`` per tensor, each chain with ITS ``bhn`` and
preconditioners) is followed from the oracle's sums through all steps and compared wherever the state is settled, and
on metric steps ``est_temperature`` and ``est_config_temp`` (ITS ``num_data``) too.  The graph route (case H)
finalizes in its own launch and has every step's sums compared directly.

Largest gradient error observed on an MI355X, as a fraction of the 2e-6 bar (two runs, the same figures), per route:
  two-launch split, mlp_f1_kernel + mlp_rest_kernel + sgmcmc_step_parts_value   0.13
      (A .06, B .09, C .13, D .12, F .11, I .09, J .09)
  ... with a gradient clamp (K: against the clamped reference, scale = the clamp)   0.23
  inline one-launch kernels, mlp_fwdbwd_kernel_inline / _inline_fin              0.14  (E .14, G .09)
  graph replicas + sgmcmc_step_indirect_parts (H, ten steps)                     0.13
  sgmcmc_dense_step_multi, one block (L)                                         0.18
  sgmcmc_dense_step_multi_args, a block per chain (Ln .18, M .46)                0.46
The transition comparison is exact on every route: theta, momentum and square_avg are the oracle's bits.
"""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

import dense_step_helpers as H

pytestmark = pytest.mark.gpu
DEV = H.DEV

_spec = importlib.util.spec_from_file_location(
    "make_dense_step_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_dense_step_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


def _prepare(case, c):
    "chain c of ``case``: a begun runner put into the start state the CPU knows, and everything its checks need"
    from bnn_priors_amd.fused_dense import FusedDenseLeapfrog
    kw = H.runner_kwargs(case, c)
    r, f = H._begun(c, **kw)
    opt = r.optimizer
    assert FusedDenseLeapfrog.supported(r._potential(), opt)
    x, y, model = H._problem(c, n=kw["n"], prior=kw["prior"], width=kw["width"], in_features=kw["in_features"],
                             classes=kw["classes"], data_seed=kw["data_seed"])
    theta0 = [p.detach().clone() for p in model.parameters()]
    m0, v0 = H.start_state(case, c, theta0)
    with torch.no_grad():
        for p, t, m, v in zip(r._params, theta0, m0, v0):
            p.copy_(t.to(DEV))
            opt.state[p]["momentum_buffer"].copy_(m.to(DEV))
            opt.state[p]["square_avg"].copy_(v.to(DEV))
    opt.update_preconditioner()          # the route a runner takes: M from the per-tensor square_avg means
    M = [float(opt.state[p]["preconditioner"]) for p in r._params]
    assert len(set(M)) == 6 and max(M) / min(M) > 2, M
    ch = types.SimpleNamespace(c=c, r=r, f=f, x=x[:kw["n"]], y=y[:kw["n"]], priors=H.prior_specs(model),
                               st=float(model.softmax_temp), N=kw["n"], idx=H.row_indices(case, c), M=M, clamp=0.0)
    # (delta_energy, prev_new_momentum_delta) per tensor as begin() left them: followed through every step below
    ch.book = opt.engine.fetch_state()[:, 6:8].copy()
    assert r.eff_num_data == ch.N and opt.param_groups[0]["num_data"] == ch.N
    if case["clamp"]:
        ch.clamp = opt.grad_clamp = H.clamp_of(case, theta0, ch.x, ch.y, ch.idx[0], ch.st, ch.priors, ch.N)
        assert ch.clamp > 0
    return ch


def _check(case, ch, t, pre, draw, out, sums_readable, own_group=True):
    """both references for chain ``ch``'s step t, taken from the state ``pre`` with sweep index ``draw``; ``out``: what
    the step returned for this chain (a dict on a metric step).  Returns the gradient error as a fraction of the bar."""
    opt, eng, params = ch.r.optimizer, ch.r.optimizer.engine, ch.r._params
    kind, what = case["oracle_kind"], f"case {case['name']} chain {ch.c} step {t}"
    rows = torch.from_numpy(ch.idx[t])
    assert int(rows.max()) == ch.N - 1, what                 # the data set's last row is in every draw
    # ---- 1. the gradient, against float64
    ref = H.float64_reference(pre[0], ch.x[rows], ch.y[rows], ch.st, ch.priors, ch.N)
    assert ref["gap"] >= H.LOGIT_GAP, (what, ref["gap"])
    got = [p.grad.detach().cpu().clone() for p in params]
    ratio = H.gradient_ratio(got, ref["grads"], ch.clamp)
    print(f"{what}: gradient error {ratio / H.GRAD_BAR:.3f} of the bar, logit gap {ref['gap']:.2e}")
    assert ratio <= H.GRAD_BAR, (what, ratio)
    if ch.clamp > 0:
        c32 = float(np.float32(ch.clamp))
        assert all(g.abs().max().item() <= c32 for g in got), what
        assert sum(int((g.abs() == c32).sum()) for g in got) > 0, what        # ... and the clamp did bite
    flat = ch.f.g_flat.cpu()
    for o, p, nxt in zip(ch.f.offs, params, ch.f.offs[1:] + [ch.f.stride]):
        assert torch.equal(flat[o:o + p.numel()], p.grad.detach().cpu().reshape(-1)), what
        assert not flat[o + p.numel():nxt].any(), (what, "a 4-alignment pad of g_flat was written")
    if out is not None:
        assert out["loss"] == pytest.approx(ref["loss"], rel=2e-6, abs=1e-6), what
        assert out["acc"] == pytest.approx(ref["acc"], abs=1e-7), what
        assert out["log_prior"] == pytest.approx(ref["log_prior"], rel=3e-6), what
        assert out["nonfinite"] is False, what
    # ---- 2. the transition, against the C oracle
    grp = opt.param_groups[0]
    restated = H.group_scalars(kind, grp["lr"], grp["num_data"], grp["momentum"], grp["temperature"])
    restated["rmsprop_alpha"] = grp["rmsprop_alpha"]
    if own_group:      # (the one-block multi-chain call derives chain 0's keys only: the others' are restated alone)
        assert all(grp[k] == v for k, v in restated.items()), (what, grp, restated)
    fa, sums = H.oracle_transition(kind, pre[0], pre[1], pre[2], got, ch.M, H.oracle_scalars(kind, restated),
                                   seed=eng.seed, draw=draw, stream=eng.chain_id)
    post = H._snapshot(ch.r)
    for part, arr, tensors in zip(("theta", "momentum", "square_avg"), (fa.theta, fa.m, fa.v), post):
        for s, tns in enumerate(tensors):
            assert np.array_equal(tns.cpu().numpy().reshape(-1), fa.seg(arr, s)), f"{what}: {part} of tensor {s}"
    if grp["momentum"] == 0:             # NO_MOMENTUM: m is neither read nor written
        assert all(torch.equal(a, b) for a, b in zip(post[1], pre[1])), what
    # the energy bookkeeping every transition's finalize does with ITS scalars (mcmc/verlet_sgld.py: delta_energy +=
    # prev_delta - bhn M g.m_old / 2; prev_delta = -bhn M g.m_new / 2; HMC and SGLD leave both alone), from the
    # oracle's sums: this is where the sums of a step whose finalize was deferred are still seen afterwards
    if kind == "verlet":
        c_gm = -.5 * restated["bhn"] * np.asarray(ch.M)
        ch.book[:, 0] += ch.book[:, 1]
        ch.book[:, 0] += c_gm * sums[:, 1]
        ch.book[:, 1] = c_gm * sums[:, 2]
    if sums_readable:
        state = eng.fetch_state()
        np.testing.assert_allclose(state[:, :6], sums, rtol=1e-12, atol=1e-300, err_msg=what)
        np.testing.assert_allclose(state[:, 6:8], ch.book, rtol=1e-9, atol=1e-12, err_msg=what + ": energy bookkeeping")
        if out is not None:     # est_temperature = m_old.m_old / d, est_config_temp = theta.g N / d
            d = np.array([p.numel() for p in params], dtype=np.float64)
            np.testing.assert_allclose(state[:, 8], sums[:, 3] / d, rtol=1e-11, atol=1e-300, err_msg=what)
            np.testing.assert_allclose(state[:, 9], sums[:, 5] * (ch.N / d), rtol=1e-11, atol=1e-300, err_msg=what)
    return ratio / H.GRAD_BAR


def _run_single(name):
    case = H.case_of(name)
    ch = _prepare(case, 0)
    f, eng = ch.f, ch.r.optimizer.engine
    f.split, f.direct = case["split"], case["direct"]          # (before the first step: _setup reads `split`)
    f.lib = lib = H._Counting(f.lib)
    worst = 0.0
    for t in range(case["steps"]):
        metric = t in case["metric"]
        pre, draw = H._snapshot(ch.r), eng.draw
        out = f.replay(ch.idx[t], metrics=metric)
        assert (out is not None) == metric
        # a direct step that is no metric step leaves its bookkeeping pending: nothing here may flush it before the
        # next step has carried it, so its sums are read only where the step (or the end of the case) settles them
        settled = metric or not case["direct"] or t == case["steps"] - 1
        assert settled or eng.pending is not None
        worst = max(worst, _check(case, ch, t, pre, draw, out, settled))
        assert settled or eng.pending is not None
        ch.r.scheduler.step()
    assert not eng.nonfinite_seen(reset=False)
    route, other = "sgmcmc_dense_step_direct", "sgmcmc_dense_stepper_step"
    if not case["direct"]:
        route, other = other, route
    assert lib.calls[route] == case["steps"] and lib.calls[other] == 0, lib.calls
    print(f"case {name}: largest gradient error {worst:.3f} of the bar")
    return case, ch


def _split_scratch_used(case, ch):
    return bool(ch.f._by_batch[case["batch"]]["split"].any().item())


def _run_multi(name, expect):
    from bnn_priors_amd.fused_dense import MultiChainDense
    case = H.case_of(name)
    chains = [_prepare(case, c) for c in range(len(case["n"]))]
    multi = MultiChainDense([ch.f for ch in chains])
    multi.lib = lib = H._Counting(multi.lib)
    uniform = expect == "sgmcmc_dense_step_multi"
    worst = 0.0
    for t in range(case["steps"]):
        metric = t in case["metric"]
        pre = [H._snapshot(ch.r) for ch in chains]
        draws = [ch.r.optimizer.engine.draw for ch in chains]
        rows = multi.step([ch.idx[t] for ch in chains], metrics=metric)
        assert (rows is not None) == metric
        settled = metric or t == case["steps"] - 1
        for c, ch in enumerate(chains):
            worst = max(worst, _check(case, ch, t, pre[c], draws[c], rows[c] if metric else None, settled,
                                      own_group=c == 0 or not uniform))
        for ch in chains:
            ch.r.scheduler.step()
    for ch in chains:
        assert not ch.r.optimizer.engine.nonfinite_seen(reset=False)
    other = ({"sgmcmc_dense_step_multi", "sgmcmc_dense_step_multi_args"} - {expect}).pop()
    assert lib.calls[expect] == case["steps"] and lib.calls[other] == 0, lib.calls
    # the chains are different problems: their own weights, rows and chain ids
    assert not torch.equal(chains[0].r._params[0], chains[1].r._params[0])
    assert len({ch.r.optimizer.engine.chain_id for ch in chains}) == len(chains)
    print(f"case {name}: largest gradient error {worst:.3f} of the bar")
    return chains


# ------------------------------------------------------------------ the two-launch split (mlp_f1_kernel + mlp_rest_kernel)
@pytest.mark.parametrize("name", ["A", "B", "C", "F", "I", "J", "K"])
def test_split_step_matches_both_references(name):
    """A: one 16-column step (three of the four K quarters empty), one live row.  B: quarters of 0, 1, 0, 1 steps, 4 live
    columns in the last tile, a second slice of one row; Laplace weights.  C: HMC, Student-t weights, quarters 1, 1, 1, 2,
    ragged column and hidden tiles, exactly one full slice.  F: the workload's own shape (12, 12, 12, 13).  I: SGLD
    without momentum (m neither read nor written).  J: T = 0, no noise draw.  K: a gradient clamp at the median |g|."""
    case, ch = _run_single(name)
    assert _split_scratch_used(case, ch)


def test_split_at_its_limit_of_thirteen_steps_per_quarter():
    "D: 832 input columns = 52 steps of 16 = F1_UNROLL per quarter; full hidden and class tiles; SGLD with momentum"
    case, ch = _run_single("D")
    assert _split_scratch_used(case, ch)                 # the split ran: it did not fall back


def test_one_step_more_falls_back_to_the_inline_one_launch_kernels():
    "E: 836 columns -- mlp_fwdbwd_kernel_inline (step 0, 2) and ..._inline_fin (step 1: the trailing finalize block)"
    case, ch = _run_single("E")
    assert not _split_scratch_used(case, ch)             # the split did not run: its scratch is still all zero


def test_inline_one_launch_kernels_on_a_small_shape():
    "G: ``split = False`` before the first step"
    case, ch = _run_single("G")
    assert ch.f._by_batch[case["batch"]]["mlp"].split_scratch is None and not _split_scratch_used(case, ch)


def test_graph_replicas_and_the_indirect_transition():
    """H: ``direct = False`` -- sgmcmc_dense_stepper_step replays the captured launches with the scalars and rows shipped
    through the ring of pinned slots (sgmcmc_step_indirect_parts); ring + 2 steps, so a slot is reused; every step's
    sums are checked (this route finalizes in its own launch)"""
    case, ch = _run_single("H")
    assert case["steps"] == ch.f._ring + 2


# ------------------------------------------------------------------ several chains per launch
def test_two_chains_share_one_block_at_the_batch_limit():
    """L: K = 2 chains with equal scalars and seeds at the 128-row limit of the multi-chain launch take
    sgmcmc_dense_step_multi; each with its own weights, rows and chain id (Philox stream)"""
    _run_multi("L", "sgmcmc_dense_step_multi")


def test_two_chains_with_their_own_num_data():
    """as L with data sets of 200 and 168 rows: ``num_data`` is a scalar of the transition, so the chains no longer share
    one block (sgmcmc_dense_step_multi_args) -- and a kernel that took chain 0's N for chain 1's prior gradient fails
    the float64 reference"""
    chains = _run_multi("Ln", "sgmcmc_dense_step_multi_args")
    assert len({ch.N for ch in chains}) == 2


def test_ladder_of_three_chains_each_with_its_own_scalars():
    "M: T = 1 / 0.1 / 0, learning rate, momentum and the data-set size differ per chain: sgmcmc_dense_step_multi_args"
    chains = _run_multi("M", "sgmcmc_dense_step_multi_args")
    assert len({ch.N for ch in chains}) == 3


# ------------------------------------------------------------------ the bits themselves
@pytest.fixture(scope="module")
def recorded_bits():
    with open(bits.PATH) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", list(H.CASES))
def test_every_route_reproduces_the_recorded_bits(name, recorded_bits):
    """sha256 of gpart / loss_part / corr_part, g_flat and every tensor of theta, momentum and square_avg after every step
    of every chain, against tests/golden/dense_step_bits.json -- recorded (tests/golden/make_dense_step_bits.py) with the
    library as it was before the phases of csrc/mlp_hip.inc were written once for both kernel families.  The library is
    built with -ffp-contract=off: the same operations in the same order are the same bits."""
    want, got = recorded_bits["cases"][name], bits.digests(name)
    assert len(got) == len(want) == len(H.case_of(name)["n"])
    for c, (gc, wc) in enumerate(zip(got, want)):
        assert len(gc) == len(wc) == H.case_of(name)["steps"]
        for t, (gs, ws) in enumerate(zip(gc, wc)):
            assert sorted(gs) == sorted(ws)
            for array in gs:
                assert gs[array] == ws[array], (
                    f"case {name} chain {c} step {t}: {array} differs from the recording "
                    f"(recorded under {recorded_bits['versions']}, running {bits.versions()})")


def _same_trajectory(a, b, what):
    "g_flat, theta, momentum and square_avg of two drives of one problem, after every step"
    a, b = list(a), list(b)
    assert len(a) == len(b) > 0
    for (c, t, xa), (_, _, xb) in zip(a, b):
        xb = dict(xb)
        for array, ta in xa:
            if array not in ("gpart", "loss_part", "corr_part"):      # (per-slice partials: a route's own scratch)
                assert torch.equal(ta, xb[array]), f"{what}: chain {c} step {t}: {array}"


def test_routes_agree_bit_for_bit():
    """The two-launch split, the inline one-launch kernels and the graph replicas run the same phase functions, so
    wherever a K quarter has at most F1_UNROLL = 13 steps they perform the same operations in the same order: B against G
    (``split`` off), B against H (the graph route, with B's metric steps, three steps), and D -- the split at its limit
    -- against D with ``split`` off."""
    B = list(bits.tensors_per_step("B"))
    _same_trajectory(B, bits.tensors_per_step("G"), "B vs G")
    _same_trajectory(B, bits.tensors_per_step("H", metric=H.case_of("B")["metric"], steps=H.case_of("B")["steps"]), "B vs H")
    _same_trajectory(bits.tensors_per_step("D"), bits.tensors_per_step("D", split=False), "D vs D without the split")
