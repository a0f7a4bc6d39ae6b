"""Per-chain temperature / step size / momentum for the lock-step dense chains: ``sgmcmc_dense_step_multi_args``
(every chain's own block of transition scalars by value), ``MultiChainDense`` choosing between it and the one-block
call, and ``multichain.run_dense_lockstep`` driving whole runners.  The bar everywhere: every chain is bit-identical to
the same chain run alone.

Shapes are the smallest at which the kernels can go wrong: 16 input features (the kernels need ``in % 4 == 0``), hidden
8 and 8, 4 classes; batches of 12 of 48 rows (one partial slice of MLP_ROWS = 16 rows, four batches per epoch), 10 of 50,
and MLP_ROWS + 4 of 3 (MLP_ROWS + 4) rows (two slices, the last one partial)."""
import ctypes

import numpy as np
import pytest
import torch

from bnn_priors_amd import _hip
from dense_step_helpers import CLASSES, IN, LADDER, WIDTH, _begun, _Counting, _runner, _snapshot

ROWS2 = _hip.MLP_ROWS + 4            # a batch of two slices, the second one partial
INVALID = 1                          # hipErrorInvalidValue


# ------------------------------------------------------------------ builders (shared: tests/dense_step_helpers.py)
def _same(a, b, what):
    for part, u, v in zip(("theta", "momentum", "square_avg"), a, b):
        for i, (s, t) in enumerate(zip(u, v)):
            assert torch.equal(s, t), f"{what}: {part} of tensor {i} differs"


def _ladder_vs_twins(specs, steps, metric_steps, n=48, batch=12, expect="sgmcmc_dense_step_multi_args", batches=None):
    """chains built from ``specs`` (keyword sets of ``_runner``) stepped in lock-step, against twins of the same
    construction each stepped alone by its own FusedDenseLeapfrog: after EVERY step theta, momentum and square_avg are
    equal bit for bit, on metric steps the returned dicts too, at the end the per-tensor running scalars"""
    from bnn_priors_amd.fused_dense import MultiChainDense
    K = len(specs)
    rng = np.random.default_rng(5)
    sizes = [batch] * steps if batches is None else batches       # (``batches``: the batch size of every step)
    idx = [[rng.choice(n, sizes[t], replace=False).astype(np.int64) for _ in range(K)] for t in range(steps)]
    chains = [_begun(c, n=n, batch=batch, **sp) for c, sp in enumerate(specs)]
    twins = [_begun(c, n=n, batch=batch, **sp) for c, sp in enumerate(specs)]
    multi = MultiChainDense([f for _, f in chains])
    multi.lib = lib = _Counting(multi.lib)
    for t in range(steps):
        m = t in metric_steps
        rows = multi.step(idx[t], metrics=m)
        assert (rows is not None) == m
        for c, ((r, _), (tr, tf)) in enumerate(zip(chains, twins)):
            row = tf.replay(idx[t][c], metrics=m)
            if m:
                assert rows[c] == row, (t, c, rows[c], row)
            _same(_snapshot(r), _snapshot(tr), f"step {t}, chain {c}")
            r.scheduler.step()
            tr.scheduler.step()
    for c, ((r, _), (tr, _f)) in enumerate(zip(chains, twins)):
        a, b = r.optimizer.engine.fetch_state(), tr.optimizer.engine.fetch_state()      # (flushes what is pending)
        assert np.array_equal(a, b, equal_nan=True), f"running scalars of chain {c}"
    other = ({"sgmcmc_dense_step_multi", "sgmcmc_dense_step_multi_args"} - {expect}).pop()
    assert lib.calls[expect] == steps and lib.calls[other] == 0, lib.calls
    # different chains did different things
    assert not torch.equal(_snapshot(chains[0][0])[0][0], _snapshot(chains[1][0])[0][0])
    return chains



gpu = pytest.mark.gpu


# ------------------------------------------------------------------ 1. differing scalars
@gpu
@pytest.mark.parametrize("n,batch", [(48, 12), (50, 10), (3 * ROWS2, ROWS2)])
def test_chains_with_their_own_scalars_equal_themselves_alone(n, batch):
    """K = 3 Verlet chains, temperature (1, 0.1, 0) -- the last one draws no noise --, lr in ratio 1 : 0.5 : 2, momentum
    (0.9, 0.5, 0.99), own seeds and Philox streams; eight lock-step steps, metrics on steps 0 and 4"""
    _ladder_vs_twins(LADDER, 8, (0, 4), n=n, batch=batch)


@gpu
def test_a_change_of_batch_size_leaves_the_pending_transition_its_own_scalars():
    """the ragged last minibatch of an epoch: the step before the change is no metric step, so every chain's
    bookkeeping is still pending -- with ITS block -- when the per-chain table is rebuilt for the other batch size, and
    it is finalized inside the first launch of that size (12, 12, 2, 12, 12, 2, ...; metrics on steps 0 and 4 only)"""
    _ladder_vs_twins(LADDER, 9, (0, 4), n=50, batches=[12, 12, 2, 12, 12, 2, 12, 2, 12])


@gpu
def test_chains_that_differ_in_temperature_alone_equal_themselves_alone():
    "equal lr and momentum: nothing used to refuse these chains, and all were stepped with chain 0's noise_std"
    _ladder_vs_twins([dict(T=1.0), dict(T=0.1), dict(T=0.0)], 8, (0, 4))


# ------------------------------------------------------------------ 2. prior families
@gpu
def test_gaussian_laplace_and_student_t_chains_share_a_launch():
    chains = _ladder_vs_twins([dict(T=1.0, prior="gaussian"), dict(T=0.1, prior="laplace"),
                               dict(T=0.01, prior="student-t")], 8, (0, 4))
    kinds = [int(r.optimizer.engine.seg_host["prior_kind"][0]) for r, _ in chains]
    assert kinds == [_hip.PRIOR_NORMAL, _hip.PRIOR_LAPLACE, _hip.PRIOR_STUDENT_T]


# ------------------------------------------------------------------ 3. the other sampler kinds
@gpu
def test_sgld_ladder_equals_its_chains_alone():
    _ladder_vs_twins([dict(kind="SGLDReject", **sp) for sp in LADDER], 3, (0,))


@gpu
def test_hmc_ladder_equals_its_chains_alone():
    "HMC: per-chain lr, and the tempered extension's per-chain temperature (mcmc.HMC(..., temperature=T))"
    _ladder_vs_twins([dict(kind="HMCReject", T=T, lr=lr, mom=1.0, tempered=True, warmup_epochs=1, sample_epochs=1)
                      for T, lr in ((1.0, 0.01), (0.1, 0.005), (0.5, 0.02))], 3, (0,))


# ------------------------------------------------------------------ 4. uniform chains: the old entry point
@gpu
def test_chains_with_equal_scalars_still_take_the_one_block_call():
    _ladder_vs_twins([dict(seed=99)] * 3, 8, (0, 4), expect="sgmcmc_dense_step_multi")


# ------------------------------------------------------------------ 5. refusals
@gpu
def test_chains_that_cannot_share_a_launch_are_refused_before_any_launch():
    from bnn_priors_amd.fused_dense import MultiChainDense
    (ra, fa), (rb, fb) = _begun(0), _begun(1, T=0.1)
    _, f_sgld = _begun(2, kind="SGLDReject")
    _, f_wide = _begun(3, width=12)
    with pytest.raises(ValueError, match="sampler kind"):
        MultiChainDense([fa, f_sgld])
    with pytest.raises(ValueError, match="architecture"):
        MultiChainDense([fa, f_wide])
    with pytest.raises(ValueError, match="chains per launch"):
        MultiChainDense([fa] * (_hip.MAX_CHAINS + 1))
    multi = MultiChainDense([fa, fb])
    multi.lib = lib = _Counting(multi.lib)
    rb.optimizer.engine.next_draw()                     # chain 1 one sweep index ahead
    draws = [r.optimizer.engine.draw for r in (ra, rb)]
    before = [_snapshot(r) for r in (ra, rb)]
    idx = [np.arange(12, dtype=np.int64)] * 2
    with pytest.raises(ValueError, match="draw counter"):
        multi.step(idx)
    assert not lib.calls and [r.optimizer.engine.draw for r in (ra, rb)] == draws
    for r, b in zip((ra, rb), before):
        _same(_snapshot(r), b, "a refused step")
    ra.optimizer.engine.next_draw()                     # in step again: now it runs
    multi.step(idx)
    assert lib.calls["sgmcmc_dense_step_multi_args"] == 1


# ------------------------------------------------------------------ 6. / 7. the driver
def _assert_same_run(got, want, c):
    names = want.metrics_saver.names()
    assert got.metrics_saver.names() == names
    for name in names:
        (s1, v1), (s2, v2) = got.metrics_saver.column(name), want.metrics_saver.column(name)
        assert np.array_equal(s1, s2), (c, name)
        assert np.array_equal(v1, v2, equal_nan=True), (c, name, v1, v2)
    a, b = got.model_saver.load_samples(), want.model_saver.load_samples()
    assert set(a) == set(b) and len(b["steps"]) > 0
    for k in b:
        if k != "timestamps":
            assert torch.equal(a[k], b[k]), (c, k)


# The step size at which this ladder both accepts and rejects within two epochs, found with the CPU oracle's sampler
# (oracle/samplers.py, same Philox draws) in place of the HIP one: at 0.1 the T = 0.01 chain's energy falls at both M-H
# points (-0.31, -2.6: accepted whatever the uniform is) and the T = 0.1 chain's second one rises by 19 (accepted with
# probability e^-190); at 0.02 and below nothing is rejected, at 0.05 only the T = 1 chain is.
REJECT_LR = 0.1


def _reject_runner(c, T):
    return _runner(c, T=T, lr=REJECT_LR, mom=0.9, reject_samples=True, cycle_seed=300 + c, cycles=1, metrics_skip=2,
                   epochs_per_cycle=2, warmup_epochs=0, sample_epochs=2, skip=1)


@gpu
def test_lockstep_driver_runs_a_temperature_ladder_as_each_runner_alone():
    """K = 3 VerletSGLDRunnerReject at T = (1, 0.1, 0.01), M-H tests on, two sampling epochs: every metric column
    (rejected, delta_energy, total_energy, lr, acc, ... included) and every stored sample equal ``runner.run()`` of an
    identically built runner alone; somewhere in the run an M-H test accepts and one rejects, so a chain rolled back
    while the others went on"""
    from bnn_priors_amd import multichain
    temps = (1.0, 0.1, 0.01)
    alone = [_reject_runner(c, T) for c, T in enumerate(temps)]
    for r in alone:
        r.run()
    together = [_reject_runner(c, T) for c, T in enumerate(temps)]
    multichain.run_dense_lockstep(together)
    verdicts = []
    for c, (g, w) in enumerate(zip(together, alone)):
        _assert_same_run(g, w, c)
        steps, rej = g.metrics_saver.column("acceptance/rejected")
        verdicts.append([bool(v) for s, v in zip(steps, rej) if s > 0 and not np.isnan(v)])
        assert "_fused_dense" not in g.__dict__           # the runner is its own again
    print("M-H verdicts (rejected) per chain:", verdicts)
    assert all(len(v) == 2 for v in verdicts)
    assert any(any(v) for v in verdicts) and any(not all(v) for v in verdicts), verdicts


@gpu
def test_lockstep_driver_with_a_ragged_last_minibatch_equals_each_runner_alone():
    "50 rows in batches of 12: every epoch ends on a minibatch of 2 rows, and starts again with 12"
    from bnn_priors_amd import multichain
    mk = lambda c, T, lr: _runner(c, T=T, lr=lr, mom=0.9, n=50, reject_samples=True, cycle_seed=300 + c,  # noqa: E731
                                  metrics_skip=4, epochs_per_cycle=3, warmup_epochs=1, sample_epochs=2)
    ladder = ((1.0, 0.01), (0.1, 0.02), (0.01, 0.005))
    alone = [mk(c, T, lr) for c, (T, lr) in enumerate(ladder)]
    for r in alone:
        r.run()
    together = [mk(c, T, lr) for c, (T, lr) in enumerate(ladder)]
    multichain.run_dense_lockstep(together)
    for c, (g, w) in enumerate(zip(together, alone)):
        _assert_same_run(g, w, c)


@gpu
def test_lockstep_driver_runs_plain_sgld_runners_with_their_own_step_sizes():
    from bnn_priors_amd import multichain
    mk = lambda c, lr: _runner(c, kind="SGLD", lr=lr, mom=0.9, metrics_skip=2, loader_seed=40 + c,  # noqa: E731
                               epochs_per_cycle=1, warmup_epochs=0, sample_epochs=1)
    alone = [mk(0, 0.01), mk(1, 0.003)]
    for r in alone:
        r.run()
    together = [mk(0, 0.01), mk(1, 0.003)]
    multichain.run_dense_lockstep(together)
    for c, (g, w) in enumerate(zip(together, alone)):
        _assert_same_run(g, w, c)
    assert not np.array_equal(together[0].metrics_saver.column("loss")[1], together[1].metrics_saver.column("loss")[1])


@gpu
def test_lockstep_driver_refuses_runners_it_cannot_step_together():
    from bnn_priors_amd import multichain
    cases = {
        "class": [_runner(0), _runner(1, kind="SGLDReject")],
        "architecture": [_runner(0), _runner(1, width=12)],
        "batches": [_runner(0), _runner(1, n=60)],
        "metrics_skip": [_runner(0), _runner(1, metrics_skip=3)],
        "priors": [_runner(0), _runner(1, prior="gennorm")],
        "too many": [_runner(c) for c in range(_hip.MAX_CHAINS + 1)],
        "T = 0 among T > 0 with M-H tests": [_runner(0, reject_samples=True), _runner(1, T=0.0, reject_samples=True)],
    }
    for what, runners in cases.items():
        with pytest.raises(ValueError, match="run_dense_lockstep"):
            multichain.run_dense_lockstep(runners)
        assert not any(hasattr(r, "optimizer") for r in runners), what      # refused before anything ran
    # a runner without a fused dense step is an error, not a chain stepped on its own
    runners = [_runner(0), _runner(1)]
    runners[1]._fused = False
    with pytest.raises(ValueError, match="no fused dense step"):
        multichain.run_dense_lockstep(runners)
    assert all(max(r.metrics_saver.rows, default=0) == 0 for r in runners)  # ... before any leapfrog step


# ------------------------------------------------------------------ 8. the entry point's own validation (no device)
def _host_call(K=2, edit=None, pending=False, n_chains=None):
    chain = _hip.DenseChain()
    chain.mlp.batch, chain.mlp.in_features, chain.mlp.hidden1, chain.mlp.hidden2 = 12, IN, WIDTH, WIDTH
    chain.mlp.out_features, chain.mlp.split_scratch = CLASSES, 0x1000
    chain.layout.dtype, chain.layout.chunk_elems = _hip.F32, _hip.CHUNK_SMALL

    def blocks(flags):
        arr = (_hip.StepArgs * _hip.MAX_CHAINS)()
        for a in arr:
            a.kind, a.flags, a.seg_begin, a.seg_end, a.chunk_begin, a.chunk_end, a.draw = _hip.VERLET, flags, 0, 6, 0, 6, 7
        return arr
    A = blocks(_hip.SMALL_FINALIZE | _hip.DEFER_FINALIZE | _hip.WITH_LOG_PRIOR)
    P = blocks(_hip.SMALL_FINALIZE | _hip.DEFER_FINALIZE | _hip.WITH_LOG_PRIOR) if pending else None
    if edit:
        edit(A, P)
    idx = (ctypes.c_uint16 * (_hip.MAX_CHAINS * 12))()
    # (0x1000 stands for the device table: nothing dereferences it before the blocks are known to agree)
    return _hip.lib().sgmcmc_dense_step_multi_args(0x1000, ctypes.byref(chain), K if n_chains is None else n_chains, A,
                                                    ctypes.addressof(idx), P, None)


# (the stand-in addresses below must never reach a kernel: were a host check to regress, a machine with a GPU would
#  launch on them -- so these run where there is no device, which is also where they prove the most)
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="host-side validation is tested without a device")


@no_device
@pytest.mark.parametrize("what,edit,pending", [
    ("kind", lambda A, P: setattr(A[1], "kind", _hip.SGLD), False),
    ("flags", lambda A, P: setattr(A[1], "flags", A[1].flags | _hip.CALC_METRICS), False),
    ("draw", lambda A, P: setattr(A[1], "draw", 8), False),
    ("chunk range", lambda A, P: setattr(A[1], "chunk_end", 5), False),
    ("segment range", lambda A, P: setattr(A[1], "seg_begin", 1), False),
    ("pending draw", lambda A, P: setattr(P[1], "draw", 6), True),
    ("pending flags", lambda A, P: setattr(P[1], "flags", P[1].flags | _hip.CALC_METRICS), True),
    ("no deferred finalize", lambda A, P: [setattr(a, "flags", _hip.SMALL_FINALIZE) for a in A], False),
    ("unknown kind", lambda A, P: [setattr(a, "kind", 3) for a in A], False),
])
def test_entry_point_refuses_blocks_that_disagree_without_touching_a_device(what, edit, pending):
    "the host-side checks of sgmcmc_dense_step_multi_args precede every HIP call: they answer on a machine without a GPU"
    assert _host_call(edit=edit, pending=pending) == INVALID, what


@no_device
def test_entry_point_refuses_too_many_chains_without_touching_a_device():
    assert _host_call(n_chains=_hip.MAX_CHAINS + 1) == INVALID
    assert _host_call(n_chains=0) == INVALID
