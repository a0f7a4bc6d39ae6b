"""Whole leapfrog step of the dense classifier as a 3-kernel hipGraph.

For ``ClassificationDenseNet`` (Linear-ReLU-Linear-ReLU-Linear, categorical likelihood,
element-wise priors; reference models/dense_nets.py:48-67) a leapfrog step is

    [one async copy: per-step scalars + the minibatch's row indices]
    mlp_fwdbwd_kernel       fused forward + backward on the matrix cores, rows gathered by
                            index from the device-resident data set      (csrc/mlp_hip.inc)
    prior_kernel_indirect   fixed-order sum of the per-slice partial gradients + prior
                            gradient (+ log-prior partials on metric steps)
    step_kernel_indirect    fused sampler transition (noise, momentum, position, RMSprop, dots)
    finalize_small_kernel   energy / temperature bookkeeping, energy total, log-prior total

captured once per batch size (by the library itself, on an internal stream:
``sgmcmc_dense_stepper_create``) and replayed with ONE native call per step that also ships the
per-step scalars and row indices through a ring of pinned slots; metric steps read ONE buffer back.  Numerically
the gradient differs from the autograd path only by fp32 summation order (the one-launch kernel is tested against a
PyTorch reference in tests/test_fused_dense.py; the routes a step actually takes -- the two-launch split, the inline
one-launch kernels, the graph replicas, the multi-chain launches -- against a float64 gradient and, for the transition,
bit for bit against the C oracle in tests/test_dense_step_reference.py); everything downstream is the same code.
"""
import ctypes

import numpy as np
import torch
from torch import nn

from . import _hip
from .graphed import PendingRow, _ReportSlots
from .models.base import ClassificationModel


class IndexBatch:
    """A minibatch named by its row indices into a device-resident data set."""
    __slots__ = ("idx", "X", "Y", "ptr")

    def __init__(self, idx, X, Y):
        self.idx = np.ascontiguousarray(idx, dtype=np.int64)   # host
        self.X, self.Y = X, Y
        self.ptr = self.idx.__array_interface__["data"][0]

    def __len__(self):
        return len(self.idx)

    def materialize(self):
        i = torch.from_numpy(np.ascontiguousarray(self.idx)).to(self.X.device)
        return self.X.index_select(0, i), self.Y.index_select(0, i)


def _dense_layers(model):
    "the three Linear layers if ``model`` is the supported topology, else None"
    if not isinstance(model, ClassificationModel) or not isinstance(model.softmax_temp, (int, float)):
        return None
    net = getattr(model.net, "module", model.net)
    if not isinstance(net, nn.Sequential) or len(net) != 5:
        return None
    lin = [net[0], net[2], net[4]]
    if not all(isinstance(net[i], nn.ReLU) for i in (1, 3)):
        return None
    from .models.nets import Linear
    for l in lin:
        if not isinstance(l, Linear) or l.bias_prior is None:
            return None
    return lin


def _parse_row(v, n_seg):
    "a read-back report row: (dict(loss, acc, nonfinite, log_prior, energy), the per-segment state [n_seg][...])"
    r = dict(loss=float(v[4]), acc=float(v[5]), nonfinite=bool(v[1] != 0.0), log_prior=float(v[2]), energy=float(v[3]))
    return r, v[8:].reshape(n_seg, -1).copy()


class FusedDenseLeapfrog(_ReportSlots):
    @staticmethod
    def supported(potential, optimizer):
        lin = _dense_layers(potential.model)
        eng = optimizer.engine
        if lin is None or not potential.fast or potential.leftover or not eng.small_finalize:
            return False
        if eng.dtype != torch.float32 or len(optimizer.param_groups) != 1:
            return False
        if eng.prior_links or eng.prior_max_kind > _hip.PRIOR_CAUCHY:
            return False       # the step kernel's in-flight prior covers the constant-scale families only
        want = [t for l in lin for t in (l.weight_prior.p, l.bias_prior.p)]
        if len(want) != len(eng.params) or any(a is not b for a, b in zip(want, eng.params)):
            return False
        (h1, i), (h2, h1b), (o, h2b) = (l.weight_prior.p.shape for l in lin)
        return (i % 4 == 0 and h1 == h1b and h2 == h2b and h1 <= 64 and h2 <= 64 and o <= 16
                and _hip.lib().sgmcmc_mlp_lds_bytes(i) <= 160 * 1024)

    def __init__(self, potential, optimizer, X, Y, ring=8, direct=None):
        assert self.supported(potential, optimizer)
        import os
        # three direct launches with by-value arguments vs replaying a captured graph
        self.direct = (os.environ.get("SGMCMC_DENSE_DIRECT", "1") == "1") if direct is None else direct
        # forward/backward as two launches over 4x more workgroups (csrc/mlp_hip.inc, 'two-launch split')
        self.split = True
        self.pot, self.opt, self.eng = potential, optimizer, optimizer.engine
        self.lib = _hip.lib()
        eng, dev = self.eng, optimizer.engine.device
        self.X_source = X      # identity of the data set this stepper gathers from
        self.X = X.to(dev, torch.float32).contiguous().view(X.shape[0], -1)
        self.Y = Y.to(dev, torch.int64).contiguous()
        self.lin = _dense_layers(potential.model)
        # static gradient buffer, packed like the noise index (4-aligned per tensor)
        self.offs = [int(o) for o in eng.seg_host["noise_base"]]
        self.stride = self.offs[-1] + -(-eng.params[-1].numel() // 4) * 4
        self.g_flat = torch.zeros(self.stride, device=dev)
        self.static_grads = [self.g_flat[o:o + p.numel()].view(p.shape)
                             for o, p in zip(self.offs, eng.params)]
        self.nbytes_args = ctypes.sizeof(_hip.StepArgs)
        self._ring, self._k, self._pp = ring, 0, 0
        self._by_batch = {}
        self._init_slots(eng.report.numel())

    # ------------------------------------------------------------------ per batch size
    def _mlp_args(self, *, X, Y, idx, gpart, loss_part, corr_part, batch, grad_scale, split_scratch):
        """the forward/backward kernels' argument struct for ``batch`` rows of the set at (X, Y) (device addresses), named
        by the device index array ``idx`` (None: rows 0..batch-1), the partials going to the given tensors"""
        W1, b1, W2, b2, W3, b3 = self.eng.params
        o = self.offs
        return _hip.MlpArgs(
            X=X, Y=Y, idx=idx, W1=W1.data_ptr(), b1=b1.data_ptr(), W2=W2.data_ptr(), b2=b2.data_ptr(),
            W3=W3.data_ptr(), b3=b3.data_ptr(), gpart=gpart.data_ptr(), loss_part=loss_part.data_ptr(),
            correct_part=corr_part.data_ptr(), gpart_stride=self.stride, off_W1=o[0], off_b1=o[1], off_W2=o[2],
            off_b2=o[3], off_W3=o[4], off_b3=o[5], batch=batch, in_features=W1.shape[1], hidden1=W1.shape[0],
            hidden2=W2.shape[0], out_features=W3.shape[0],
            inv_softmax_temp=1.0 / float(self.pot.model.softmax_temp), trace=None,
            args_src=None, args_dst=None, args_bytes=0, grad_scale=grad_scale, split_scratch=split_scratch)

    def _state_for(self, batch):
        "the per-batch-size state (buffers, argument structs, graph replicas), set up on first use"
        st = self._by_batch.get(batch)
        if st is None:
            st = self._by_batch[batch] = self._setup(batch)
            self._static_flags = st["A"].flags & ~_hip.CALC_METRICS
        return st

    def _setup(self, batch):
        eng, dev = self.eng, self.eng.device
        S = -(-batch // _hip.MLP_ROWS)
        slot_bytes = self.nbytes_args + 8 * batch
        st = dict(batch=batch, S=S)
        st["dev"] = torch.zeros(slot_bytes, dtype=torch.uint8, device=dev)
        st["pinned"] = torch.zeros(self._ring * slot_bytes, dtype=torch.uint8).pin_memory()
        st["gpart"] = torch.zeros(S * self.stride, device=dev)
        st["loss_part"] = torch.zeros(S, device=dev)
        st["corr_part"] = torch.zeros(S, device=dev)
        st["split"] = torch.zeros(self.lib.sgmcmc_mlp_split_scratch_floats(batch), device=dev)
        st["mlp"] = self._mlp_args(X=self.X.data_ptr(), Y=self.Y.data_ptr(), idx=st["dev"].data_ptr() + self.nbytes_args,
                                   gpart=st["gpart"], loss_part=st["loss_part"], corr_part=st["corr_part"], batch=batch,
                                   grad_scale=0.0, split_scratch=st["split"].data_ptr() if self.split else None)
        st["param_ptrs"] = [p.data_ptr() for p in eng.params]
        self._bind_grads()
        eng.refresh(self.opt._preconditioners())
        torch.cuda.synchronize(dev)
        st["A"] = self._args(st.get("A"), False, advance=False)
        handle = ctypes.c_void_p()
        _hip.check(self.lib.sgmcmc_dense_stepper_create(
            ctypes.byref(eng.layout), ctypes.byref(st["mlp"]), ctypes.byref(st["A"]), self.pot.N,
            st["dev"].data_ptr(), st["pinned"].data_ptr(), self._ring, slot_bytes,
            ctypes.byref(handle)), "sgmcmc_dense_stepper_create")
        st["handle"] = handle
        st["App"] = [self._args(None, False, advance=False), self._args(None, False, advance=False)]
        torch.cuda.synchronize(dev)
        return st

    def __del__(self):
        for st in getattr(self, "_by_batch", {}).values():
            try:
                self.lib.sgmcmc_dense_stepper_destroy(st["handle"])
            except Exception:
                pass

    def _args(self, A, calc_metrics, advance=True):
        "fill (or create) the per-step scalar struct for an ordinary step at the CURRENT lr"
        kind, flags, sc = self.opt._plain_step_spec(calc_metrics)
        eng = self.eng
        draw = eng.next_draw() if advance else eng.draw
        if A is None:
            return eng.make_args(0, kind, flags | _hip.WITH_LOG_PRIOR, draw,
                                 grad_clamp=self.opt.grad_clamp, **sc)
        A.flags = self._static_flags | flags
        A.draw = draw
        A.b2h2, A.bh, A.bhn = sc["b2h2"], sc["bh"], sc["bhn"]
        A.mom_decay, A.grad_v, A.noise_std = sc["mom_decay"], sc["grad_v"], sc["noise_std"]
        A.num_data, A.rmsprop_alpha = sc["num_data"], sc["rmsprop_alpha"]
        return A

    def _bind_grads(self):
        params = self.eng.params
        if params[0].grad is not self.static_grads[0]:
            for p, g in zip(params, self.static_grads):
                p.grad = g
            self.eng._seg_dirty = True

    # ------------------------------------------------------------------ exact full-data gradient
    MEGA = 2048   # rows per launch of the fused kernel in the full-data pass (128 workgroups)

    def exact(self):
        """g <- grad[-log_prior/N] + grad[-sum_i log p(y_i|x_i)/N] over the WHOLE device-resident
        data set (reference: inference_reject.py:18-33, one autograd pass per minibatch): the fused
        forward/backward kernel on mega-batches of 2048 rows, fp64 accumulation across them, then
        the prior gradient and log-density.  Returns (loss, log_prior, potential) as 0-d tensors."""
        eng, dev, lib = self.eng, self.eng.device, self.lib
        n_data = self.X.shape[0]
        ex = getattr(self, "_exact_state", None)
        if ex is None:
            S = self.MEGA // _hip.MLP_ROWS
            ex = self._exact_state = dict(
                gpart=torch.zeros(S * self.stride, device=dev), loss_part=torch.zeros(S, device=dev),
                corr_part=torch.zeros(S, device=dev),
                acc=torch.zeros(self.stride, dtype=torch.float64, device=dev),
                gsum=torch.zeros(self.stride, device=dev),
                stats=torch.zeros(2, dtype=torch.float64, device=dev))
        stream = eng.stream()
        self._bind_grads()
        eng.refresh(self.opt._preconditioners())
        in_f = self.X.shape[1]
        for start in range(0, n_data, self.MEGA):
            mb = min(self.MEGA, n_data - start)
            A = self._mlp_args(X=self.X.data_ptr() + 4 * start * in_f, Y=self.Y.data_ptr() + 8 * start, idx=None,
                               gpart=ex["gpart"], loss_part=ex["loss_part"], corr_part=ex["corr_part"], batch=mb,
                               grad_scale=1.0 / self.pot.N, split_scratch=None)
            _hip.check(lib.sgmcmc_mlp_fwdbwd(ctypes.byref(A), stream), "sgmcmc_mlp_fwdbwd")
            last = start + mb >= n_data
            _hip.check(lib.sgmcmc_accumulate_parts(
                ex["gpart"].data_ptr(), -(-mb // _hip.MLP_ROWS), self.stride, ex["acc"].data_ptr(),
                ex["gsum"].data_ptr() if last else None, self.stride, ex["loss_part"].data_ptr(),
                ex["corr_part"].data_ptr(), ex["stats"].data_ptr(), int(start == 0), stream),
                "sgmcmc_accumulate_parts")
        # prior gradient + log-density on top of the accumulated likelihood gradient (one "slice")
        _hip.check(lib.sgmcmc_grad_reduce_prior(
            ctypes.byref(eng.layout), ex["gsum"].data_ptr(), 1, self.stride, ex["loss_part"].data_ptr(),
            ex["corr_part"].data_ptr(), 1, self.pot.N, _hip.CALC_METRICS, None, stream),
            "sgmcmc_grad_reduce_prior")
        eng._touch()
        loss = ex["stats"][0] / self.pot.N
        log_prior = eng.scalars[2].clone()
        return loss, log_prior, loss - log_prior / self.pot.N

    # ------------------------------------------------------------------ replay
    def replay(self, idx, metrics=False, idx_ptr=None, wait=True, calc_metrics=None):
        """One leapfrog step on the rows ``idx`` (host int64 array).  Returns None, or on a
        metric step dict(loss, acc, log_prior, energy, nonfinite) after one read-back."""
        batch = len(idx)
        st = self._by_batch.get(batch)
        eng = self.eng
        if st is not None and any(p.data_ptr() != q for p, q in zip(eng.params, st["param_ptrs"])):
            self.lib.sgmcmc_dense_stepper_destroy(st["handle"])     # parameter storage moved (p.data = ...): re-capture
            del self._by_batch[batch]
        st = self._state_for(batch)
        self._bind_grads()
        if eng._seg_dirty or eng._precond_dirty:
            eng.refresh(self.opt._preconditioners())
        if idx_ptr is None:
            idx_ptr = idx.__array_interface__["data"][0]
        if self.direct and batch <= 256:
            # ping-pong argument structs: the previous step's may still be pending
            self._pp ^= 1
            A = self._args(st["App"][self._pp], metrics if calc_metrics is None else calc_metrics)
            if not metrics and eng.small_finalize:
                A.flags |= _hip.DEFER_FINALIZE      # its bookkeeping rides in the NEXT launch
            pending, eng.pending = eng.pending, None
            err = self.lib.sgmcmc_dense_step_direct(eng.layout, st["mlp"], A, self.pot.N, idx_ptr,
                                                    pending, eng.stream())
            if A.flags & _hip.DEFER_FINALIZE:
                eng.pending = A
        else:
            eng.flush()
            A = self._args(st["A"], metrics if calc_metrics is None else calc_metrics)
            err = self.lib.sgmcmc_dense_stepper_step(st["handle"], A, idx_ptr, eng.stream())
        if err:
            _hip.check(err, "sgmcmc_dense_step")
        eng._state_host = None
        eng.energy_ready = True
        if not metrics:
            return None
        eng.metrics_ready = True
        buf, ev = self._take_slot()
        buf.copy_(eng.report, non_blocking=True)
        ev.record()
        n_seg = eng.n_seg
        return self._hand_over(PendingRow(self, buf, ev, lambda v: _parse_row(v, n_seg)), wait)

    def _hand_over(self, row, wait):
        """what ``replay`` returns on a metric step, given the row's read-back (``get()`` -> (dict, per-segment state)):
        the row itself when the caller does not wait, else its dict -- with the state left for the per-tensor reads and
        the non-finite flag re-armed.  (``multichain.run_dense_lockstep`` hands a chain ITS row of a joint step over
        through this too.)"""
        if not wait:
            return row
        eng = self.eng
        r, state = row.get()
        eng._state_host = state
        if r["nonfinite"]:
            eng.scalars[1].zero_()
        return r


class MultiChainDense:
    """K independent chains of the dense classifier stepped in lock-step by THREE launches per leapfrog step
    (``sgmcmc_dense_step_multi`` / ``sgmcmc_dense_step_multi_args``: grid dimension y = chain) instead of 3 K.

    One chain's launches occupy 33-46 workgroups of the 256 CUs and are latency-bound (a step is three dependent
    launches of 6-12 us whatever the net's size); chains are independent, so K of them -- each with its own
    ``FusedDenseLeapfrog`` (weights, sampler arena, data order, Philox stream) -- share the launches and the GPU does
    K steps in about the time of one.  All chains must have one architecture, one sampler kind, one batch size and one
    metrics cadence, and they share the sweep counter (``engine.draw``): those are properties of the launch.  Everything
    that is a scalar of the transition may differ from chain to chain -- learning rate, temperature (0 included: that
    chain draws no noise), momentum, ``num_data``, ``rmsprop_alpha``, the gradient clamp, the Philox seed -- and so may
    the prior family of every tensor (it comes from the chain's own segment table): a temperature ladder or a sweep
    over step sizes is one ``MultiChainDense``.  Chains whose scalars all agree take ``sgmcmc_dense_step_multi`` (one
    128-byte block for all of them, as before); otherwise every chain's own block travels by value
    (``sgmcmc_dense_step_multi_args``, K x 128 bytes).  Either way chain c's trajectory is bit-identical to the same
    chain stepped alone (tests/test_fused_dense.py, tests/test_dense_ladder.py).  This is an addition to the
    reference's one-process-per-chain model (experiments/run_experiment.sh:15-34), for the small nets only;
    ``multichain.run_dense_lockstep`` drives whole runners through it."""

    def __init__(self, steppers):
        self.steppers = list(steppers)
        K = len(self.steppers)
        if not 1 <= K <= _hip.MAX_CHAINS:
            raise ValueError(f"1..{_hip.MAX_CHAINS} chains per launch")
        s0 = self.steppers[0]
        for s in self.steppers:
            if not (s.direct and s.split and s.eng.small_finalize and s.eng.chunk == _hip.CHUNK_SMALL):
                raise ValueError("multi-chain stepping needs the direct, split fused dense path")
            if [tuple(p.shape) for p in s.eng.params] != [tuple(p.shape) for p in s0.eng.params]:
                raise ValueError("chains must share one architecture")
            if s.opt._KIND != s0.opt._KIND:
                raise ValueError("chains must share one sampler kind (it selects the kernel)")
            if s.X.shape[0] > 65536:
                raise ValueError("16-bit row indices: data sets of up to 65,536 rows")
            if s.eng.prior_flags() != 0:
                raise ValueError("the multi-chain kernels carry the lean prior code only (kinds <= CAUCHY, no links)")
        self.lib, self.device = s0.lib, s0.eng.device
        self._host = (_hip.DenseChain * K)()
        self._dev = torch.zeros(ctypes.sizeof(self._host), dtype=torch.uint8, device=self.device)
        self._uploaded = None
        self._sig = None
        self._idx16 = np.zeros((K, _hip.MLP_BATCH_MULTI), dtype=np.uint16)
        # per-chain argument blocks (ping-pong: the previous step's are still pending) and the pending ones, gathered
        self._blocks = [(_hip.StepArgs * K)(), (_hip.StepArgs * K)()]
        self._refs = [[arr[c] for c in range(K)] for arr in self._blocks]
        self._pend = (_hip.StepArgs * K)()
        self._bp = 0
        self._seeded = [None, None]                # the table signature each array's static fields were filled under

    def _table(self, batch):
        "per-chain pointers, uploaded when any of them changed (first use, roll-back arrays allocated, ...)"
        sig = [batch]
        for s in self.steppers:
            st = s._state_for(batch)
            s._bind_grads()
            if s.eng._seg_dirty or s.eng._precond_dirty:
                s.eng.refresh(s.opt._preconditioners())
            sig.append(id(st))
            sig.append(bytes(s.eng.layout))        # (pointers of the arenas / roll-back arrays: 100-odd bytes)
        if sig == self._sig:                       # nothing moved since the table was last built: the usual step
            return
        self._sig = sig
        for c, s in enumerate(self.steppers):
            st = s._by_batch[batch]
            row = self._host[c]
            ctypes.memmove(ctypes.addressof(row.mlp), ctypes.addressof(st["mlp"]), ctypes.sizeof(_hip.MlpArgs))
            ctypes.memmove(ctypes.addressof(row.layout), ctypes.addressof(s.eng.layout), ctypes.sizeof(_hip.Layout))
            row.num_data, row.chain_id = float(s.pot.N), int(s.eng.chain_id)
        raw = bytes(self._host)
        if raw != self._uploaded:
            self._dev.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))     # synchronous: rare
            self._uploaded = raw

    _SAME = ctypes.sizeof(_hip.StepArgs) - 8       # a block up to its `stream` (the chain id: every chain's own)

    def step(self, idx_list, metrics=False, calc_metrics=None):
        """one leapfrog step of every chain on ITS rows ``idx_list[c]`` (host int arrays of one length <= 128), each
        chain with the scalars of ITS optimizer as they are now (lr, temperature, momentum, ...).
        ``metrics``: returns one dict(loss, acc, log_prior, energy, nonfinite) per chain (after one read-back for
        all), else None; the transition also updates the temperature estimates / log-prior unless
        ``calc_metrics=False`` (the loss and accuracy of this forward pass alone: what
        ``FusedDenseLeapfrog.replay(..., metrics=True, calc_metrics=False)`` gives one chain).
        ValueError, before any chain is stepped or its sweep counter advanced: chains whose sweep counters differ, that
        do not agree on having a momentum (SGLD) or on the static flags of the transition."""
        steppers = self.steppers
        K, batch = len(steppers), len(idx_list[0])
        if len(idx_list) != K or batch > _hip.MLP_BATCH_MULTI or any(len(i) != batch for i in idx_list):
            raise ValueError("one batch size of at most 128 rows for all chains")
        cm = metrics if calc_metrics is None else calc_metrics
        s0 = steppers[0]
        g0 = s0.opt.param_groups[0]
        d0, lr0, t0, a0, n0, r0 = s0.eng.draw, g0["lr"], g0["temperature"], g0["momentum"], g0["num_data"], g0["rmsprop_alpha"]
        uniform = True
        for s in steppers[1:]:
            if s.eng.draw != d0:
                raise ValueError("chains stepped together must share the draw counter (engine.draw): "
                                 f"{[x.eng.draw for x in steppers]}")
            g = s.opt.param_groups[0]
            if (g["lr"] != lr0 or g["temperature"] != t0 or g["momentum"] != a0 or g["num_data"] != n0
                    or g["rmsprop_alpha"] != r0 or s.opt.grad_clamp != s0.opt.grad_clamp or s.eng.seed != s0.eng.seed):
                uniform = False
                if (g["momentum"] > 0) != (a0 > 0):
                    raise ValueError("chains stepped together must agree on having a momentum (a flag of the launch)")
        self._table(batch)
        for c, idx in enumerate(idx_list):
            self._idx16[c, :batch] = idx
        idx16 = np.ascontiguousarray(self._idx16[:, :batch])
        pend = [s.eng.pending for s in steppers]
        p0 = pend[0]
        if uniform:
            # every chain's block would be the same bytes up to its chain id: ONE block for all (the call, and the
            # bits, of before there were per-chain blocks)
            st0 = s0._by_batch[batch]
            s0._pp ^= 1
            A = s0._args(st0["App"][s0._pp], cm)
            A.flags |= _hip.DEFER_FINALIZE
            for s in steppers[1:]:
                s.eng.next_draw()
            # the launch finalizes ONE deferred transition for all chains: they must agree on what is pending.  A chain
            # flushed on its own (a state read, a preconditioner refresh) while another was not would otherwise have its
            # bookkeeping run twice -- or the others' dropped: settle every chain first.  (Likewise chains whose last
            # step had blocks of their own.)
            if any(p is not p0 and ((p is None) != (p0 is None) or p0 is None
                                    or bytes(p)[:self._SAME] != bytes(p0)[:self._SAME]) for p in pend[1:]):
                for s in steppers:
                    s.eng.flush()
            pending = s0.eng.pending
            err = self.lib.sgmcmc_dense_step_multi(self._dev.data_ptr(), ctypes.byref(self._host[0]), K, A,
                                                   idx16.ctypes.data, pending, s0.eng.stream())
            if err:
                _hip.check(err, "sgmcmc_dense_step_multi")
            for s in steppers:
                s.eng.pending = A
        else:
            f0 = s0._static_flags
            if any(s._static_flags != f0 for s in steppers[1:]):
                raise ValueError("chains stepped together must share the transition's flags: "
                                 f"{[s._static_flags for s in steppers]}")
            bp = self._bp ^ 1
            blocks, refs = self._blocks[bp], self._refs[bp]
            # the array about to be written is never one a chain's deferred transition still reads: normally the pending
            # blocks are the OTHER array's (or a stepper's own); whatever led here otherwise, settle first
            mine = {ctypes.addressof(A) for A in refs}
            if any(p is not None and ctypes.addressof(p) in mine for p in pend):
                for s in steppers:
                    s.eng.flush()
                pend = [None] * K
                p0 = None
            if self._seeded[bp] is not self._sig:  # what _args leaves alone: kind, ranges, clamp, seed, chain id
                for s, A in zip(steppers, refs):
                    ctypes.memmove(ctypes.addressof(A), ctypes.addressof(s._by_batch[batch]["App"][0]),
                                   ctypes.sizeof(_hip.StepArgs))
                self._seeded[bp] = self._sig
            self._bp = bp
            for s, A in zip(steppers, refs):
                s._args(A, cm)
                A.flags |= _hip.DEFER_FINALIZE
            # one deferred transition PER CHAIN is finalized by the launch, each with its own block; the chains must
            # still agree on whether one is pending, and on its flags and sweep index: else settle every chain first
            if any((p is None) != (p0 is None) or (p is not None and (p.draw != p0.draw or p.flags != p0.flags))
                   for p in pend[1:]):
                for s in steppers:
                    s.eng.flush()
                p0 = None
            pending = None
            if p0 is not None:
                pending = self._pend
                for c, p in enumerate(pend):
                    ctypes.memmove(ctypes.addressof(pending[c]), ctypes.addressof(p), ctypes.sizeof(_hip.StepArgs))
            err = self.lib.sgmcmc_dense_step_multi_args(self._dev.data_ptr(), ctypes.byref(self._host[0]), K, blocks,
                                                        idx16.ctypes.data, pending, s0.eng.stream())
            if err:
                _hip.check(err, "sgmcmc_dense_step_multi_args")
            for s, A in zip(steppers, refs):
                s.eng.pending = A
        for s in steppers:
            s.eng._state_host = None
            s.eng.energy_ready = True
        if not metrics:
            return None
        for s in steppers:
            s.eng.flush()                    # every chain's bookkeeping, now (the rows read its results) ...
            s.eng.metrics_ready = True
        rows = torch.stack([s.eng.report for s in steppers]).cpu().numpy()      # ... and ONE read-back for all
        out = []
        for s, v in zip(steppers, rows):
            r, s.eng._state_host = _parse_row(v, s.eng.n_seg)
            out.append(r)
        return out
