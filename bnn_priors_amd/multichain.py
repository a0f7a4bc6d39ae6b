"""Several chains on ONE GPU from one process: every runner on its own HIP stream, their steps interleaved.

A captured step of the convolutional nets is a chain of ~90 dependent launches, each of which leaves the GPU partly idle at
its boundaries; independent chains fill those gaps (googleresnet: 1.36x one chain's throughput with two chains on two
streams, profiles/r02_bench_googleresnet_stream_chains.json).  The reference runs one chain per process
(experiments/run_experiment.sh:15-34); this is the same set of independent Markov chains -- own model, own data order,
Philox stream = ``chain_id`` -- scheduled differently.  For the dense classifier use ``run_dense_lockstep`` instead:
the chains are a grid dimension of the step's kernels (``fused_dense.MultiChainDense``), and they may differ in
temperature, learning rate, momentum and prior -- a cold-posterior ladder in one process.

    runners = [runner_class("VerletSGLDReject")(model=make_model(), ..., seed=1234, chain_id=c) for c in range(2)]
    multichain.run_on_streams(runners)         # == r.run() for every r, interleaved step by step
    multichain.run_dense_lockstep(runners)     # == r.run() for every r, every leapfrog step ONE set of launches
"""
import time

import torch


def _spin_time(streams, device, cycles, links):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for s in streams:
        with torch.cuda.stream(s):
            for _ in range(links):
                torch.cuda._sleep(cycles)
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


_distinct = {}      # device index -> streams measured to own a hardware queue each
_probes = {}        # device index -> how often the measurement ran (a busy GPU makes it reject good streams: it is repeated)
_reserved = {}      # device index -> handles of the streams that carry a chain's own launches (never handed out as lanes)
MAX_PROBES = 3
# How many streams carry CHAINS at once.  The spin-kernel race finds up to 8 queues that run trivial kernels side by side,
# but with real work the aggregate of K chains on K streams collapses beyond four (googleresnet, round 6,
# profiles/r06_chains_per_gpu.txt: lock-step of 4 chains 1.93 ms, of 5 chains 3.35 ms, of 8 chains 4.93 ms; the same with
# GPU_MAX_HW_QUEUES=16) -- four queues make progress together, a fifth makes the hardware take turns.  More chains than this
# share the four streams (two chains on one stream run back to back, which costs nothing against taking turns): 8 chains
# then run at the aggregate of 4 instead of 0.79 of it.
MAX_CHAIN_STREAMS = 4


def _measure(device, candidates, cycles, links):
    pool = [torch.cuda.Stream(device=device) for _ in range(candidates)]
    for s in pool:                                   # first use of a stream creates its queue: not inside the race
        _spin_time([s], device, 1000, 1)
    alone = min(_spin_time([pool[0]], device, cycles, links) for _ in range(3))
    chosen = []
    for s in pool:
        if len(chosen) == 8:
            break
        if chosen:
            raced = min(_spin_time(chosen + [s], device, cycles, links) for _ in range(2))
            if raced >= 1.5 * alone:                 # (a shared queue gives >= 2.0, distinct queues ~1.0)
                continue
        chosen.append(s)
    return chosen


def concurrent_streams(k, device, exclude=(), candidates=16, cycles=400_000, links=3):
    """Up to ``k`` HIP streams that the GPU really runs side by side (none of them in ``exclude``).

    HIP multiplexes a process's streams onto a few hardware queues (``GPU_MAX_HW_QUEUES``, 4 unless the variable is set
    before the runtime starts -- bench.py sets 8) and two streams that share a queue run their work back
    to back: measured in round 5, chains 3 and 4 of ``run_on_streams`` landed on the queues of chains 1 and 2 and the
    aggregate fell back to two chains' throughput (profiles/r05_chains_per_gpu.txt).  Which stream shares which queue is
    not an API property, so it is measured: every candidate is raced against the streams already chosen with chains of
    one-thread spin kernels (a queue slot and nothing else) and kept when the race takes one chain's time rather than
    two -- about 20 ms.  The race is a wall-clock measurement: with other work on the GPU (ranks sharing it over gloo,
    another process, launches in flight) it rejects streams that are fine.  Hence: a result with fewer than ``k``
    streams is measured again (up to MAX_PROBES times per device, the largest set kept), one with a single stream is
    never kept for the process, and falling short is said out loud.  ``SGMCMC_STREAM_PROBE=0`` skips the measurement:
    ``k`` fresh streams are returned as they are (what round 4 did)."""
    import os
    import warnings
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    skip = {e.cuda_stream for e in exclude}
    if os.environ.get("SGMCMC_STREAM_PROBE", "1") == "0":
        return [torch.cuda.Stream(device=device) for _ in range(k)]

    def usable(chosen):
        return [s for s in chosen if s.cuda_stream not in skip]
    chosen = _distinct.get(device.index, [])
    while len(usable(chosen)) < k and len(chosen) < 8 and _probes.get(device.index, 0) < MAX_PROBES:
        _probes[device.index] = _probes.get(device.index, 0) + 1
        again = _measure(device, candidates, cycles, links)
        if len(again) > len(chosen):
            chosen = again
        if len(chosen) > 1:
            _distinct[device.index] = chosen
    out = usable(chosen)[:k]
    if len(out) < k:
        warnings.warn(f"multichain: {len(out)} concurrent HIP stream(s) found where {k} were asked for (GPU_MAX_HW_QUEUES="
                      f"{os.environ.get('GPU_MAX_HW_QUEUES', 'unset: 4')}; a GPU that is busy during the 20 ms probe also "
                      "hides queues): chains / lanes beyond that share streams and run back to back", stacklevel=2)
    return out


def reserve(streams, device):
    "these streams carry a chain's own launches from now on: ``lanes`` never hands them out"
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    _reserved.setdefault(idx, set()).update(s.cuda_stream for s in streams)


def lanes(k, device, exclude=()):
    """``k`` DISTINCT streams for helper lanes (the exact pass's ``ConcurrentAccumulate``): measured-concurrent streams
    that are nobody's main stream (``reserve``) and not in ``exclude``; when the measured set has fewer, FRESH streams make
    up the number -- a fresh stream may share a hardware queue with another one, but no lane is the same stream twice and
    no lane queues behind another chain's steps (round 5 took the lanes from the chains' own pool: with K chains a
    chain's exact pass ran on the other chains' main streams and the K > 1 samples/s figures contained that
    serialisation)."""
    import warnings
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    taken = _reserved.get(idx, set()) | {e.cuda_stream for e in exclude}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pool = [s for s in concurrent_streams(8, device) if s.cuda_stream not in taken]
    out = pool[:k]
    # torch hands out streams from a fixed pool round-robin: a fresh stream can be one handed out before -- a measured
    # one, a reserved one -- so fresh ones are drawn until their handles are new (the pool's size bounds the draws)
    seen = taken | {s.cuda_stream for s in out}
    for _ in range(4 * k + 64):
        if len(out) == k:
            break
        s = torch.cuda.Stream(device=device)
        if s.cuda_stream not in seen:
            seen.add(s.cuda_stream)
            out.append(s)
    out += [torch.cuda.Stream(device=device) for _ in range(k - len(out))]
    return out


def chain_streams(k, device):
    "one stream per chain for ``k`` chains: at most MAX_CHAIN_STREAMS distinct ones, dealt round-robin (chain c on stream c mod 4)"
    own = concurrent_streams(min(k, MAX_CHAIN_STREAMS), device) or [torch.cuda.Stream(device=device)]
    return spread(own, k)


def spread(streams, n):
    "``n`` streams out of ``streams``, cycling when there are fewer (work on a shared stream simply runs back to back)"
    return [streams[i % len(streams)] for i in range(n)]


def run_on_streams(runners, streams=None):
    """``runner.run()`` for every runner, one HIP stream each, advanced round-robin one minibatch step at a time
    (``run_iter``).  Every chain's results are those of running it alone (the chains share nothing but the GPU)."""
    runners = list(runners)
    if not runners:
        return
    device = next(runners[0].model.parameters()).device
    if streams is None:
        streams = chain_streams(len(runners), device)
    reserve(streams, device)        # (the chains' exact passes take their lanes from the rest)
    main = torch.cuda.current_stream(device)
    for s in streams:
        s.wait_stream(main)
    gens = [r.run_iter() for r in runners]
    alive = list(range(len(runners)))
    while alive:
        for k in list(alive):
            with torch.cuda.stream(streams[k]):
                try:
                    next(gens[k])
                except StopIteration:
                    alive.remove(k)
    for s in streams:
        main.wait_stream(s)


# ------------------------------------------------------------------ dense classifier: K runners, one set of launches per step
class _ReadyRow:
    "a metric row whose read-back has happened (what ``FusedDenseLeapfrog.replay(..., wait=False)`` hands a runner)"

    def __init__(self, r, state):
        self._r, self._state = r, state

    def ready(self):
        return True

    def get(self):
        return self._r, self._state


class _LockstepPort:
    """Stands where a runner's ``FusedDenseLeapfrog`` stands while ``run_dense_lockstep`` drives it: ``replay`` hands the
    minibatch to the group and returns once ALL chains' steps have been launched together; everything else (``exact``,
    ``X_source``, ...) is the chain's own stepper."""

    def __init__(self, group, c, stepper):
        self._group, self._c, self._stepper = group, c, stepper

    def __getattr__(self, name):
        return getattr(self._stepper, name)

    def replay(self, idx, metrics=False, idx_ptr=None, wait=True, calc_metrics=None):
        return self._group.submit(self._c, idx, metrics, wait, calc_metrics)


class _Lockstep:
    """The K generators of ``run_dense_lockstep``.  A chain that reaches a leapfrog step waits inside ``submit`` while the
    chains that have not reached theirs are advanced (each in turn waits likewise); the last one to arrive launches the
    step for all, and every chain then goes on from where it was -- with its own scheduler step, M-H point, roll-back,
    evaluation.  A chain's own scalars are read when the launch is made, i.e. before any chain's code after its step
    has run: exactly the values it would have stepped with alone."""

    def __init__(self, runners):
        self.runners = runners
        self.K = len(runners)
        self.ports = [None] * self.K
        self.req = [None] * self.K
        self.out = None
        self.multi = None
        self.gens = None
        self.done = [False] * self.K

    def port(self, c):
        "runner c's ``_fused_dense()`` while it is driven: the port in front of ITS stepper (never None: no fallback)"
        if self.ports[c] is None:
            r = self.runners[c]
            real = type(r)._fused_dense(r)
            if real is None:
                raise ValueError(f"run_dense_lockstep: runner {c} has no fused dense step (_fused_dense() is None): its "
                                 "model, priors or data set are not what fused_dense.FusedDenseLeapfrog supports")
            self.ports[c] = _LockstepPort(self, c, real)
        return self.ports[c]

    def advance(self, c):
        try:
            next(self.gens[c])
        except StopIteration:
            self.done[c] = True

    def submit(self, c, idx, metrics, wait, calc_metrics):
        assert self.req[c] is None
        self.req[c] = (idx, bool(metrics), calc_metrics)
        mine = self.round
        if all(q is not None for q in self.req):
            self._launch()
        while self.round == mine:        # the others have not all arrived: bring them to their step
            j = next((j for j in range(self.K) if self.req[j] is None), None)
            if j is None or self.done[j]:
                raise RuntimeError(f"run_dense_lockstep: chain {c} is at a leapfrog step that chain {j} never reaches "
                                   "(the runners are not in lock-step)")
            self.advance(j)
        if not metrics:
            return None
        stepper = self.ports[c]._stepper
        state, stepper.eng._state_host = stepper.eng._state_host, None
        return stepper._hand_over(_ReadyRow(self.out[c], state), wait)

    round = 0

    def _launch(self):
        from .fused_dense import MultiChainDense
        if self.multi is None:
            self.multi = MultiChainDense([p._stepper for p in self.ports])
        idx, metrics, calc = self.req[0]
        if any(q[1] != metrics or q[2] != calc or len(q[0]) != len(idx) for q in self.req[1:]):
            raise RuntimeError("run_dense_lockstep: the chains disagree on this step's metrics or batch size "
                               "(the runners are not in lock-step)")
        out = self.multi.step([q[0] for q in self.req], metrics=metrics, calc_metrics=calc)
        self.out = out
        self.req = [None] * self.K
        self.round += 1


def _lockstep_check(runners):
    "everything that can be told before a runner has an optimizer: ValueError when the runners cannot be stepped together"
    from . import _hip
    from .fused_dense import _dense_layers
    from .prior import named_priors
    if not 1 <= len(runners) <= _hip.MAX_CHAINS:
        raise ValueError(f"run_dense_lockstep: 1..{_hip.MAX_CHAINS} (SGMCMC_MAX_CHAINS) runners, got {len(runners)}")
    r0 = runners[0]

    def shapes(r):
        return [tuple(p.shape) for p in r._params]

    def layout(r):
        dl = r.dataloader
        return dict(rows=len(dl.dataset), batch_size=dl.batch_size, batches=len(dl), drop_last=dl.drop_last,
                    metrics_skip=r.metrics_skip, epochs_per_cycle=r.epochs_per_cycle, warmup_epochs=r.warmup_epochs,
                    sample_epochs=r.sample_epochs, skip=r.skip, cycles=r.cycles, precond_update=r.precond_update,
                    reject_samples=r.reject_samples, trajectory_length=getattr(r, "trajectory_length", None),
                    has_momentum=r.momentum > 0, device=r._device)
    for c, r in enumerate(runners):
        if type(r) is not type(r0):
            raise ValueError(f"run_dense_lockstep: runner {c} is a {type(r).__name__}, runner 0 a {type(r0).__name__}")
        if shapes(r) != shapes(r0):
            raise ValueError(f"run_dense_lockstep: runner {c}'s architecture {shapes(r)} is not runner 0's {shapes(r0)}")
        a, b = layout(r), layout(r0)
        if a != b:
            diff = {k: (a[k], b[k]) for k in a if a[k] != b[k]}
            raise ValueError(f"run_dense_lockstep: runner {c} and runner 0 differ in {diff}: chains in lock-step share the "
                             "data set size, batch size, metrics cadence and the cycle / epoch layout")
        if not r.use_graph or _dense_layers(r.model) is None:
            raise ValueError(f"run_dense_lockstep: runner {c}'s model is not the dense classifier of the fused step "
                             "(or use_graph=False)")
        if [len(sh) for sh in shapes(r)] != [2, 1, 2, 1, 2, 1]:
            raise ValueError(f"run_dense_lockstep: runner {c}'s parameters {shapes(r)} are not three Linear layers'")
        (h1, i), _, (h2, _), _, (o, _), _ = shapes(r)
        if (i % 4 or h1 > 64 or h2 > 64 or o > 16 or any(p.dtype != torch.float32 for p in r._params)
                or _hip.lib().sgmcmc_mlp_lds_bytes(i) > 160 * 1024):
            raise ValueError(f"run_dense_lockstep: runner {c}'s layer sizes {shapes(r)} / dtype are not the fused dense "
                             "step's (float32, inputs a multiple of 4, hidden <= 64, classes <= 16)")
        if not getattr(r._batches(), "fast", False):
            raise ValueError(f"run_dense_lockstep: runner {c}'s data set is not device resident (a TensorDataset of two "
                             "tensors behind a plain DataLoader): the fused dense step gathers its rows by index")
        for name, pr in named_priors(r.model):
            if getattr(pr, "is_component", False):
                continue
            spec = pr.fused_spec()
            if spec is None or spec[0] > _hip.PRIOR_CAUCHY or pr.scale_link() is not None:
                raise ValueError(f"run_dense_lockstep: runner {c}'s prior {name} ({type(pr).__name__}) is not one the "
                                 "multi-chain kernels carry (constant-scale Normal, Laplace, Student-t, Cauchy)")
    dl = r0.dataloader
    if dl.batch_size is None or dl.batch_size > _hip.MLP_BATCH_MULTI or len(dl.dataset) > 65536:
        raise ValueError(f"run_dense_lockstep: batches of at most {_hip.MLP_BATCH_MULTI} rows of a data set of at most "
                         "65,536 rows")
    if r0.reject_samples:
        zero = [r.temperature == 0 for r in runners]
        if any(zero) and not all(zero):
            # maybe_reject draws its uniform only when T > 0: such chains would leave the shared sweep counter
            raise ValueError("run_dense_lockstep: with reject_samples, chains at temperature 0 and chains above it do not "
                             "consume the same Philox sweep indices and cannot share a launch")


def run_dense_lockstep(runners):
    """``runner.run()`` for every one of K runners of the dense classifier, every ordinary minibatch leapfrog step of the
    K chains being ONE ``MultiChainDense.step`` (three launches for all of them).  The runners are of one class (any
    of the six), one architecture, one data-set size and batch size and one ``metrics_skip`` / cycle / epoch layout;
    they may differ in temperature, learning rate, momentum, priors, seeds, ``cycle_seed`` and sinks -- the ladder
    of a cold-posterior sweep.  Everything but the leapfrog step is each chain's own runner code, in the order it runs
    it alone: ``begin()``, M-H points with their exact pass, roll-backs (a chain that rejects rolls back alone),
    evaluation, stored samples, scheduler steps, preconditioner updates, metric rows.  Every chain's metrics and samples
    are those of ``runner.run()`` alone, bit for bit (tests/test_dense_ladder.py).

    ValueError before anything runs when the runners cannot be stepped together -- class, shapes, layout, priors,
    data source, layer sizes: every reason for a missing fused dense step that can be told from the runner and its model.
    What only the runner's optimizer can tell (it exists once ``run_iter`` has made it: several parameter groups, an
    arena too large for the one-workgroup finalize) is caught where the runner first asks for its stepper, as a
    ValueError too: before any leapfrog step of any chain, but after the ``begin()`` -- exact pass, first
    ``initial_step``, metric row 0 -- of the runners before it.  There is no fallback to stepping a chain on its own."""
    runners = list(runners)
    if not runners:
        return
    _lockstep_check(runners)
    group = _Lockstep(runners)
    for c, r in enumerate(runners):
        if "_fused_dense" in r.__dict__:
            raise ValueError(f"run_dense_lockstep: runner {c} is being driven already")
    try:
        for c, r in enumerate(runners):
            r._fused_dense = (lambda c=c: group.port(c))
        group.gens = [r.run_iter() for r in runners]
        while not all(group.done):
            for c in range(group.K):
                if not group.done[c]:
                    group.advance(c)
    finally:
        for r in runners:
            r.__dict__.pop("_fused_dense", None)
        for g in group.gens or ():
            g.close()
