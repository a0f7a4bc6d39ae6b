"""The trunk convolutions' default kernels on PREPARED weight fragments (csrc/conv_hip.inc ``FRAG``;
``sgmcmc_conv3x3_wfrag_fwd`` / ``_bwd``; conv.WEIGHT_FRAGS) and the stem's forward as the carrier of the fragment jobs
(``sgmcmc_conv_stem_fwd_frags``): the registers hold the values the raw-weight route permutes into them and the MFMA
order is the same, so every result is compared with ``torch.equal`` -- there is no tolerance in this file.  Outputs start
as NaN, so an element nobody wrote shows."""
import ctypes
import types
import warnings

import numpy as np
import pytest
import torch

from bnn_priors_amd import _hip, conv

pytestmark = pytest.mark.gpu
NAN = float("nan")
SHAPES = [(16, 32), (32, 16), (64, 8)]
FORMS = [_hip.FRAG_LDS, _hip.FRAG_REG]
FULL = {shape: {"fwd", "dgrad"} for shape in SHAPES}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _data(c, hw, n, seed=0):
    g = torch.Generator().manual_seed(1000 * c + n + seed)
    x = torch.randn(n, c, hw, hw, generator=g)
    w = torch.randn(c, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** .5
    dy = torch.randn(n, c, hw, hw, generator=g)
    return x.cuda(), w.cuda(), dy.cuda()


def _frag_jobs(ws):
    "-> (ctypes job array, [forward buffers], [data-gradient buffers]), the buffers NaN"
    fwd, dgrad = [torch.full((w.numel(),), NAN, device="cuda") for w in ws], [torch.full((w.numel(),), NAN, device="cuda") for w in ws]
    jobs = (_hip.FragJob * len(ws))()
    for j, w, f, d in zip(jobs, ws, fwd, dgrad):
        j.w, j.fwd, j.dgrad, j.channels = w.data_ptr(), f.data_ptr(), d.data_ptr(), w.shape[0]
    return jobs, fwd, dgrad


def _prepared(lib, ws):
    "the fragments of ``ws`` by sgmcmc_conv3x3_prepare_weights -> ([forward], [data gradient])"
    jobs, fwd, dgrad = _frag_jobs(ws)
    _hip.check(lib.sgmcmc_conv3x3_prepare_weights(ctypes.cast(jobs, ctypes.c_void_p), len(ws), _stream()), "prepare_weights")
    torch.cuda.synchronize()
    return fwd, dgrad


def _host_fragments(w):
    """the layout formula of csrc/conv2_hip.inc on the host: float e = ((ct KS + h) (QW / 4) + q4) 256 + lane 4 + comp is
    k-step qi = 4 q4 + comp = rs KK + k2 of half h: channel 4 (h KK + k2) + (lane >> 4), n = 16 ct + (lane & 15)"""
    w = w.cpu().numpy()
    C = w.shape[0]
    KS = 2 if C == 64 else 1
    KK = C // 4 // KS
    QW = 9 * KK
    e = np.arange(9 * C * C)
    comp, lane, rest = e & 3, (e >> 2) & 63, e >> 8
    q4, h, ct = rest % (QW // 4), (rest // (QW // 4)) % KS, rest // (QW // 4) // KS
    qi = 4 * q4 + comp
    rs, k2 = qi // KK, qi % KK
    ch, n = 4 * (h * KK + k2) + (lane >> 4), ct * 16 + (lane & 15)
    flat = w.reshape(C, C, 9)
    return flat[n, ch, rs], flat[ch, n, 8 - rs]


# ---- 1. forward -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS, ids=["lds", "reg"])
@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("c,hw", SHAPES)
def test_forward_on_fragments_equals_the_raw_weight_kernel(c, hw, n, form):
    "y and the statistics slices; n = 5 is no multiple of the 8 XCDs (identity block order), n = 16 is"
    lib, s = _hip.lib(), _stream()
    x, w, _ = _data(c, hw, n)
    slices = lib.sgmcmc_conv3x3_stat_slices(n, c, hw)
    outs = []
    for route in ("raw", "frag"):
        y = torch.full_like(x, NAN)
        stats = torch.full((c, slices, 2), NAN, dtype=torch.float64, device="cuda")
        if route == "raw":
            _hip.check(lib.sgmcmc_conv3x3(x.data_ptr(), w.data_ptr(), y.data_ptr(), n, c, hw, 0, stats.data_ptr(), s), "raw")
        else:
            frag = _prepared(lib, [w])[0][0]
            _hip.check(lib.sgmcmc_conv3x3_wfrag_fwd(x.data_ptr(), frag.data_ptr(), y.data_ptr(), n, c, hw, stats.data_ptr(),
                                                    form, s), "sgmcmc_conv3x3_wfrag_fwd")
        torch.cuda.synchronize()
        outs.append((y, stats))
    (y0, st0), (y1, st1) = outs
    assert not torch.isnan(y0).any() and not torch.isnan(st0).any()
    assert torch.equal(y1, y0) and torch.equal(st1, st0)


# ---- 2. backward ----------------------------------------------------------------------------------------------------

def _backward(lib, c, hw, n, add, form, riders):
    """the merged backward launch with the sums epilogue (``add``: + the shortcut's add), its slabs reduced by the entry
    point itself; form None: the raw-weight route; riders: (part, P, taps, numel) jobs -> dx, partial, slabs, dw, [ridden]"""
    s = _stream()
    x, w, dy = _data(c, hw, n, 77)
    g = torch.Generator().manual_seed(7 + n)
    out = torch.randn(x.shape, generator=g).relu().cuda()
    y_bn, mean, invstd = (torch.randn(x.shape, generator=g).cuda(), torch.randn(c, generator=g).cuda() * .1,
                          torch.rand(c, generator=g).cuda() + .5)
    e_dout, e_out = torch.randn(x.shape, generator=g).cuda(), torch.randn(x.shape, generator=g).cuda()
    dx, dw = torch.full_like(x, NAN), torch.full_like(w, NAN)
    partial = torch.full((c, lib.sgmcmc_conv3x3_stat_slices(n, c, hw), 2), NAN, dtype=torch.float64, device="cuda")
    part = torch.full((lib.sgmcmc_conv3x3_wrw_scratch_floats(n, c, hw),), NAN, device="cuda")
    E = _hip.ConvBwdEpilogue(s_y=y_bn.data_ptr(), s_out=out.data_ptr(), s_mean=mean.data_ptr(), s_invstd=invstd.data_ptr(),
                             s_partial=partial.data_ptr(), mask_dx=1)
    if add:
        E.e_dout, E.e_out = e_dout.data_ptr(), e_out.data_ptr()
    ridden = [torch.full((numel,), NAN, device="cuda") for _, _, _, numel in riders]
    jobs = (_hip.ReduceJob * max(len(riders), 1))()
    for j, (p, P, taps, numel), o in zip(jobs, riders, ridden):
        j.part, j.out, j.n_slabs, j.numel, j.taps = p.data_ptr(), o.data_ptr(), P, numel, taps
    jp = ctypes.cast(jobs, ctypes.c_void_p) if riders else None
    wp = w if form is None else _prepared(lib, [w])[1][0]
    args = (x.data_ptr(), wp.data_ptr(), dy.data_ptr(), dx.data_ptr(), ctypes.byref(E), dw.data_ptr(), part.data_ptr(),
            n, c, hw, None)
    if form is None:
        _hip.check(lib.sgmcmc_conv3x3_bwd_ride(*args, jp, len(riders), 0, s), "sgmcmc_conv3x3_bwd_ride")
    else:
        _hip.check(lib.sgmcmc_conv3x3_wfrag_bwd(*args, jp, len(riders), 0, form, s), "sgmcmc_conv3x3_wfrag_bwd")
    torch.cuda.synchronize()
    return dx, partial, part, dw, ridden


def _same(a, b):
    for p, q in zip(a[:4], b[:4]):
        assert not torch.isnan(q).any()
        assert torch.equal(p, q)
    for p, q in zip(a[4], b[4]):
        assert not torch.isnan(q).any()
        assert torch.equal(p, q)


@pytest.mark.parametrize("form", FORMS, ids=["lds", "reg"])
@pytest.mark.parametrize("add", [False, True], ids=["SUMS", "ADD+SUMS"])
@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("c,hw", SHAPES)
def test_backward_on_fragments_equals_the_raw_weight_launch(c, hw, n, add, form):
    "dx (stored masked), the BatchNorm-sums partials, the slabs and the reduced dw"
    lib = _hip.lib()
    _same(_backward(lib, c, hw, n, add, form, []), _backward(lib, c, hw, n, add, None, []))


@pytest.mark.parametrize("c,hw", SHAPES)
def test_backward_on_fragments_with_riders_attached(c, hw):
    "the carrier's own results and the ridden reductions, against the raw-weight launch with the same riders"
    lib, s, n = _hip.lib(), _stream(), 5
    riders = []
    for seed, (rc, rhw) in enumerate([(64, 8), (16, 32)]):
        x, w, dy = _data(rc, rhw, n, seed)
        dx = torch.empty_like(x)
        part = torch.full((lib.sgmcmc_conv3x3_wrw_scratch_floats(n, rc, rhw),), NAN, device="cuda")
        P = ctypes.c_int(0)
        _hip.check(lib.sgmcmc_conv3x3_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), 0, part.data_ptr(), n, rc,
                                          rhw, ctypes.byref(P), s), "sgmcmc_conv3x3_bwd")
        riders.append((part, P.value, 9, w.numel()))
    raw = _backward(lib, c, hw, n, True, None, riders)
    for form in FORMS:
        _same(_backward(lib, c, hw, n, True, form, riders), raw)


def test_backward_entry_point_keeps_to_the_steps_variants():
    "no sums epilogue, several minibatches per launch, an unknown form: refused before anything is launched"
    lib, s = _hip.lib(), _stream()
    x, w, dy = _data(16, 32, 2)
    frag = _prepared(lib, [w])[1][0]
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    part = torch.empty(lib.sgmcmc_conv3x3_wrw_scratch_floats(2, 16, 32), device="cuda")
    partial = torch.empty((16, lib.sgmcmc_conv3x3_stat_slices(2, 16, 32), 2), dtype=torch.float64, device="cuda")
    sums = dict(s_y=x.data_ptr(), s_out=x.data_ptr(), s_mean=x.data_ptr(), s_invstd=x.data_ptr(), s_partial=partial.data_ptr())
    for E, form in ((_hip.ConvBwdEpilogue(), 1), (_hip.ConvBwdEpilogue(wrw_mult=2, **sums), 1), (_hip.ConvBwdEpilogue(**sums), 3)):
        assert lib.sgmcmc_conv3x3_wfrag_bwd(x.data_ptr(), frag.data_ptr(), dy.data_ptr(), dx.data_ptr(), ctypes.byref(E),
                                            dw.data_ptr(), part.data_ptr(), 2, 16, 32, None, None, 0, 0, form, s) != 0
    assert lib.sgmcmc_conv3x3_wfrag_fwd(x.data_ptr(), frag.data_ptr(), dx.data_ptr(), 2, 16, 32, partial.data_ptr(), 0, s) != 0


# ---- 3. the carrier -------------------------------------------------------------------------------------------------

def _weights(n_jobs):
    g = torch.Generator().manual_seed(n_jobs)
    return [torch.randn(c, c, 3, 3, generator=g).cuda() for c in ([16, 32, 64] * 8)[:n_jobs]]


@pytest.mark.parametrize("first", [0, 1], ids=["jobs_last", "jobs_first"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n_jobs", [1, 16, 24])
def test_stem_forward_carries_the_fragment_jobs(n_jobs, n, first):
    """the stem's own y and statistics are those of the plain launch; every buffer holds what
    sgmcmc_conv3x3_prepare_weights writes (n = 3: 12 own workgroups, no multiple of 8, beside the jobs' workgroups;
    one 16-channel job: 3 blocks, padded to 8 when they lead the grid)"""
    lib, s = _hip.lib(), _stream()
    g = torch.Generator().manual_seed(n)
    x, w = torch.randn(n, 3, 32, 32, generator=g).cuda(), torch.randn(16, 3, 3, 3, generator=g).cuda()
    ws = _weights(n_jobs)
    want_fwd, want_dgrad = _prepared(lib, ws)
    y0, y1 = torch.full((n, 16, 32, 32), NAN, device="cuda"), torch.full((n, 16, 32, 32), NAN, device="cuda")
    st0, st1 = (torch.full((16, 4 * n, 2), NAN, dtype=torch.float64, device="cuda") for _ in range(2))
    _hip.check(lib.sgmcmc_conv_stem_fwd(x.data_ptr(), w.data_ptr(), y0.data_ptr(), st0.data_ptr(), n, s), "stem")
    jobs, fwd, dgrad = _frag_jobs(ws)
    _hip.check(lib.sgmcmc_conv_stem_fwd_frags(x.data_ptr(), w.data_ptr(), y1.data_ptr(), st1.data_ptr(), n,
                                              ctypes.cast(jobs, ctypes.c_void_p), n_jobs, first, s),
               "sgmcmc_conv_stem_fwd_frags")
    torch.cuda.synchronize()
    assert not torch.isnan(y0).any() and not torch.isnan(st0).any()
    assert torch.equal(y1, y0) and torch.equal(st1, st0)
    for got, want in zip(fwd + dgrad, want_fwd + want_dgrad):
        assert not torch.isnan(want).any()
        assert torch.equal(got, want)
    # ... without statistics, and with the forward buffers alone
    y2 = torch.full_like(y0, NAN)
    jobs, fwd, dgrad = _frag_jobs(ws)
    for j in jobs:
        j.dgrad = 0
    _hip.check(lib.sgmcmc_conv_stem_fwd_frags(x.data_ptr(), w.data_ptr(), y2.data_ptr(), 0, n,
                                              ctypes.cast(jobs, ctypes.c_void_p), n_jobs, first, s),
               "sgmcmc_conv_stem_fwd_frags")
    torch.cuda.synchronize()
    assert torch.equal(y2, y0)
    assert all(torch.equal(a, b) for a, b in zip(fwd, want_fwd)) and all(torch.isnan(d).all() for d in dgrad)


def test_carried_fragments_follow_the_layout_formula():
    "one job of each channel count against the permutation computed on the host"
    lib, s = _hip.lib(), _stream()
    x, w = torch.randn(2, 3, 32, 32).cuda(), torch.randn(16, 3, 3, 3).cuda()
    y = torch.empty(2, 16, 32, 32, device="cuda")
    ws = _weights(3)
    jobs, fwd, dgrad = _frag_jobs(ws)
    _hip.check(lib.sgmcmc_conv_stem_fwd_frags(x.data_ptr(), w.data_ptr(), y.data_ptr(), 0, 2,
                                              ctypes.cast(jobs, ctypes.c_void_p), 3, 0, s), "sgmcmc_conv_stem_fwd_frags")
    torch.cuda.synchronize()
    assert sorted(wt.shape[0] for wt in ws) == [16, 32, 64]
    for wt, f, d in zip(ws, fwd, dgrad):
        hf, hd = _host_fragments(wt)
        assert np.array_equal(f.cpu().numpy(), hf) and np.array_equal(d.cpu().numpy(), hd)


def test_carrier_refuses_more_jobs_than_a_launch_carries():
    lib, s = _hip.lib(), _stream()
    x, w = torch.randn(1, 3, 32, 32).cuda(), torch.randn(16, 3, 3, 3).cuda()
    y = torch.empty(1, 16, 32, 32, device="cuda")
    jobs, _, _ = _frag_jobs([torch.randn(16, 16, 3, 3).cuda()] * (_hip.FRAG_JOBS + 1))
    assert lib.sgmcmc_conv_stem_fwd_frags(x.data_ptr(), w.data_ptr(), y.data_ptr(), 0, 1, ctypes.cast(jobs, ctypes.c_void_p),
                                          _hip.FRAG_JOBS + 1, 0, s) != 0
    jobs[0].channels = 48
    assert lib.sgmcmc_conv_stem_fwd_frags(x.data_ptr(), w.data_ptr(), y.data_ptr(), 0, 1, ctypes.cast(jobs, ctypes.c_void_p),
                                          1, 0, s) != 0


# ---- 4. staleness and fallbacks -------------------------------------------------------------------------------------

def _net(batch):
    from bnn_priors_amd import models
    torch.manual_seed(1)
    x = torch.randn(batch, 3, 32, 32).cuda()
    y = (torch.arange(batch) % 10).cuda()
    net = models.get_model(x.cpu()[:2], torch.tensor([0, 9]), "googleresnet", width=50, depth=3, weight_prior="gaussian",
                           weight_scale=2 ** .5, bias_prior="gaussian", bias_scale=1.).cuda()
    models.he_initialize(net)
    net.train()
    return net, x, y


def _evaluate(net, x, y):
    for p in net.parameters():
        p.grad = None
    with conv.deferring(net):
        torch.nn.functional.cross_entropy(net.net(x), y).backward()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in net.parameters()] + [b.clone() for b in net.buffers()]


def _counting(monkeypatch):
    "launches of the preparation kernel (weights each), jobs the stem carried"
    seen = {"prepared": [], "carried": 0}
    prepare, take = conv._prepare, conv.take_frag_jobs

    def _prepare(weights):
        seen["prepared"].append(len(weights))
        prepare(weights)

    def take_frag_jobs(device):
        taken = take(device)
        seen["carried"] += len(taken)
        return taken

    monkeypatch.setattr(conv, "_prepare", _prepare)
    monkeypatch.setattr(conv, "take_frag_jobs", take_frag_jobs)
    return seen


def _perturb(net, k):
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.mul_(1.0 + 0.01 * ((i + k) % 5)).add_(0.001 * k)      # in place: the sampler's update keeps the tensors


def test_two_scopes_with_an_update_between_them_never_read_stale_fragments(monkeypatch):
    """googleresnet, batch 5.  Scope 1: every trunk weight is first seen mid-scope (a launch of its own each).  Scope 2,
    after an in-place update of every parameter: the 16 jobs ride in the stem's launch, nothing else prepares.  Both
    equal the raw-weight route on the same weights, gradients and BatchNorm buffers alike."""
    net, x, y = _net(5)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    want = {}
    monkeypatch.setattr(conv, "WEIGHT_FRAGS", {})
    for k in (1, 2):
        _perturb(net, k)
        want[k] = _evaluate(net, x, y)
    net.load_state_dict(state)
    monkeypatch.setattr(conv, "WEIGHT_FRAGS", FULL)
    seen = _counting(monkeypatch)
    for k in (1, 2):
        _perturb(net, k)
        got = _evaluate(net, x, y)
        assert all(torch.equal(a, b) for a, b in zip(got, want[k])), k
        if k == 1:
            assert seen == {"prepared": [1] * 16, "carried": 0}, seen
            seen.update(prepared=[], carried=0)
        else:
            assert seen == {"prepared": [], "carried": 16}, seen
    assert not conv._frag_queue and not conv._frag_valid


def test_a_scope_that_opens_with_a_trunk_convolution_flushes_the_queue(monkeypatch):
    """no stem, so no carrier: the first use of a queued weight prepares everything still queued in ONE launch; a weight
    the owner did not use before gets a launch of its own; the third scope queues all three"""
    monkeypatch.setattr(conv, "WEIGHT_FRAGS", FULL)
    owner = types.SimpleNamespace()
    x, w1, _ = _data(32, 16, 3, 1)
    w2, w3 = _data(32, 16, 3, 2)[1], _data(32, 16, 3, 3)[1]
    seen = _counting(monkeypatch)

    def scope(ws):
        with conv.deferring(owner):
            outs = [conv.conv3x3(x, w, True) for w in ws]
        torch.cuda.synchronize()
        return outs

    def raw(w):
        assert not conv._defer["active"]
        return conv._run(x, w, False, True)      # outside a scope: the raw-weight kernel

    for ws, prepared in (([w1, w2], [1, 1]), ([w1, w2, w3], [2, 1]), ([w3, w1, w2], [3])):
        with torch.no_grad():
            for w in (w1, w2, w3):
                w.mul_(1.25)
        seen.update(prepared=[], carried=0)
        for (y, st), w in zip(scope(ws), ws):
            y0, st0 = raw(w)
            assert torch.equal(y, y0) and torch.equal(st, st0)
        assert seen == {"prepared": prepared, "carried": 0}, seen


# ---- 5. the step ----------------------------------------------------------------------------------------------------

def _three_steps(table, monkeypatch):
    from bnn_priors_amd import graphed, mcmc, models, potential
    monkeypatch.setattr(conv, "WEIGHT_FRAGS", table)
    torch.manual_seed(0)
    x0, y0 = torch.rand(16, 3, 32, 32), torch.arange(16) % 10
    net = models.get_model(x0, y0, "googleresnet", weight_prior="gaussian", weight_loc=0., weight_scale=2 ** .5,
                           bias_prior="gaussian", bias_scale=1.).cuda()
    torch.manual_seed(1)
    models.he_initialize(net)
    opt = mcmc.VerletSGLD(net.parameters(), lr=1e-4, num_data=50000.0, momentum=0.98, temperature=1.0, seed=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pot = potential.Potential(net, opt, 50000.0)
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(8, 3, 32, 32, generator=g).cuda(), (torch.arange(8) % 10).cuda()
    opt.sample_momentum()
    pot.minibatch(x, y, False)
    opt.initial_step(save_state=False, calc_metrics=False)
    step = graphed.GraphedLeapfrog(pot, opt, x, y)
    for _ in range(3):
        step.replay(x, y)
    torch.cuda.synchronize()
    eng = opt.engine
    out = {"m": eng.m.clone(), "v": eng.v.clone()}
    out.update({"p." + k: v.detach().clone() for k, v in net.named_parameters()})
    out.update({"g." + k: v.grad.clone() for k, v in net.named_parameters()})
    out.update({"b." + k: v.clone() for k, v in net.named_buffers()})
    return out


def test_three_captured_steps_of_googleresnet_are_bit_identical(monkeypatch):
    "GraphedLeapfrog at batch 8: parameters, momentum, RMSprop statistic, gradients and BatchNorm buffers"
    raw = _three_steps({}, monkeypatch)
    frag = _three_steps(FULL, monkeypatch)
    assert sorted(raw) == sorted(frag) and len(raw) > 100
    for k in raw:
        assert not torch.isnan(raw[k].float()).any(), k
        assert torch.equal(frag[k], raw[k]), k
