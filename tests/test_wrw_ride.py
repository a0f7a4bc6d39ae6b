"""Weight-gradient slab reductions that ride in the next backward launch (csrc/conv_hip.inc ``RideJobs``,
``sgmcmc_conv3x3_bwd_ride``; conv.take_riders): the rider workgroups run ``reduce_block`` -- the blocks of
``sgmcmc_wrw_reduce_many`` -- so every weight gradient keeps its bits whatever the route, and the carrier's own
results do not notice its riders."""
import ctypes

import pytest
import torch

from bnn_priors_amd import _hip, conv

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _data(c, hw, n, seed):
    g = torch.Generator().manual_seed(1000 * c + n + seed)
    x = torch.randn(n, c, hw, hw, generator=g)
    w = torch.randn(c, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** .5
    dy = torch.randn(n, c, hw, hw, generator=g)
    return x.cuda(), w.cuda(), dy.cuda()


def _jobs(entries):
    jobs = (_hip.ReduceJob * len(entries))()
    for j, (part, out, slabs, taps) in zip(jobs, entries):
        j.part, j.out, j.n_slabs, j.numel, j.taps = part.data_ptr(), out.data_ptr(), slabs, out.numel(), taps
    return jobs


def _trunk_job(lib, c, hw, n, s, seed):
    "slabs of a (c, hw) trunk convolution's weight gradient + that gradient by the immediate route -> (part, P, 9, dw)"
    x, w, dy = _data(c, hw, n, seed)
    dx = torch.empty_like(x)
    part = torch.empty(lib.sgmcmc_conv3x3_wrw_scratch_floats(n, c, hw), device="cuda")
    P = ctypes.c_int(0)
    _hip.check(lib.sgmcmc_conv3x3_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), 0, part.data_ptr(), n, c, hw,
                                      ctypes.byref(P), s), "sgmcmc_conv3x3_bwd")
    dw = torch.full_like(w, NAN)
    part2 = torch.empty_like(part)
    _hip.check(lib.sgmcmc_conv3x3_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), part2.data_ptr(),
                                      n, c, hw, None, s), "sgmcmc_conv3x3_bwd")
    return part, P.value, 9, dw


def _stem_job(lib, n, s):
    "the stem's slabs (16 x 27 numbers each, two (image, band) items per slab) -> (part, P, 1, dw)"
    g = torch.Generator().manual_seed(n)
    x, dy = torch.randn(n, 3, 32, 32, generator=g).cuda(), torch.randn(n, 16, 32, 32, generator=g).cuda()
    part = torch.empty(lib.sgmcmc_conv_stem_scratch_floats(n), device="cuda")
    P = ctypes.c_int(0)
    _hip.check(lib.sgmcmc_conv_stem_wrw(x.data_ptr(), dy.data_ptr(), 0, part.data_ptr(), n, ctypes.byref(P), s),
               "sgmcmc_conv_stem_wrw")
    dw, part2 = torch.full((16, 3, 3, 3), NAN, device="cuda"), torch.empty_like(part)
    _hip.check(lib.sgmcmc_conv_stem_wrw(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), part2.data_ptr(), n, None, s),
               "sgmcmc_conv_stem_wrw")
    return part, P.value, 1, dw


def _carrier(lib, c, hw, n, s, riders, first):
    """the (c, hw) merged backward launch with the BatchNorm-sums epilogue, its own slabs deferred, carrying ``riders`` (None:
    sgmcmc_conv3x3_bwd_ex) -> dx, sums partials, slabs, [ridden dw]"""
    x, w, dy = _data(c, hw, n, 77)
    g = torch.Generator().manual_seed(7 + n)
    out = torch.randn(x.shape, generator=g).relu().cuda()
    y_bn, mean, invstd = (torch.randn(x.shape, generator=g).cuda(), torch.randn(c, generator=g).cuda() * .1,
                          torch.rand(c, generator=g).cuda() + .5)
    dx = torch.full_like(x, NAN)
    partial = torch.full((c, lib.sgmcmc_conv3x3_stat_slices(n, c, hw), 2), NAN, dtype=torch.float64, device="cuda")
    part = torch.full((lib.sgmcmc_conv3x3_wrw_scratch_floats(n, c, hw),), NAN, device="cuda")
    E = _hip.ConvBwdEpilogue(s_y=y_bn.data_ptr(), s_out=out.data_ptr(), s_mean=mean.data_ptr(), s_invstd=invstd.data_ptr(),
                             s_partial=partial.data_ptr(), mask_dx=1)
    P = ctypes.c_int(0)
    args = (x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), ctypes.byref(E), 0, part.data_ptr(), n, c, hw,
            ctypes.byref(P))
    outs = []
    if riders is None:
        _hip.check(lib.sgmcmc_conv3x3_bwd_ex(*args, s), "sgmcmc_conv3x3_bwd_ex")
    else:
        outs = [torch.full_like(dw, NAN) for _, _, _, dw in riders]
        jobs = _jobs([(p, o, slabs, taps) for (p, slabs, taps, _), o in zip(riders, outs)])
        _hip.check(lib.sgmcmc_conv3x3_bwd_ride(*args, ctypes.cast(jobs, ctypes.c_void_p), len(riders), int(first), s),
                   "sgmcmc_conv3x3_bwd_ride")
    torch.cuda.synchronize()
    assert P.value * w.numel() == part.numel()
    return dx, partial, part, outs


def _check(lib, c, hw, n, s, riders, first):
    many = [torch.full_like(dw, NAN) for _, _, _, dw in riders]
    jobs = _jobs([(p, o, slabs, taps) for (p, slabs, taps, _), o in zip(riders, many)])
    _hip.check(lib.sgmcmc_wrw_reduce_many(ctypes.cast(jobs, ctypes.c_void_p), len(riders), s), "sgmcmc_wrw_reduce_many")
    dx0, sums0, slabs0, _ = _carrier(lib, c, hw, n, s, None, first)
    dx1, sums1, slabs1, ridden = _carrier(lib, c, hw, n, s, riders, first)
    for r, m, (_, _, _, immediate) in zip(ridden, many, riders):
        assert not torch.isnan(r).any()
        assert torch.equal(r, m) and torch.equal(r, immediate)
    assert not torch.isnan(dx0).any() and not torch.isnan(sums0).any() and not torch.isnan(slabs0).any()
    assert torch.equal(dx0, dx1) and torch.equal(sums0, sums1) and torch.equal(slabs0, slabs1)


# carrier shape, the shapes whose slabs ride in it
CASES = [((16, 32), [(16, 32)]), ((32, 16), [(64, 8)]), ((64, 8), [(64, 8), (16, 32)])]


@pytest.mark.parametrize("first", [False, True], ids=["riders_last", "riders_first"])
@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("carrier,riding", CASES, ids=["16<-16", "32<-64", "64<-64+16"])
def test_ridden_reductions_carry_the_bits_of_the_other_routes(carrier, riding, n, first):
    """slab counts at n = 5: 10 (16 channels), 5 (32), 2 (64) -- the remainder loops of the 4-at-a-time order; n = 16 at 16
    channels: 32 slabs, 8 per thread -- the 8-deep loop.  The ridden gradient equals sgmcmc_wrw_reduce_many's on the same
    slabs and the immediate route's; the carrier's data gradient, BatchNorm sums and slabs are those of a launch without
    riders.  Outputs start as NaN, so an element nobody wrote shows."""
    lib, s = _hip.lib(), torch.cuda.current_stream().cuda_stream
    riders = [_trunk_job(lib, c, hw, n, s, seed) for seed, (c, hw) in enumerate(riding)]
    _check(lib, *carrier, n, s, riders, first)


@pytest.mark.parametrize("first", [False, True], ids=["riders_last", "riders_first"])
def test_a_wide_job_rides(first):
    """many slabs of a small gradient (P >= 256, E <= 4096: reduce_block's 16 x 16 path): the stem's 432 numbers at 128
    images = 256 slabs, beside a trunk job, in a 16-channel carrier of 16 images"""
    lib, s = _hip.lib(), torch.cuda.current_stream().cuda_stream
    stem = _stem_job(lib, 128, s)
    assert stem[1] >= 256 and stem[3].numel() <= 4096
    _check(lib, 16, 32, 16, s, [stem, _trunk_job(lib, 32, 16, 16, s, 3)], first)


def test_entry_point_refuses_more_jobs_than_a_launch_carries():
    lib, s = _hip.lib(), torch.cuda.current_stream().cuda_stream
    job = _trunk_job(lib, 16, 32, 1, s, 0)
    with pytest.raises(RuntimeError, match="sgmcmc_conv3x3_bwd_ride"):      # refused before anything is launched
        _carrier(lib, 16, 32, 1, s, [job] * (_hip.RIDE_JOBS + 1), False)


# ---- step level: googleresnet ---------------------------------------------------------------------------------------

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
    assert not conv._pending


def _counting(monkeypatch):
    "how many jobs rode, how many the end-of-pass reduction summed -- with every trunk shape a carrier"
    monkeypatch.setattr(conv, "RIDE_CARRIERS", set(conv.SHAPES))
    seen = {"rode": 0, "flushed": 0}
    take, flush = conv.take_riders, conv._flush_pending

    def take_riders(c, hw):
        taken = take(c, hw)
        seen["rode"] += len(taken or ())
        return taken

    def _flush_pending():
        seen["flushed"] += len(conv._pending)
        flush()

    monkeypatch.setattr(conv, "take_riders", take_riders)
    monkeypatch.setattr(conv, "_flush_pending", _flush_pending)
    return seen


@pytest.mark.parametrize("batch", [5, 16])
def test_every_gradient_of_googleresnet_keeps_its_bits(batch, monkeypatch):
    "one gradient evaluation with the riders and with the single reduction at the end of the pass"
    net, x, y = _net(batch)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    seen = _counting(monkeypatch)
    grads, jobs = {}, None
    for ride in (False, True):
        monkeypatch.setattr(conv, "WRW_RIDE", ride)
        net.load_state_dict(state)
        seen.update(rode=0, flushed=0)
        _evaluate(net, x, y)
        torch.cuda.synchronize()
        grads[ride] = [p.grad.clone() for p in net.parameters()]
        if not ride:
            # the 21 convolution weights (16 trunk, 2 x (strided 3x3 + 1x1 shortcut), the stem) and the head's two
            jobs = seen["flushed"]
            assert jobs >= 21 and seen["rode"] == 0, seen
        else:    # the last trunk convolution's and the stem's find no carrier behind them
            assert (seen["rode"], seen["flushed"]) == (jobs - 2, 2), seen
    assert all(not torch.isnan(g).any() for g in grads[True])
    for a, b in zip(grads[True], grads[False]):
        assert torch.equal(a, b)


def test_the_captured_pass_equals_the_eager_one(monkeypatch):
    "batch 16: the riders inside a captured graph (their job tables are kernel arguments) against the eager pass"
    from bnn_priors_amd import _capture
    net, x, y = _net(16)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    assert conv.WRW_RIDE
    seen = _counting(monkeypatch)
    _evaluate(net, x, y)
    torch.cuda.synchronize()
    eager = [p.grad.clone() for p in net.parameters()]
    rode = seen["rode"]
    assert rode >= 19 and seen["flushed"] == 2, seen
    net.load_state_dict(state)
    seen.update(rode=0, flushed=0)
    graph = torch.cuda.CUDAGraph()
    with _capture.capture(graph):
        _evaluate(net, x, y)
    assert (seen["rode"], seen["flushed"]) == (rode, 2), seen
    static = [p.grad for p in net.parameters()]
    for rep in range(2):
        net.load_state_dict(state)
        for g in static:
            g.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)
