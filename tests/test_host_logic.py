"""Host-side logic of round 4 that needs no GPU: the exact pass's group-size choice, the batch source's lazy minibatches
(same rows, same RNG consumption as its ordinary iteration), in-place filling of a consumer's buffers."""
import torch

from bnn_priors_amd import graphed
from bnn_priors_amd.inference import LazyBatch, _BatchSource


def test_group_size_leaves_the_fewest_leftovers_and_deals_groups_evenly():
    assert graphed.pick_group(390, 128, 3, "auto") == 5            # 78 groups = 26 per lane, nothing left over
    assert graphed.pick_group(468, 128, 3, "auto") == 4            # 117 groups = 39 per lane
    assert graphed.pick_group(50, 128, 3, "auto") == 5             # 10 groups, nothing left over
    assert graphed.pick_group(4, 32, 3, "auto") == 4               # one group
    assert graphed.pick_group(390, 256, 3, "auto") == 4            # 1,024 rows per launch at most (the fused head)
    assert graphed.pick_group(390, 128, 3, 16) == 8 and graphed.pick_group(390, 128, 3, 1) == 1
    assert graphed.pick_group(None, 128, 3, "auto") == 1             # unknown pass length: never grouped


def _source(shuffle, n=300):
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(n, 7, generator=g), torch.randint(0, 10, (n,), generator=g)
    ds = torch.utils.data.TensorDataset(x, y)
    return _BatchSource(torch.utils.data.DataLoader(ds, batch_size=128, shuffle=shuffle), torch.device("cpu")), x, y


def test_lazy_batches_are_the_ordinary_minibatches_and_consume_the_same_random_numbers():
    for shuffle in (True, False):
        torch.manual_seed(5)
        src, x, y = _source(shuffle)
        plain = [(a.clone(), b.clone()) for a, b in src]
        after = torch.get_rng_state()
        torch.manual_seed(5)
        src, _, _ = _source(shuffle)
        lazies = list(src.lazy_batches())
        assert torch.equal(torch.get_rng_state(), after)
        assert [len(b) for b, _ in lazies] == [128, 128, 44]
        for (lb, none), (px, py) in zip(lazies, plain):
            assert isinstance(lb, LazyBatch) and none is None and lb.shapes == (tuple(px.shape), tuple(py.shape))
            mx, my = lb.materialize()
            assert torch.equal(mx, px) and torch.equal(my, py)
        assert src.n_full_batches() == 2 and src.example()[0].shape == (128, 7)


def test_filling_writes_minibatches_into_the_consumers_buffers():
    torch.manual_seed(9)
    src, x, y = _source(True)
    plain = [(a.clone(), b.clone()) for a, b in src]
    torch.manual_seed(9)
    src, _, _ = _source(True)
    bx, by = torch.zeros(128, 7), torch.zeros(128, dtype=torch.int64)
    with src.filling(lambda rows: (bx, by) if rows == 128 else None):
        got = []
        for gx, gy in src:
            if len(gx) == 128:
                assert gx.data_ptr() == bx.data_ptr() and gy.data_ptr() == by.data_ptr()      # produced in place
            got.append((gx.clone(), gy.clone()))
    assert src._provider is None
    for (gx, gy), (px, py) in zip(got, plain):
        assert torch.equal(gx, px) and torch.equal(gy, py)


def test_a_group_provider_changes_nothing_where_a_group_cannot_be_gathered_at_once():
    """``filling(provider, group=(G, group_provider))``: on a source that cannot gather on the device (the CPU here) the
    group provider is asked, declined by ``_stage_into``, and every minibatch takes the ordinary route -- same rows."""
    torch.manual_seed(9)
    src, x, y = _source(True, n=700)
    plain = [(a.clone(), b.clone()) for a, b in src]
    torch.manual_seed(9)
    src, _, _ = _source(True, n=700)
    gx, gy = torch.zeros(256, 7), torch.zeros(256, dtype=torch.int64)
    asked = []
    with src.filling(lambda rows: None, group=(2, lambda rows: (asked.append(rows), (gx, gy))[1])):
        got = [(a.clone(), b.clone()) for a, b in src]
    assert src._provider is None and src._group is None
    assert asked and all(r == 256 for r in asked)
    assert len(got) == len(plain) == 6
    for (a, b), (px, py) in zip(got, plain):
        assert torch.equal(a, px) and torch.equal(b, py)


def test_gradient_tags_carry_the_masked_flag_and_die_with_the_tensor_version():
    "bnlink: (partial, n, masked) while the gradient tensor is untouched; an in-place change or a disabled link: None"
    from bnn_priors_amd import bnlink
    t = torch.zeros(4)
    part = torch.zeros(2, 3, 2, dtype=torch.float64)
    assert bnlink.sums_of(t) is None
    bnlink.tag_gradient(t, part, 3, masked=True)
    got = bnlink.sums_of(t)
    assert got[0] is part and got[1] == 3 and got[2] is True
    bnlink.tag_gradient(t, part, 3)
    assert bnlink.sums_of(t)[2] is False
    t.add_(1.0)
    assert bnlink.sums_of(t) is None
    out = torch.ones(2, 3)
    bnlink.tag_output(out, torch.zeros(2, 3), torch.zeros(2, 3))
    assert bnlink.source_of(out)[0] is not None and bnlink.source_of(torch.ones(2, 3)) == (None, None)


# ---- the slab hand-over of conv.py (slabs_for / reduce_or_defer), driven on CPU tensors by a toy operator ------------
class _Toy(torch.autograd.Function):
    "y = sum(x * w) [+ sum(bias)]; backward leaves one slab per row of x and hands them over like a conv operator"
    @staticmethod
    def forward(ctx, x, w, bias, log):
        from bnn_priors_amd import conv
        conv._note_use(*((w,) if bias is None else (w, bias)))
        ctx.save_for_backward(x, w, bias)
        ctx.log = log
        return (x * w).sum() if bias is None else (x * w).sum() + bias.sum()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from bnn_priors_amd import conv
        x, w, bias = ctx.saved_tensors
        log = ctx.log
        part, out = dy * x, torch.empty_like(w)
        if bias is None:
            got = conv.reduce_or_defer(part, out, x.shape[0], 1, w)
            # (``got`` itself is not kept: AccumulateGrad adopts only a gradient that nobody else references)
            log.append(dict(part=part, out=out, same=got is out, aliased=got.data_ptr() == out.data_ptr()))
            if log[0].get("boom"):
                raise RuntimeError("boom")
            return None, got, None, None
        S = conv.slabs_for(w, bias)
        assert (S.ref is not None) == S.defer
        S.count.value = x.shape[0]                  # (what a launch leaves through S.ref)
        bpart, bout = (dy * torch.ones_like(x))[:, :bias.numel()].contiguous(), torch.empty_like(bias)
        if not S.defer:                             # (... and a launch given NULL reduces by itself)
            out.copy_(part.sum(0)), bout.copy_(bpart.sum(0))
        got, bgot = S.hand(part, out, 1), S.hand(bpart, bout, 1)
        log.append(dict(defer=S.defer, out=out, bout=bout, same=got is out and bgot is bout))
        return None, got, bgot, None


def _handover_stubs(monkeypatch):
    "conv._flush_pending and conv._reduce_now replaced AFTER import by stubs that sum the slabs in torch"
    from bnn_priors_amd import conv
    seen = dict(flushed=[], now=[])

    def reduce_now(entries):
        seen["now"].append(list(entries))
        for part, out, n, taps in entries:
            out.copy_(part[:n].sum(0))

    def flush():
        seen["flushed"].append(list(conv._pending))
        for part, out, n, taps in conv._pending:
            out.copy_(part[:n].sum(0))
        conv._pending.clear()

    monkeypatch.setattr(conv, "_reduce_now", reduce_now)
    monkeypatch.setattr(conv, "_flush_pending", flush)
    return conv, seen


def test_handover_defers_inside_the_scope_and_autograd_adopts_an_alias(monkeypatch):
    conv, seen = _handover_stubs(monkeypatch)
    x, w, log = torch.arange(12.).view(3, 4), torch.ones(4, requires_grad=True), []
    with conv.deferring():
        _Toy.apply(x, w, None, log).backward()
        # the replaced _flush_pending ran as autograd's final callback: the attribute is looked up at call time
        assert len(seen["flushed"]) == 1 and not conv._pending
    (job,), rec = seen["flushed"][0], log[0]
    assert job[0] is rec["part"] and job[1] is rec["out"] and job[2:] == (3, 1)
    assert not rec["same"] and rec["aliased"]
    assert w.grad.data_ptr() == rec["out"].data_ptr() and torch.equal(w.grad, x.sum(0))
    assert not seen["now"] and not conv._pending and not conv._defer["active"]
    assert seen["flushed"][1:] == [[]]            # (the scope's own call at its end found nothing left)


def test_handover_reduces_at_once_where_autograd_would_not_adopt(monkeypatch):
    conv, seen = _handover_stubs(monkeypatch)
    x = torch.arange(12.).view(3, 4)

    def immediate(rec):
        job, = seen["now"][len(log) - 1]
        assert rec["same"] and job[1] is rec["out"] and job[2:] == (3, 1) and not conv._pending
    w, log = torch.ones(4, requires_grad=True), []
    _Toy.apply(x, w, None, log).backward()                       # outside the scope
    immediate(log[0])
    assert torch.equal(w.grad, x.sum(0))
    with conv.deferring():                                       # a .grad exists already
        _Toy.apply(x, w, None, log).backward()
    immediate(log[1])
    assert torch.equal(w.grad, 2 * x.sum(0))
    w, log = torch.ones(4, requires_grad=True), []
    with conv.deferring():                                       # the weight is used twice in the scope
        (_Toy.apply(x, w, None, log) + _Toy.apply(x, w, None, log)).backward()
    assert all(r["same"] for r in log) and {id(e[0][1]) for e in seen["now"][2:]} == {id(r["out"]) for r in log}
    assert torch.equal(w.grad, 2 * x.sum(0))
    assert len(seen["now"]) == 4 and all(f == [] for f in seen["flushed"])


def test_handover_for_several_parameters_defers_only_if_all_qualify(monkeypatch):
    conv, seen = _handover_stubs(monkeypatch)
    x = torch.arange(12.).view(3, 4)
    w, bias, log = torch.ones(4, requires_grad=True), torch.zeros(2, requires_grad=True), []
    with conv.deferring():
        _Toy.apply(x, w, bias, log).backward()
    assert log[0]["defer"] and not log[0]["same"]
    assert [j[1:] for j in seen["flushed"][0]] == [(log[0]["out"], 3, 1), (log[0]["bout"], 3, 1)]
    assert w.grad.data_ptr() == log[0]["out"].data_ptr() and bias.grad.data_ptr() == log[0]["bout"].data_ptr()
    assert torch.equal(w.grad, x.sum(0)) and torch.equal(bias.grad, torch.full((2,), 3.))
    w, bias, log = torch.ones(4, requires_grad=True), torch.zeros(2, requires_grad=True), []
    with conv.deferring():
        conv._note_use(bias)                                     # (a second use of the bias alone: a prior, say)
        _Toy.apply(x, w, bias, log).backward()
    assert not log[0]["defer"] and log[0]["same"]
    assert all(f == [] for f in seen["flushed"][1:]) and torch.equal(w.grad, x.sum(0))
    # ``when=False`` never defers, and nothing is queued outside a backward pass
    with conv.deferring():
        assert not conv.slabs_for(w, when=False).defer


def test_an_exception_inside_the_scope_leaves_no_pending_slabs(monkeypatch):
    import pytest
    conv, seen = _handover_stubs(monkeypatch)
    x, w, log = torch.arange(12.).view(3, 4), torch.ones(4, requires_grad=True), [dict(boom=True)]
    with pytest.raises(RuntimeError, match="boom"):
        with conv.deferring():
            _Toy.apply(x, w, None, log).backward()
    assert not log[1]["same"]                                     # it had deferred ...
    assert not conv._pending and not conv._defer["active"] and not seen["flushed"]
