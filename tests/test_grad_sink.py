"""The gradient-sink predicate (ops/grad_sink.py), on CPU: when may a
backward kernel add a weight gradient into ``param.grad`` in place."""

import torch

from mpi4dl_amd.comm import FlatGrads
from mpi4dl_amd.ops.grad_sink import grad_sink, opt_in, opt_out


def _param(shape=(4, 3), grad=True, opted=True):
    p = torch.nn.Parameter(torch.randn(shape))
    if grad:
        p.grad = torch.zeros(shape)
    if opted:
        opt_in(p)
    return p


def _sink(p):
    with torch.no_grad():  # a plain backward runs with grad mode off
        return grad_sink(p)


def test_opted_in_parameter_gives_its_grad():
    p = _param()
    assert _sink(p) is p.grad


def test_flatgrads_opts_its_parameters_in():
    m = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))
    fg = FlatGrads(m)
    for p in m.parameters():
        s = _sink(p)
        assert s is p.grad
        assert s.untyped_storage().data_ptr() == \
            fg.buffer.untyped_storage().data_ptr()


def test_no_grad_tensor():
    assert _sink(_param(grad=False)) is None


def test_wrong_dtype():
    p64 =torch.nn.Parameter(torch.randn(4, 3, dtype=torch.float64))
    p64.grad = torch.zeros(4, 3, dtype=torch.float64)
    opt_in(p64)
    assert _sink(p64) is None
    h = torch.nn.Parameter(torch.randn(4, 3, dtype=torch.bfloat16))
    h.grad = torch.zeros(4, 3, dtype=torch.bfloat16)
    opt_in(h)
    assert _sink(h) is None


def test_wrong_shape_or_layout():
    p = _param()
    # .grad's setter refuses another shape, so stand in for the parameter
    class Holder:
        pass

    q = Holder()
    q.__dict__.update(_mpi4dl_grad_sink=True, grad=torch.zeros(3, 4),
                      device=p.device, shape=p.shape, requires_grad=True,
                      _backward_hooks=None, _post_accumulate_grad_hooks=None)
    assert _sink(q) is None
    # same shape, not contiguous
    t = torch.nn.Parameter(torch.randn(4, 3))
    t.grad = torch.zeros(3, 4).t()
    assert not t.grad.is_contiguous()
    opt_in(t)
    assert _sink(t) is None


def test_not_opted_in():
    p = _param(opted=False)
    assert _sink(p) is None
    opt_in(p)
    assert _sink(p) is p.grad
    opt_out(p)
    assert _sink(p) is None


def test_tensor_hook():
    p = _param()
    h = p.register_hook(lambda g: g)
    assert _sink(p) is None
    h.remove()
    assert _sink(p) is p.grad


def test_post_accumulate_hook():
    p = _param()
    h = p.register_post_accumulate_grad_hook(lambda q: None)
    assert _sink(p) is None
    h.remove()
    assert _sink(p) is p.grad


def test_grad_mode_on():
    p = _param()
    with torch.enable_grad():
        assert grad_sink(p) is None


def test_switch_off(monkeypatch):
    p = _param()
    monkeypatch.setenv("MPI4DL_GRAD_SINK", "0")
    assert _sink(p) is None
    monkeypatch.setenv("MPI4DL_GRAD_SINK", "1")
    assert _sink(p) is p.grad


class _Probe(torch.autograd.Function):
    """Asks grad_sink(w) from inside a backward pass."""

    seen = []

    @staticmethod
    def forward(ctx, x, w):
        ctx.w = w
        return x * w.sum()

    @staticmethod
    def backward(ctx, g):
        _Probe.seen.append(grad_sink(ctx.w))
        return g * ctx.w.sum().detach(), g.sum() * torch.ones_like(ctx.w)


def test_only_a_pass_that_accumulates_into_grad_gets_the_sink():
    """torch.autograd.grad and backward(inputs=...) without the parameter
    must leave p.grad alone: no sink there; a plain backward gets it."""
    p = _param()
    x = torch.randn(4, 3, requires_grad=True)
    _Probe.seen = []
    _Probe.apply(x, p).sum().backward()
    torch.autograd.grad(_Probe.apply(x, p).sum(), x)
    torch.autograd.grad(_Probe.apply(x, p).sum(), [x, p])
    _Probe.apply(x, p).sum().backward(inputs=[x])
    _Probe.apply(x, p).sum().backward(inputs=[x, p])
    assert _Probe.seen[0] is p.grad
    assert _Probe.seen[1] is None
    assert _Probe.seen[2] is None
    assert _Probe.seen[3] is None
    assert _Probe.seen[4] is p.grad
