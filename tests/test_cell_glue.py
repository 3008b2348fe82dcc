"""CPU tests of the cell glue (ops/fuse.py): state_fan against the unfused
composition under autograd, the shared-ReLU table, and whole cells with
MPI4DL_CELL_GLUE on against off. Everything is compared with
torch.equal: the fused gradient is the unfused one bit for bit, which
holds only when the fold takes autograd's order."""

import gc

import pytest
import torch

from mpi4dl_amd.ops import fuse
from mpi4dl_amd.ops.fuse import add_cat, shared_relu, state_fan

SHAPE = (2, 6, 5, 7)


def _state(dtype, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(SHAPE, generator=g)
    y[0, :, 0, :] = 0.0  # exact zeros; randn gives the negative values
    assert (y == 0).any() and (y < 0).any() and (y > 0).any()
    return y.to(dtype)


def _weights(n, dtype, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(SHAPE, generator=g).to(dtype) for _ in range(n)]


def _consume(t, w, sliced):
    """One consumer of its own autograd node; ``sliced`` delivers its
    gradient as a channel slice of a wider tensor (add_cat's backward)."""
    if not sliced:
        return t * w
    wide = add_cat([(w, None), (t, None), (w, None)])
    return wide * torch.cat([w, w, w], 1)


def _unfused(y0, kinds, ws, order, sliced=()):
    """y's gradient with plain torch.relu (made with its first consumer)
    and autograd's own accumulation; consumers are created in ``order``."""
    y = y0.clone().requires_grad_(True)
    r = None
    outs = {}
    for i in order:
        if kinds[i]:
            if r is None:
                r = torch.relu(y)
            outs[i] = _consume(r, ws[i], i in sliced)
        else:
            outs[i] = _consume(y, ws[i], i in sliced)
    outs = [outs[i] for i in sorted(outs)]
    torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    return y.grad, outs


def _fused(y0, kinds, ws, used, sliced=()):
    y = y0.clone().requires_grad_(True)
    aliases = state_fan(y, kinds)
    assert len({id(a) for a in aliases}) == len(kinds)
    for a, k in zip(aliases, kinds):
        assert torch.equal(a, torch.relu(y) if k else y)
    outs = [_consume(aliases[i], ws[i], i in sliced) for i in used]
    torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    return y.grad, outs


# name -> (kinds in creation order, consumers used, sliced consumers,
#          addends of the longest fold)
PATTERNS = {
    "raw_only": ((False, False, False), (0, 1, 2), (), 3),
    "relu_only": ((True, True, True), (0, 1, 2), (), 3),
    "one_relu": ((True,), (0,), (), 1),
    "states0": ((True, True, True, False), (0, 1, 2, 3), (), 3),
    "states1": ((True, False, False, False), (0, 1, 2, 3), (), 4),
    "relu_in_the_middle": ((False, True, False, True, False), (0, 1, 2, 3, 4), (), 4),
    "unused_alias": ((True, False, True, False, False), (0, 1, 3, 4), (), 4),
    "unused_first_relu": ((True, False, True, False), (1, 2, 3), (), 3),
    "sliced_raw": ((True, False, False, False), (0, 1, 2, 3), (3,), 4),
    "sliced_all": ((True, True, False, False), (0, 1, 2, 3), (0, 1, 2, 3), 3),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_state_fan_matches_unfused(name, dtype):
    kinds, used, sliced, addends = PATTERNS[name]
    seed = sorted(PATTERNS).index(name)
    y0 = _state(dtype, seed)
    ws = _weights(len(kinds), dtype, seed)
    want, want_outs = _unfused(y0, kinds, ws, used, sliced)
    got, got_outs = _fused(y0, kinds, ws, used, sliced)
    for a, b in zip(got_outs, want_outs):
        assert torch.equal(a, b)
    assert got.dtype == want.dtype and torch.equal(got, want)
    if dtype == torch.bfloat16 and addends >= 3:
        # the case can fail: the same consumers folded the other way round
        # give other bits somewhere
        other, _ = _unfused(y0, kinds, ws, tuple(reversed(used)), sliced)
        assert not torch.equal(other, want), "seed shows nothing about order"


def test_state_fan_nothing_used():
    y = _state(torch.float32, 0).requires_grad_(True)
    a, b = state_fan(y, (False, True))
    (g,) = torch.autograd.grad((y * 2).sum(), y)
    assert torch.equal(g, torch.full_like(y, 2))
    del a, b


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_shared_relu_matches_separate_relus(dtype):
    """Three modules with a ReLU each on one tensor (the stem's output)."""
    y0 = _state(dtype, 3)
    ws = _weights(3, dtype, 3)
    y = y0.clone().requires_grad_(True)
    outs = [torch.relu(y) * w for w in ws]
    torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    for leaf_input in (False, True):  # shared / a ReLU per request
        leaf = y0.clone().requires_grad_(True)
        t = leaf if leaf_input else leaf * 1
        outs2 = [shared_relu(t) * w for w in ws]
        assert (outs2[0].grad_fn.next_functions[0][0]
                is outs2[1].grad_fn.next_functions[0][0]) != leaf_input
        torch.autograd.backward(outs2, [torch.ones_like(o) for o in outs2])
        assert torch.equal(leaf.grad, y.grad)
        for a, b in zip(outs, outs2):
            assert torch.equal(a, b)


def test_shared_relu_table():
    gc.collect()
    assert len(fuse._relu_memo) == 0
    leaf = _state(torch.float32, 4).requires_grad_(True)
    # a leaf that requires grad is never entered (its AccumulateGrad node
    # would keep it alive through a waiting alias)
    shared_relu(leaf)
    assert len(fuse._relu_memo) == 0
    t = leaf * 1
    a = shared_relu(t)
    b = shared_relu(t)
    assert a is not b and a.data_ptr() == b.data_ptr()  # one ReLU
    twin = leaf * 1  # equal values, another object
    c = shared_relu(twin)
    assert c.data_ptr() != a.data_ptr() and torch.equal(c, a)
    assert len(fuse._relu_memo) == 2
    # the requests past the pre-made aliases start afresh
    d, e = shared_relu(t), shared_relu(t)
    assert d.data_ptr() == a.data_ptr() and e.data_ptr() != a.data_ptr()
    # another grad mode does not get the graph-mode aliases
    with torch.no_grad():
        f = shared_relu(t)
    assert not f.requires_grad
    # sharing off: a ReLU per request, nothing in the table
    with fuse.relu_sharing(False):
        n = len(fuse._relu_memo)
        p, q = shared_relu(twin), shared_relu(twin)
        assert p.data_ptr() != q.data_ptr() and len(fuse._relu_memo) == n
    del a, b, c, d, e, f, p, q, t, twin, leaf
    gc.collect()
    assert len(fuse._relu_memo) == 0


def _cell_run(make, inputs, glue, monkeypatch):
    monkeypatch.setenv("MPI4DL_CELL_GLUE", "1" if glue else "0")
    torch.manual_seed(7)
    net = make()
    net.train()
    xs = [x.clone().requires_grad_(True) for x in inputs]
    out = net(tuple(xs) if len(xs) > 1 else xs[0])
    outs = out if isinstance(out, tuple) else (out,)
    g = torch.Generator().manual_seed(11)
    loss = sum((o * torch.randn(o.shape, generator=g)).sum() for o in outs[:1])
    loss.backward()
    grads = {n: p.grad for n, p in net.named_parameters()}
    return outs[0].detach(), [x.grad for x in xs], grads


def _same(a, b):
    oa, xa, ga = a
    ob, xb, gb = b
    assert torch.equal(oa, ob)
    for u, v in zip(xa, xb):
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v))
    assert ga.keys() == gb.keys()
    for n in ga:
        assert (ga[n] is None) == (gb[n] is None), n
        assert ga[n] is None or torch.equal(ga[n], gb[n]), n


@pytest.mark.parametrize("reduction", [False, True])
def test_cell_glue_on_equals_off(reduction, monkeypatch):
    from mpi4dl_amd.models.amoebanet import Cell
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    def make():
        return Cell(24, 32, 8, reduction, False, mknorm=TileBatchNorm2d)

    g = torch.Generator().manual_seed(5)
    s1 = torch.randn(2, 32, 8, 8, generator=g)
    s2 = torch.randn(2, 24, 8, 8, generator=g)
    on = _cell_run(make, [s1, s2], True, monkeypatch)
    off = _cell_run(make, [s1, s2], False, monkeypatch)
    _same(on, off)


def test_cell_fan_plan():
    """The plan follows node creation, not get() order: the reduction
    cell's states[3] is read raw by op 6, whose sum lives only in the
    concat (AddCat, created last), and through ReLU by op 9."""
    from mpi4dl_amd.models.amoebanet import Cell

    red = Cell(24, 32, 8, True, False)
    assert red._fans[3] == ((True, False), {9: 0, 6: 1})
    nor = Cell(24, 32, 8, False, False)
    assert nor._fans[0] == ((True, True, True, False), {3: 0, 4: 1, 5: 2, "cat": 3})
    assert nor._fans[1] == ((True, False, False, False), {0: 0, 1: 1, 8: 2, 2: 3})
    assert nor._fans[2] == ((False, False), {6: 0, 7: 1})
    assert nor._fans[5] == ((True,), {9: 0})
    assert set(nor._fans) == {0, 1, 2, 5}


def test_model_glue_on_equals_off(monkeypatch):
    """The whole small model: cell outputs shared between the next two
    cells, the stem's output between three reductions, FactorizedReduce."""
    from mpi4dl_amd.models.amoebanet import amoebanetd

    def make():
        return amoebanetd(num_classes=5, num_layers=3, num_filters=32)

    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    on = _cell_run(make, [x], True, monkeypatch)
    off = _cell_run(make, [x], False, monkeypatch)
    _same(on, off)
    gc.collect()
    assert len(fuse._relu_memo) == 0
