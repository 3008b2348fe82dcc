"""GPU (MI355X) tests of the cell glue: the fan_bwd kernel against the
unfused path (torch.relu per consumer, autograd's own accumulation) on the
same device, and a cell's step under hipGraph. bf16, and
torch.equal wherever the arithmetic is order-free."""

import pytest
import torch

gpu = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

BF = torch.bfloat16


def _randn(shape, seed, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).cuda()


def _state(shape, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(shape, generator=g)
    y[:, :, 0, :] = 0.0  # exact zeros; randn gives the negative values
    return y.to(BF).cuda()


def _consume(t, w, place):
    """One consumer with an autograd node of its own. place = (offset,
    total): the consumer is a concat of ``total`` channels that holds t at
    channel ``offset``, so t's gradient arrives as that slice."""
    from mpi4dl_amd.ops.fuse import add_cat

    if place is None:
        return t * w
    off, total = place
    n, c, h, wd = t.shape
    parts = []
    if off:
        parts.append((w.new_ones(n, off, h, wd), None))
    parts.append((t, None))
    if total - off - c:
        parts.append((w.new_ones(n, total - off - c, h, wd), None))
    wide = add_cat(parts)
    scale = w.repeat(1, (total + c - 1) // c, 1, 1)[:, :total]
    return wide * scale


def _grad(y0, kinds, used, places, ws, fused):
    from mpi4dl_amd.ops.fuse import state_fan

    y = y0.clone().requires_grad_(True)
    outs = []
    if fused:
        aliases = state_fan(y, kinds)
        for i in used:
            outs.append(_consume(aliases[i], ws[i], places.get(i)))
    else:
        r = None
        for i in used:
            if kinds[i] and r is None:
                r = torch.relu(y)
            outs.append(_consume(r if kinds[i] else y, ws[i], places.get(i)))
    torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    return y.grad


def _check(shape, kinds, used=None, places=None, seed=0, monkeypatch=None):
    from mpi4dl_amd.ops import fuse

    used = tuple(range(len(kinds))) if used is None else used
    places = places or {}
    y0 = _state(shape, seed)
    ws = [_randn(shape, 100 + seed + i) for i in range(len(kinds))]
    want = _grad(y0, kinds, used, places, ws, fused=False)

    def no_torch_fold(*a):
        raise AssertionError("the torch fold ran on the GPU")

    monkeypatch.setattr(fuse, "_fold_torch", no_torch_fold)
    got = _grad(y0, kinds, used, places, ws, fused=True)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(got, want), (got.float() - want.float()).abs().max()


@gpu
@requires_gpu
def test_fan_concat_slices_vector_path(monkeypatch):
    """(2, 11, 4, 8) concat buffer, slices at channels 0 / 3 / 7 of widths
    3 / 4 / 4: whole 16-byte slots, aligned slice bases, a batch stride."""
    _check((2, 3, 4, 8), (True, False, False), places={2: (0, 11)},
           monkeypatch=monkeypatch)
    _check((2, 4, 4, 8), (True, True, False, False),
           places={2: (3, 11), 3: (7, 11)}, seed=1, monkeypatch=monkeypatch)
    _check((2, 4, 4, 8), (False, True, False), places={1: (7, 11), 2: (3, 11)},
           seed=2, monkeypatch=monkeypatch)


@gpu
@requires_gpu
def test_fan_ragged_planes_element_path(monkeypatch):
    """(2, 5, 5, 7): 35-element planes, and a slice base off the 16-byte
    grid (channel 3 of 9)."""
    _check((2, 5, 5, 7), (True, False, False, True), monkeypatch=monkeypatch)
    _check((2, 5, 5, 7), (True, False, False), places={1: (3, 9), 2: (0, 9)},
           seed=1, monkeypatch=monkeypatch)


@gpu
@requires_gpu
@pytest.mark.parametrize("nrel", [0, 1, 2, 3])
@pytest.mark.parametrize("nraw", [1, 2, 3, 4])
def test_fan_term_counts(nraw, nrel, monkeypatch):
    """(3, 9, 16, 24), every count of raw and ReLU terms the cells use and
    more, the ReLU consumers in the middle of the raw ones, one alias
    unused (a None gradient), one raw gradient a slice."""
    kinds = [False] * nraw
    kinds[1:1] = [True] * nrel
    kinds = tuple(kinds) + (False, True)  # the unused ones
    used = tuple(range(nraw + nrel))
    places = {nraw + nrel - 1: (2, 20)}
    _check((3, 9, 16, 24), kinds, used, places, seed=nraw * 4 + nrel,
           monkeypatch=monkeypatch)


@gpu
@requires_gpu
def test_fan_grid_stride(monkeypatch):
    """The launcher caps the grid at 4096 blocks of 256 threads: an image
    of more than 4096 * 256 * 8 bf16 elements makes threads loop."""
    shape = (1, 4, 1024, 2056)
    assert shape[1] * shape[2] * shape[3] > 4096 * 256 * 8
    _check(shape, (True, False, False), monkeypatch=monkeypatch)


def _cell_step(cell, s1, s2, wout):
    with torch.autocast("cuda", dtype=BF):
        out, _ = cell((s1, s2))
    return torch.autograd.grad((out * wout).sum(), (s1, s2))


@gpu
@requires_gpu
def test_cell_hipgraph_and_switch(monkeypatch):
    """A normal cell's forward and backward, bf16 autocast on the native kernels:
    captured in a hipGraph and replayed twice, the gradients of the cell's
    inputs equal the eager run's, and the eager run's equal the unfused
    path's. Every fan of the cell lies on the way to them. The conv
    weights' gradients are left out: their kernels add with fp32 atomics in
    an order that differs from run to run."""
    from mpi4dl_amd.models.amoebanet import Cell
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    torch.manual_seed(0)
    cell = Cell(48, 64, 16, False, False, mknorm=TileBatchNorm2d)
    cell = cell.cuda().train()
    s1 = _randn((2, 64, 16, 24), 1).requires_grad_(True)
    s2 = _randn((2, 48, 16, 24), 2).requires_grad_(True)
    wout = _randn((2, 64, 16, 24), 3)

    monkeypatch.setenv("MPI4DL_CELL_GLUE", "0")
    off = [g.clone() for g in _cell_step(cell, s1, s2, wout)]
    monkeypatch.setenv("MPI4DL_CELL_GLUE", "1")
    eager = [g.clone() for g in _cell_step(cell, s1, s2, wout)]
    for a, c in zip(eager, off):
        assert torch.equal(a, c)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _cell_step(cell, s1, s2, wout)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = _cell_step(cell, s1, s2, wout)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for a, c in zip(static, eager):
            assert torch.equal(a, c)
