"""Every tile of a grid on one device: a loopback transport and two
oracles for ``HaloExchanger``.

Shared by ``test_halo_loopback.py`` (CPU: torch-slicing packer) and
``test_gpu_halo_loopback.py`` (MI355X: staging buffers and the
``halo_pack`` / ``halo_unpack`` / ``halo_unpack_add`` kernels).

* ``Loopback``: an in-process mailbox in the place of
  ``mpi4dl_amd.ops.halo.p2p.exchange``. ``exchange`` stores a clone of
  every send under (src, dst, tag); a transfer's ``wait`` copies
  (peer, me, tag) into each recv buffer and removes it. No threads, no
  process group, no second device. An empty mailbox afterwards means
  that every send was received exactly once: peers and tags pair up.
* ``Grid``: one ``HaloExchanger`` per tile; ``run`` calls begin for every
  tile, then finish for every tile, then asserts the mailbox is empty.
* ``fwd_case`` / ``grad_case``: the oracles, written on the
  global image and sharing nothing with the code under test.
  Forward: the finished padded tile is the matching window of the
  zero-padded global image. Transposed: every tile's padded gradient is
  folded into a zero canvas of the padded global size at its global
  position; the canvas cropped to the image, sliced per tile, is what
  each tile must return. D2 tiles carry pads on interior sides only
  (``pads_d2``) and are placed at their own offsets.

Data are integers from a seeded generator, so every comparison is
``torch.equal``. A gradient pixel of a tile is covered by the padded
windows of ``k`` tiles; values are drawn from [1, min(60, 255 // k)], so
every partial sum is an integer below 256 and exact in bf16 and fp16
whatever the order of the adds. k is 4 at most (values up to 60) while
the halo is smaller than the tile; the whole-tile halo 8 on the 3x3 grid
reaches k = 9 (values up to 28). k is the maximum of the same fold over
ones.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

T = 8           # tile edge
N, C = 2, 3
# (slice_method, parts): 2x2, 3x3 (centre tile: all 8 strips), 1x2, 3x1
GRIDS = [("square", 4), ("square", 9), ("vertical", 2), ("horizontal", 3)]
HALOS = [1, 3, (0, 3), (3, 0), (2, 1), 8]   # 8: the whole tile
CASES = [(g, h, d2) for g in GRIDS for h in HALOS for d2 in (False, True)]


def case_id(case):
    (method, parts), h, d2 = case
    hs = "x".join(map(str, h)) if isinstance(h, tuple) else str(h)
    return f"{method}{parts}-h{hs}-{'d2' if d2 else 'sym'}"


class Loopback:
    """The mailbox. ``me`` is the tile whose exchanger runs next.

    ``prime`` serves blocking callers (the autograd Functions), which
    cannot run begin for every tile first: a primed pass posts each
    tile's sends and delivers nothing, the real pass after it must post
    the very same messages and receives them."""

    def __init__(self):
        self.box = {}
        self.me = None
        self.prime = False
        self._primed = {}

    def pending(self):
        """Messages not yet received, or primed and not yet re-posted."""
        return sorted(self.box) + sorted(self._primed)

    def exchange(self, sends, recvs):
        me = self.me
        for t, peer, tag in sends:
            key = (me, peer, tag)
            if key in self._primed and not self.prime:
                # its receiver may have taken it from the box already
                assert torch.equal(self._primed.pop(key), t), key
                continue
            assert key not in self.box, f"sent twice: {key}"
            self.box[key] = t.clone()
            if self.prime:
                self._primed[key] = self.box[key]
        return _Transfer(self, me, recvs)


class _Transfer:
    def __init__(self, loop, me, recvs):
        self.loop, self.me, self.recvs = loop, me, recvs

    def wait(self):
        if self.loop.prime:
            return
        for buf, peer, tag in self.recvs:
            buf.copy_(self.loop.box.pop((peer, self.me, tag)))


def install(monkeypatch):
    from mpi4dl_amd.ops import halo

    loop = Loopback()
    monkeypatch.setattr(halo.p2p, "exchange", loop.exchange)
    return loop


class Grid:
    def __init__(self, grid, loop):
        from mpi4dl_amd.ops.halo import HaloExchanger, TileLayout

        method, parts = grid
        self.loop = loop
        self.layout = TileLayout(parts, method)
        self.exs = [
            HaloExchanger(self.layout, t, lambda t: t) for t in range(parts)
        ]
        self.Hg, self.Wg = self.layout.rows * T, self.layout.cols * T

    def each(self, fn):
        """fn(tile, exchanger) for every tile in turn."""
        out = []
        for t, ex in enumerate(self.exs):
            self.loop.me = t
            out.append(fn(t, ex))
        return out

    def run(self, begin):
        """begin(tile, exchanger) -> finish for every tile, then every
        finish(); every message must have been received."""
        outs = [finish() for finish in self.each(begin)]
        assert not self.loop.pending(), self.loop.pending()
        return outs

    def pads(self, t, h, d2):
        """(top, bottom, left, right) pads of tile t."""
        hh, hw = (h, h) if isinstance(h, int) else h
        return self.exs[t].pads_d2(h) if d2 else (hh, hh, hw, hw)

    def kwargs(self, t, h, d2):
        """off / nominal of tile t as the exchanger takes them."""
        if not d2:
            return {}
        top, _, left, _ = self.pads(t, h, d2)
        return {"off": (top, left), "nominal": (T, T)}

    def window(self, t, h, d2):
        """Row and column slices of tile t's padded window inside the
        global image padded by (hh, hw)."""
        hh, hw = (h, h) if isinstance(h, int) else h
        r, c = self.layout.pos(t)
        top, bottom, left, right = self.pads(t, h, d2)
        return (slice(r * T + hh - top, r * T + hh + T + bottom),
                slice(c * T + hw - left, c * T + hw + T + right))


def _ints(gen, shape, hi):
    return torch.randint(1, hi + 1, shape, generator=gen).double()


def fwd_case(grid: Grid, h, d2, seed):
    """-> (global image, padded tile inputs, expected finished tiles),
    float64 CPU."""
    hh, hw = (h, h) if isinstance(h, int) else h
    gen = torch.Generator().manual_seed(seed)
    full = _ints(gen, (N, C, grid.Hg, grid.Wg), 60)
    fullp = F.pad(full, (hw, hw, hh, hh))
    xps, expect = [], []
    for t in range(len(grid.exs)):
        top, bottom, left, right = grid.pads(t, h, d2)
        tile = grid.layout.slice_input(full, t)
        xps.append(F.pad(tile, (left, right, top, bottom)))
        rows, cols = grid.window(t, h, d2)
        expect.append(fullp[:, :, rows, cols])
    return full, xps, expect


def _fold(grid: Grid, h, d2, pieces):
    hh, hw = (h, h) if isinstance(h, int) else h
    canvas = torch.zeros(N, C, grid.Hg + 2 * hh, grid.Wg + 2 * hw,
                         dtype=torch.float64)
    for t, p in enumerate(pieces):
        rows, cols = grid.window(t, h, d2)
        canvas[:, :, rows, cols] += p
    return canvas[:, :, hh:hh + grid.Hg, hw:hw + grid.Wg]


def grad_case(grid: Grid, h, d2, seed):
    """-> (padded tile gradients, expected unpadded tile gradients),
    float64 CPU."""
    shapes = []
    for t in range(len(grid.exs)):
        top, bottom, left, right = grid.pads(t, h, d2)
        shapes.append((N, C, T + top + bottom, T + left + right))
    k = int(_fold(grid, h, d2, [torch.ones(s, dtype=torch.float64)
                                for s in shapes]).max())
    gen = torch.Generator().manual_seed(seed)
    gps = [_ints(gen, s, min(60, 255 // k)) for s in shapes]
    folded = _fold(grid, h, d2, gps)
    assert folded.max() < 256
    expect = [grid.layout.slice_input(folded, t)
              for t in range(len(grid.exs))]
    return gps, expect


def check_forward(grid: Grid, h, d2, device, dtype, seed=0):
    _, xps, expect = fwd_case(grid, h, d2, seed)
    xps = [x.to(device=device, dtype=dtype).contiguous() for x in xps]
    grid.run(lambda t, ex: ex.exchange_padded_async(
        xps[t], h, **grid.kwargs(t, h, d2)))
    for t, (got, want) in enumerate(zip(xps, expect)):
        assert got.dtype == dtype
        assert torch.equal(got.double().cpu(), want), f"tile {t}"


def check_transposed(grid: Grid, h, d2, device, dtype, seed=0):
    gps, expect = grad_case(grid, h, d2, seed)
    gps = [g.to(device=device, dtype=dtype).contiguous() for g in gps]
    outs = grid.run(lambda t, ex: ex.exchange_grad_padded_async(
        gps[t], h, **grid.kwargs(t, h, d2)))
    for t, (got, want) in enumerate(zip(outs, expect)):
        assert got.dtype == dtype and got.shape[-2:] == (T, T)
        assert torch.equal(got.double().cpu(), want), f"tile {t}"


def check_autograd(grid: Grid, h, d2, device, dtype):
    """halo_pad / halo_pad_d2 with grad_mode='exact', forward and
    backward, against the same two oracles. The Functions block, so a
    primed pass posts every tile's messages first (``Loopback.prime``)."""
    from mpi4dl_amd.ops.halo import halo_pad, halo_pad_d2

    pad = halo_pad_d2 if d2 else halo_pad
    loop = grid.loop
    full, _, fwd_expect = fwd_case(grid, h, d2, 0)
    gps, grad_expect = grad_case(grid, h, d2, 0)
    gps = [g.to(device=device, dtype=dtype) for g in gps]

    def leaves():
        return [grid.layout.slice_input(full, t).to(device=device, dtype=dtype)
                .contiguous().requires_grad_(True)
                for t in range(len(grid.exs))]

    def forward(xs):
        return grid.each(lambda t, ex: pad(xs[t], h, ex, "exact"))

    loop.prime = True
    primed = forward(leaves())
    loop.prime = False
    xs = leaves()
    outs = forward(xs)
    assert not loop.pending(), loop.pending()
    for t, (got, want) in enumerate(zip(outs, fwd_expect)):
        assert torch.equal(got.detach().double().cpu(), want), f"tile {t}"

    loop.prime = True
    grid.each(lambda t, ex: primed[t].backward(gps[t]))
    loop.prime = False
    grid.each(lambda t, ex: outs[t].backward(gps[t]))
    assert not loop.pending(), loop.pending()
    for t, (x, want) in enumerate(zip(xs, grad_expect)):
        assert torch.equal(x.grad.double().cpu(), want), f"tile {t}"


ENTRY_POINTS = ["exchange_padded", "exchange_padded_async",
                "exchange_grad_padded", "exchange_grad_padded_async"]
