"""Halo exchange primitive for spatial (tile) parallelism.

Reference parity: the 9-neighbour exchange inside ``conv_spatial``
(src/torchgems/spatial.py:336-413, neighbour tables :868-1018) and the
standalone ``halo_exchange_layer`` (:1032-1413).

MI355X-native design:
* All strips of one exchange are issued as ONE grouped RCCL P2P call
  (p2p.exchange) — every xGMI link carries its neighbour's message
  concurrently; no MPI tags, no host-side synchronize fences
  (the reference needed manual ``torch.cuda.synchronize`` + tag
  discipline, spatial.py:170-175, 377-383).
* Strips are packed/unpacked with torch slicing on CPU and with the
  gemscore HIP pack/unpack kernels on gfx950 (ops/backend.py) — one
  kernel per exchange instead of 8 ``.clone()`` launches.
* Backward is a REAL transposed halo exchange (``grad_mode='exact'``):
  pad-ring gradients are returned to the neighbour that owns those
  pixels and accumulated, making distributed training mathematically
  identical to single-GPU. ``grad_mode='drop'`` reproduces the
  reference's behaviour (halo grads silently dropped —
  SURVEY.md §3.2 note) for apples-to-apples comparison.
* Meta tensors short-circuit: shape-correct output, no communication
  (used by the partitioner's shape inference).
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn.functional as F

from .. import p2p

# direction index (dr, dc) — receiver-side tag = direction the strip
# arrives FROM, so sender tags with the opposite direction.
DIRS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
_DIR_IDX = {d: i for i, d in enumerate(DIRS)}


def _opposite(d: Tuple[int, int]) -> Tuple[int, int]:
    return (-d[0], -d[1])


@dataclass
class TileLayout:
    """Grid placement of spatial tiles (reference slice_method semantics:
    'square' = row-major sqrt(p) x sqrt(p) grid; 'vertical' = W-strips;
    'horizontal' = H-strips — train_spatial.py:241-290)."""

    num_parts: int
    slice_method: str = "square"

    def __post_init__(self):
        if self.slice_method == "square":
            r = int(math.isqrt(self.num_parts))
            assert r * r == self.num_parts, (
                f"square slicing needs a square part count, got {self.num_parts}"
            )
            self.rows, self.cols = r, r
        elif self.slice_method == "vertical":
            self.rows, self.cols = 1, self.num_parts
        elif self.slice_method == "horizontal":
            self.rows, self.cols = self.num_parts, 1
        else:
            raise ValueError(f"unknown slice_method {self.slice_method}")

    def pos(self, tile: int) -> Tuple[int, int]:
        return divmod(tile, self.cols)

    def tile_at(self, row: int, col: int) -> Optional[int]:
        if 0 <= row < self.rows and 0 <= col < self.cols:
            return row * self.cols + col
        return None

    def neighbours(self, tile: int) -> List[Tuple[Tuple[int, int], int]]:
        """[(direction, neighbour_tile)] for existing neighbours."""
        r, c = self.pos(tile)
        out = []
        for d in DIRS:
            t = self.tile_at(r + d[0], c + d[1])
            if t is not None:
                out.append((d, t))
        return out

    def slice_input(self, x: torch.Tensor, tile: int) -> torch.Tensor:
        """My tile of the full input (reference split_input,
        train_spatial.py:241-290)."""
        H, W = x.shape[-2], x.shape[-1]
        r, c = self.pos(tile)
        th, tw = H // self.rows, W // self.cols
        return x[..., r * th : (r + 1) * th, c * tw : (c + 1) * tw]


def _hpair(h):
    """halo spec -> (hh, hw): rows halo, cols halo (asymmetric kernels
    like AmoebaNet's 1x7/7x1 exchange in one axis only)."""
    if isinstance(h, (tuple, list)):
        return int(h[0]), int(h[1])
    return int(h), int(h)


def send_region(d, H, W, h, off=None):
    """Interior boundary band (in padded coords) sent toward direction d.

    ``off`` = (top, left) pad offsets of the nominal region inside the
    padded tensor; defaults to (hh, hw) (symmetric pad). D2 tiles pad
    interior sides only, so boundary tiles pass off 0 for those sides.
    """
    hh, hw = _hpair(h)
    t, l = (hh, hw) if off is None else off
    dr, dc = d
    rs = {-1: (t, t + hh), 0: (t, t + H), 1: (t + H - hh, t + H)}[dr]
    cs = {-1: (l, l + hw), 0: (l, l + W), 1: (l + W - hw, l + W)}[dc]
    return rs, cs


def recv_region(d, H, W, h, off=None):
    hh, hw = _hpair(h)
    t, l = (hh, hw) if off is None else off
    dr, dc = d
    rs = {-1: (t - hh, t), 0: (t, t + H), 1: (t + H, t + H + hh)}[dr]
    cs = {-1: (l - hw, l), 0: (l, l + W), 1: (l + W, l + W + hw)}[dc]
    return rs, cs


@dataclass
class _Strip:
    """One neighbour's share of an exchange: what goes to ``peer`` and
    what comes back. Boxes are (row, col, rows, cols)."""

    peer: int
    send_tag: int
    send_box: Tuple[int, int, int, int]
    recv_tag: int
    recv_box: Tuple[int, int, int, int]


def _box(x, box):
    r, c, rows, cols = box
    return x[:, :, r : r + rows, c : c + cols]


class HaloExchanger:
    """Performs forward halo exchange and (optionally) the transposed
    backward exchange among the tile ranks of one spatial partition.

    ``rank_of_tile`` maps tile index -> global rank (built by the caller
    from Communicator topology, honouring GEMS inversion —
    reference spatial.py:913-918).
    """

    def __init__(self, layout: TileLayout, tile: int, rank_of_tile):
        self.layout = layout
        self.tile = tile
        self.rank_of_tile = rank_of_tile
        self.neigh = layout.neighbours(tile)
        # (shape, h, dtype, device, grad, off, nominal) -> strips, and on
        # the GPU their descriptors and flat staging buffers
        self._plans = {}

    def pads_d2(self, h):
        """Per-side pad amounts (top, bottom, left, right) for D2 mode:
        interior sides get the halo pad, image-boundary sides get none
        (each conv re-applies its own zero pad there)."""
        hh, hw = _hpair(h)
        r, c = self.layout.pos(self.tile)
        t = hh if r > 0 else 0
        b = hh if r < self.layout.rows - 1 else 0
        l = hw if c > 0 else 0
        rr = hw if c < self.layout.cols - 1 else 0
        return t, b, l, rr

    def crop_d2(self, x, n):
        """Crop n surplus pixels from each interior side (the inverse of
        a D2 pad by n; image-boundary sides carry no surplus)."""
        t, b, l, r = self.pads_d2(n)
        H, W = x.shape[-2], x.shape[-1]
        return x[:, :, t : H - b, l : W - r]

    # -- the strip plan ------------------------------------------------------

    def _strips(self, H, W, h, off, grad):
        """One _Strip per neighbour that takes part. The only place that
        walks the neighbours.

        Forward packs send_region of the padded tile and unpacks into its
        recv_region. The transposed (``grad``) exchange runs the other
        way: the ring band received FROM d in forward carries gradients
        for that neighbour's interior, so recv_region is packed, and what
        comes back belongs to the strips SENT in forward: send_region,
        shifted by (-t0, -l0) because it is added into the UNpadded tile.
        The receiver tags by arrival direction, so a send carries the
        opposite of its direction of travel; gradients use tags 8..15.
        """
        hh, hw = _hpair(h)
        t0, l0 = (hh, hw) if off is None else off
        src, dst = (recv_region, send_region) if grad else (send_region, recv_region)
        up, left, tagb = (t0, l0, 8) if grad else (0, 0, 0)
        strips = []
        for d, t in self.neigh:
            if (d[0] != 0 and hh == 0) or (d[1] != 0 and hw == 0):
                continue  # no halo along that axis
            (ss, se), (cs, ce) = src(d, H, W, h, off)
            (rs, re), (ks, ke) = dst(d, H, W, h, off)
            strips.append(_Strip(
                self.rank_of_tile(t),
                tagb + _DIR_IDX[_opposite(d)], (ss, cs, se - ss, ce - cs),
                tagb + _DIR_IDX[d], (rs - up, ks - left, re - rs, ke - ks),
            ))
        return strips

    def _plan(self, xp, H, W, h, off, nominal, grad):
        """Cached strips; for a CUDA tensor also the pack/unpack
        descriptors and the flat staging buffers with one view per strip,
        so a call allocates nothing."""
        key = (tuple(xp.shape), _hpair(h), xp.dtype, xp.device, grad, off, nominal)
        plan = self._plans.get(key)
        if plan is None:
            strips = self._strips(H, W, h, off, grad)
            plan = self._plans[key] = {"strips": strips}
            if xp.is_cuda and strips:
                nc = xp.shape[0] * xp.shape[1]
                for side in "sr":
                    boxes = [s.send_box if side == "s" else s.recv_box for s in strips]
                    sizes = [nc * b[2] * b[3] for b in boxes]
                    flat = torch.empty(sum(sizes), device=xp.device, dtype=xp.dtype)
                    plan[side + "desc"] = torch.tensor(boxes, dtype=torch.int64)
                    plan[side + "buf"] = flat
                    plan[side + "views"] = list(flat.split(sizes))
        return plan

    # -- begin / finish ------------------------------------------------------

    def _begin(self, xp, h, off, nominal, grad):
        """Pack and post one exchange; the returned finish() waits for it,
        unpacks and returns the result: ``xp`` with its ring filled, or
        for ``grad`` the unpadded tile with the neighbours' ring
        gradients added."""
        hh, hw = _hpair(h)
        if nominal is None:
            H, W = xp.shape[-2] - 2 * hh, xp.shape[-1] - 2 * hw
        else:
            H, W = nominal
        out = xp
        if grad:
            t0, l0 = (hh, hw) if off is None else off
            out = xp[:, :, t0 : t0 + H, l0 : l0 + W].clone(
                memory_format=torch.contiguous_format
            )
        if (hh == 0 and hw == 0) or not self.neigh:
            return lambda: out
        assert hh <= H and hw <= W, (
            f"halo ({hh},{hw}) exceeds local tile {H}x{W}: the spatial "
            "region extends past the resolution where tiling is valid - "
            "shrink spatial_size / use fewer tiles (the reference has the "
            "same constraint, it just corrupts silently)"
        )
        plan = self._plan(xp, H, W, h, off, nominal, grad)
        strips = plan["strips"]
        if not strips:  # the neighbours lie along an axis without halo
            return lambda: out
        if xp.is_cuda:
            from . import backend

            ge = backend.ext()
            ge.halo_pack(xp, plan["sbuf"], plan["sdesc"])
            sbufs, rbufs = plan["sviews"], plan["rviews"]
        else:
            sbufs = [_box(xp, s.send_box).contiguous() for s in strips]
            rbufs = [xp.new_empty(xp.shape[:2] + s.recv_box[2:]) for s in strips]
        tr = p2p.exchange(
            [(b, s.peer, s.send_tag) for b, s in zip(sbufs, strips)],
            [(b, s.peer, s.recv_tag) for b, s in zip(rbufs, strips)],
        )

        def finish():
            tr.wait()
            if xp.is_cuda:
                unpack = ge.halo_unpack_add if grad else ge.halo_unpack
                unpack(out, plan["rbuf"], plan["rdesc"])
            else:
                for b, s in zip(rbufs, strips):
                    if grad:
                        _box(out, s.recv_box).add_(b)
                    else:
                        _box(out, s.recv_box).copy_(b)
            return out

        return finish

    def exchange_padded_async(self, xp: torch.Tensor, h, off=None, nominal=None):
        """Start filling xp's pad ring (width h) from the neighbours and
        return a finish() callable.

        xp: (N, C, H+2h, W+2h), already zero-padded (symmetric) — or, in
        D2 mode, padded on interior sides only, with ``off`` = (top,
        left) pad offsets and ``nominal`` = (H, W) of the nominal region.

        Used by the halo/compute overlap path (_overlap_halo_apply):
        pack+send/recv are issued now; finish() waits the transfer and
        unpacks the ring, AFTER the caller has queued interior compute.
        On RCCL everything is stream-ordered; the comm rides RCCL's own
        streams so the interior conv overlaps the wire time.
        """
        return self._begin(xp, h, off, nominal, grad=False)

    def exchange_padded(self, xp: torch.Tensor, h, off=None, nominal=None) -> None:
        """In-place, blocking exchange_padded_async."""
        from ..utils import GLOBAL_TIMER  # noqa: F811 (cheap; cached import)

        if xp.is_cuda and any(_hpair(h)) and self.neigh:
            with GLOBAL_TIMER.phase("halo/exchange"):
                self.exchange_padded_async(xp, h, off, nominal)()
        else:
            self.exchange_padded_async(xp, h, off, nominal)()

    def exchange_grad_padded_async(self, gp: torch.Tensor, h, off=None, nominal=None):
        """Start the transposed halo exchange; finish() returns the grad
        wrt the UNpadded tile.

        gp: gradient wrt the padded tile (N, C, H+2h, W+2h). The pad-ring
        bands belong to neighbours' interior pixels: send each band to its
        owner; add received bands into my interior edge regions.
        """
        return self._begin(gp, h, off, nominal, grad=True)

    def exchange_grad_padded(
        self, gp: torch.Tensor, h, off=None, nominal=None
    ) -> torch.Tensor:
        """Blocking exchange_grad_padded_async."""
        return self.exchange_grad_padded_async(gp, h, off, nominal)()


def exchanger_for(
    num_spatial_parts, slice_method, spatial_local_rank, rank_of_tile=None, **_
):
    """The HaloExchanger of one tile, from the keys of a plan ctx
    (``exchanger_for(**ctx)``); None where there is a single tile.
    ``rank_of_tile=None``: tile index == global rank (tests)."""
    if num_spatial_parts <= 1:
        return None
    if rank_of_tile is None:
        rank_of_tile = lambda t: t  # noqa: E731
    return HaloExchanger(
        TileLayout(num_spatial_parts, slice_method), spatial_local_rank, rank_of_tile
    )


class _HaloPadFn(torch.autograd.Function):
    """pad(x, h) + halo fill, with exact or reference ('drop') backward."""

    @staticmethod
    def forward(ctx, x, h, exchanger, grad_mode, fill):
        ctx.h = h
        ctx.exchanger = exchanger
        ctx.grad_mode = grad_mode
        hh, hw = _hpair(h)
        xp = F.pad(x, (hw, hw, hh, hh), value=fill)
        if not x.is_meta:
            exchanger.exchange_padded(xp, h)
        return xp

    @staticmethod
    def backward(ctx, gp):
        hh, hw = _hpair(ctx.h)
        if hh == 0 and hw == 0:
            return gp, None, None, None, None
        if ctx.grad_mode == "exact" and not gp.is_meta:
            g = ctx.exchanger.exchange_grad_padded(gp.contiguous(), ctx.h)
        else:
            H, W = gp.shape[-2] - 2 * hh, gp.shape[-1] - 2 * hw
            g = gp[:, :, hh : hh + H, hw : hw + W]
        return g, None, None, None, None


def halo_pad(x, h, exchanger: HaloExchanger, grad_mode: str = "exact", fill: float = 0.0):
    """Pad by h (fill value for outer/image-boundary ring, e.g. -inf for
    max pool to match single-GPU semantics) and fill interior sides from
    neighbours (autograd-aware)."""
    hh, hw = _hpair(h)
    if exchanger is None or not exchanger.neigh:
        return F.pad(x, (hw, hw, hh, hh), value=fill)
    return _HaloPadFn.apply(x, h, exchanger, grad_mode, fill)


class _OverlapExactPadFn(torch.autograd.Function):
    """F.pad only (the async exchange fills the ring outside autograd,
    overlapped with the interior conv — spatial_conv._forward_overlap);
    backward performs the exact transposed halo-gradient exchange, so
    overlap mode and grad_mode='exact' compose.

    Correctness: the band/interior decomposition computes the same
    outputs as one conv over the padded tile, so d(loss)/d(pad) is
    identical by linearity; the interior conv's input grad flows to x
    directly (autograd sums it with this Function's cropped output)."""

    @staticmethod
    def forward(ctx, x, h, exchanger, fill=0.0):
        ctx.h = h
        ctx.exchanger = exchanger
        hh, hw = _hpair(h)
        return F.pad(x, (hw, hw, hh, hh), value=fill)

    @staticmethod
    def backward(ctx, gp):
        if gp.is_meta:
            hh, hw = _hpair(ctx.h)
            H, W = gp.shape[-2] - 2 * hh, gp.shape[-1] - 2 * hw
            return gp[:, :, hh : hh + H, hw : hw + W], None, None, None
        g = ctx.exchanger.exchange_grad_padded(gp.contiguous(), ctx.h)
        return g, None, None, None


class _HaloPadD2Fn(torch.autograd.Function):
    """D2 pad: interior sides only (boundary sides stay unpadded — each
    conv re-applies its own zero pad there, reference spatial.py:67-111)."""

    @staticmethod
    def forward(ctx, x, h, exchanger, grad_mode):
        t, b, l, r = exchanger.pads_d2(h)
        ctx.h = h
        ctx.exchanger = exchanger
        ctx.grad_mode = grad_mode
        ctx.nominal = (x.shape[-2], x.shape[-1])
        ctx.off = (t, l)
        xp = F.pad(x, (l, r, t, b))
        if not x.is_meta:
            exchanger.exchange_padded(xp, h, off=(t, l), nominal=ctx.nominal)
        return xp

    @staticmethod
    def backward(ctx, gp):
        t, l = ctx.off
        H, W = ctx.nominal
        if ctx.grad_mode == "exact" and not gp.is_meta:
            g = ctx.exchanger.exchange_grad_padded(
                gp.contiguous(), ctx.h, off=ctx.off, nominal=ctx.nominal
            )
        else:
            g = gp[:, :, t : t + H, l : l + W]
        return g, None, None, None


def halo_pad_d2(x, h, exchanger: HaloExchanger, grad_mode: str = "exact"):
    """D2 fused-halo pad: grow the tile by h on interior sides only and
    fill from neighbours; the surplus is then consumed by `fused_layers`
    unpadded convs (reference resnet_spatial_d2.py design)."""
    if exchanger is None or not exchanger.neigh:
        return x
    return _HaloPadD2Fn.apply(x, h, exchanger, grad_mode)
