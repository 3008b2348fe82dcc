"""Distributed spatial nn.Modules: halo-aware conv / pool / exchange layer.

Reference parity: ``conv_spatial`` (src/torchgems/spatial.py:25-1029),
``halo_exchange_layer`` (:1032-1413), ``Pool`` (:1416-1509).

Design notes (MI355X-first):
* A module owns a HaloExchanger; communication is one grouped RCCL call
  per exchange (see ops/halo.py), stream-ordered — none of the
  reference's tag bookkeeping or host fences.
* Compute runs on halo-padded tiles with padding=0. On gfx950 the conv
  itself is either MIOpen (via F.conv2d) or the gemscore implicit-GEMM
  MFMA kernel (ops/conv_native.py), selected per-layer.
* ``grad_mode='exact'`` (default) gives bit-parity with single-GPU conv
  by doing a transposed halo exchange in backward; 'drop' reproduces the
  reference's halo-gradient-dropping semantics.
* Meta tensors: shape-only path, no comm (partitioner shape inference).
* D2 support: ``halo_len=0`` convs with asymmetric outer-edge padding by
  tile position (reference spatial.py:67-111), and a standalone
  HaloExchangeLayer with a large halo every ``fused_layers`` blocks
  (reference resnet_spatial_d2.py).
"""

from __future__ import annotations

from typing import Optional

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .conv_native import NativeConv2d
from .halo import TileLayout, _hpair, exchanger_for, halo_pad


def outer_pad_only(x: torch.Tensor, layout: TileLayout, tile: int, pad, fill: float = 0.0):
    """Asymmetric zero-pad: pad only the sides of the tile that lie on the
    image boundary (D2 design — reference spatial.py:67-111). Interior
    sides are covered by earlier large-halo exchanges."""
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    if ph == 0 and pw == 0:
        return x
    r, c = layout.pos(tile)
    left = pw if c == 0 else 0
    right = pw if c == layout.cols - 1 else 0
    top = ph if r == 0 else 0
    bottom = ph if r == layout.rows - 1 else 0
    if left or right or top or bottom:
        return F.pad(x, (left, right, top, bottom), value=fill)
    return x


def _overlap_halo_apply(op, x, hh, hw, exchanger, grad_mode, fill=0.0):
    """Generic halo/compute overlap for any k=2h+1 / stride-1 / pad-h op
    (conv or pool): start the ring exchange, run ``op`` on the interior
    while it flies, then compute the border bands from the landed ring
    and concatenate. Output == op(halo_padded(x)) exactly; gradient per
    grad_mode (exact: transposed exchange via _OverlapExactPadFn; drop:
    ring treated as constant)."""
    if grad_mode == "exact":
        from .halo import _OverlapExactPadFn

        xp = _OverlapExactPadFn.apply(x, (hh, hw), exchanger, fill)
    else:
        xp = F.pad(x, (hw, hw, hh, hh), value=fill)
    with torch.no_grad():
        finish = exchanger.exchange_padded_async(xp, (hh, hw))
    interior = op(x)
    with torch.no_grad():
        finish()
    H, W = x.shape[-2], x.shape[-1]
    rows = []
    if hh > 0:
        rows.append(op(xp[:, :, 0 : 3 * hh, :]))
    mid = [interior]
    if hw > 0:
        mid.insert(0, op(xp[:, :, hh : H + hh, 0 : 3 * hw].contiguous()))
        mid.append(op(xp[:, :, hh : H + hh, W - hw : W + 2 * hw].contiguous()))
    rows_mid = torch.cat(mid, dim=3) if len(mid) > 1 else interior
    if hh > 0:
        return torch.cat(
            [rows[0], rows_mid, op(xp[:, :, H - hh : H + 2 * hh, :])], dim=2
        )
    return rows_mid


class _SpatialBase(nn.Module):
    """Shared plumbing: layout, exchanger, rank map."""

    def __init__(
        self,
        num_spatial_parts: int,
        slice_method: str,
        spatial_local_rank: int,
        rank_of_tile=None,
        grad_mode: str = "exact",
    ):
        super().__init__()
        self.layout = TileLayout(num_spatial_parts, slice_method)
        self.tile = spatial_local_rank
        self.grad_mode = grad_mode
        self.exchanger = exchanger_for(
            num_spatial_parts, slice_method, spatial_local_rank, rank_of_tile
        )


class HaloConv2d(_SpatialBase):
    """Spatially-distributed Conv2d (reference conv_spatial, spatial.py:25).

    Forward: halo-pad the local tile by ``halo_len`` (= the padding the
    undistributed conv would use), exchange the ring with up to 8
    neighbours, then convolve with padding=0. With stride s the local
    tile size must be divisible by s (power-of-two image sizes — the
    reference's verify_spatial_config enforces the same).

    ``halo_len=None`` derives (kernel_size-1)//2. ``halo_len=0`` with
    ``d2=True`` applies asymmetric outer-edge padding instead (D2).
    """

    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        kernel_size,
        stride=1,
        padding=None,
        bias: bool = True,
        num_spatial_parts: int = 1,
        slice_method: str = "square",
        spatial_local_rank: int = 0,
        rank_of_tile=None,
        grad_mode: str = "exact",
        d2: bool = False,
        halo_len=None,
    ):
        super().__init__(
            num_spatial_parts, slice_method, spatial_local_rank, rank_of_tile, grad_mode
        )
        # int-or-pair arguments are expanded here, once: _kernel, _halo
        self._kernel = kh, kw = _hpair(kernel_size)
        padding = ((kh - 1) // 2, (kw - 1) // 2) if padding is None else _hpair(padding)
        self.halo_len = padding if halo_len is None else halo_len
        self._halo = _hpair(self.halo_len)
        self.d2 = d2
        self.outer_pad = padding if d2 else (0, 0)
        self.conv = NativeConv2d(
            in_channels, out_channels, kernel_size, stride=stride, padding=0, bias=bias
        )
        self.stride = stride
        self.kernel_size = kernel_size

    def forward(self, x):
        if self.d2 and self._halo == (0, 0):
            if self.exchanger is not None:
                xp = outer_pad_only(x, self.layout, self.tile, self.outer_pad)
            else:
                ph, pw = self.outer_pad
                xp = F.pad(x, (pw, pw, ph, ph))
        else:
            (hh, hw), (kh, kw) = self._halo, self._kernel
            if (
                self.exchanger is not None
                and not x.is_meta
                and self.stride in (1, (1, 1))
                and (hh or hw)
                # band decomposition is only valid for k == 2*halo+1 per
                # axis (i.e. padding == (k-1)//2); other paddings take the
                # blocking halo_pad path below
                and kh == 2 * hh + 1
                and kw == 2 * hw + 1
                # interior conv must be valid: tile bigger than the kernel
                and x.shape[-2] > 2 * hh
                and x.shape[-1] > 2 * hw
                # debugging knob: force the blocking exchange path
                and os.environ.get("MPI4DL_NO_OVERLAP", "0") != "1"
            ):
                return self._forward_overlap(x)
            xp = halo_pad(x, self.halo_len, self.exchanger, self.grad_mode)
        return self.conv(xp)

    def _forward_overlap(self, x):
        """Halo/compute overlap (the reference's dormant Hy-Fi design,
        spatial.py:415-826, implemented properly): the INTERIOR output
        depends only on the local tile, so its conv is queued while the
        ring is still on the wire; border bands are computed after the
        ring lands and the pieces are concatenated.

        Gradient semantics per grad_mode: 'drop' treats the received
        ring as a constant (weight grads still include ring pixels —
        identical to the blocking drop path); 'exact' routes the pad
        through _OverlapExactPadFn, whose backward performs the
        transposed halo-gradient exchange — same trajectory as the
        blocking exact path, with the forward ring overlapped.
        """
        return _overlap_halo_apply(
            self.conv, x, *self._halo, self.exchanger, self.grad_mode
        )


class HaloExchangeLayer(_SpatialBase):
    """Standalone pad+exchange module (reference halo_exchange_layer,
    spatial.py:1032). Output spatial dims grow by 2*halo_len; used by the
    D2 design to amortise one large exchange over ``fused_layers`` convs."""

    def __init__(
        self,
        halo_len: int,
        num_spatial_parts: int = 1,
        slice_method: str = "square",
        spatial_local_rank: int = 0,
        rank_of_tile=None,
        grad_mode: str = "exact",
    ):
        super().__init__(
            num_spatial_parts, slice_method, spatial_local_rank, rank_of_tile, grad_mode
        )
        self.halo_len = halo_len

    def forward(self, x):
        return halo_pad(x, self.halo_len, self.exchanger, self.grad_mode)


class HaloPool2d(_SpatialBase):
    """Spatial max/avg pool (reference Pool, spatial.py:1416): halo-pad by
    (kernel-1)//2 then pool with padding=0.

    avg pool supports BOTH count_include_pad semantics exactly:
    * True — zero-filled ring, every window divides by k*k (trivially
      equals the single-GPU op);
    * False — the divisor is the number of window cells inside the
      GLOBAL image, computed analytically from the tile's grid position
      (the reference simply refuses this case, spatial.py:1440-1441).
    """

    def __init__(
        self,
        kind: str,
        kernel_size: int,
        stride: Optional[int] = None,
        padding: int = 0,
        num_spatial_parts: int = 1,
        slice_method: str = "square",
        spatial_local_rank: int = 0,
        rank_of_tile=None,
        grad_mode: str = "exact",
        d2: bool = False,
        count_include_pad: bool = True,
    ):
        super().__init__(
            num_spatial_parts, slice_method, spatial_local_rank, rank_of_tile, grad_mode
        )
        assert kind in ("max", "avg")
        self.kind = kind
        self.kernel_size = kernel_size
        self.stride = stride or kernel_size
        self.halo_len = padding
        self.d2 = d2
        self.count_include_pad = count_include_pad

    def _avg_divisors(self, out_h, out_w, H_loc, W_loc, device):
        """Per-output-position count of window cells inside the global
        image (count_include_pad=False semantics)."""
        k, s, p = self.kernel_size, self.stride, self.halo_len
        r, c = self.layout.pos(self.tile)
        Hg, Wg = H_loc * self.layout.rows, W_loc * self.layout.cols
        gr0 = r * H_loc - p
        gc0 = c * W_loc - p
        rows = gr0 + torch.arange(out_h, device=device) * s
        cols = gc0 + torch.arange(out_w, device=device) * s
        rcnt = (torch.clamp(rows + k, max=Hg) - torch.clamp(rows, min=0)).clamp(min=0)
        ccnt = (torch.clamp(cols + k, max=Wg) - torch.clamp(cols, min=0)).clamp(min=0)
        return (rcnt.view(-1, 1) * ccnt.view(1, -1)).to(torch.float32)

    def _to_global_divisors(self, avg, H_loc, W_loc):
        """Turn count_include_pad=True averages (already rounded to the
        tensor's dtype) into count_include_pad=False ones: times k*k/div
        in fp32, rounded back once. The factor is exactly 1.0 wherever the
        window lies inside the global image, so those pixels keep their
        single rounding bit for bit; only image-border pixels round twice."""
        k = self.kernel_size
        div = self._avg_divisors(
            avg.shape[-2], avg.shape[-1], H_loc, W_loc, avg.device
        )
        return (avg * (float(k * k) / div)).to(avg.dtype)

    def forward(self, x):
        h = self.halo_len
        k, s = self.kernel_size, self.stride
        on_gpu = (
            x.is_cuda
            and not x.is_meta
            and os.environ.get("MPI4DL_NATIVE_POOL", "1") != "0"
        )
        # max pool pads with -inf so image-boundary windows match the
        # single-GPU op exactly (zero-pad would win over negative inputs)
        fill = float("-inf") if self.kind == "max" else 0.0
        H_loc, W_loc = x.shape[-2], x.shape[-1]

        # ---- plain (no tiles): padding handled inside the op ------------
        if self.exchanger is None and not self.d2:
            if self.kind == "max":
                if on_gpu:
                    from .native import native_maxpool

                    return native_maxpool(x, k, s, h)
                return F.max_pool2d(x, k, s, padding=h)
            if on_gpu:
                from .native import native_avgpool

                return native_avgpool(x, k, s, h, include_pad=self.count_include_pad)
            return F.avg_pool2d(
                x, k, s, padding=h, count_include_pad=self.count_include_pad
            )

        # ---- tiled: halo-pad then pool with padding=0 -------------------
        # stride-1 pools (AmoebaNet normal cells) get the same
        # halo/compute overlap as convs: interior pool while the ring
        # is on the wire, border bands after
        if (
            s == 1
            and h > 0
            and k == 2 * h + 1  # band decomposition needs pad == (k-1)//2
            and not self.d2
            and self.exchanger is not None
            and not x.is_meta
            and H_loc > 2 * h
            and W_loc > 2 * h
            and os.environ.get("MPI4DL_NO_OVERLAP", "0") != "1"
        ):
            if self.kind == "max":
                if on_gpu:
                    from .native import native_maxpool

                    op = lambda t: native_maxpool(t, k, s, 0)  # noqa: E731
                else:
                    op = lambda t: F.max_pool2d(t, k, s, padding=0)  # noqa: E731
                return _overlap_halo_apply(
                    op, x, h, h, self.exchanger, self.grad_mode, fill=fill
                )
            # avg: assemble include_pad sums, then global-geometry divisors
            if on_gpu:
                from .native import native_avgpool

                op = lambda t: native_avgpool(  # noqa: E731
                    t, k, s, 0, include_pad=True
                )
            else:
                op = lambda t: F.avg_pool2d(  # noqa: E731
                    t, k, s, padding=0, count_include_pad=True
                )
            out = _overlap_halo_apply(
                op, x, h, h, self.exchanger, self.grad_mode, fill=0.0
            )
            if self.count_include_pad:
                return out
            return self._to_global_divisors(out, H_loc, W_loc)
        if self.d2 and h > 0:
            xp = (
                outer_pad_only(x, self.layout, self.tile, h, fill=fill)
                if self.exchanger is not None
                else F.pad(x, (h,) * 4, value=fill)
            )
        else:
            xp = (
                halo_pad(x, h, self.exchanger, self.grad_mode, fill=fill)
                if h > 0
                else x
            )
        if self.kind == "max":
            if on_gpu and not self.d2:
                from .native import native_maxpool

                return native_maxpool(xp, k, s, 0)
            return F.max_pool2d(xp, k, s, padding=0)
        # avg: divisors from GLOBAL geometry when count_include_pad=False
        r, c = self.layout.pos(self.tile)
        Hg, Wg = H_loc * self.layout.rows, W_loc * self.layout.cols
        gr0, gc0 = r * H_loc - h, c * W_loc - h
        if on_gpu and not self.d2:
            from .native import native_avgpool

            return native_avgpool(
                xp, k, s, 0, gr0=gr0, gc0=gc0, Hg=Hg, Wg=Wg,
                include_pad=self.count_include_pad,
            )
        if self.count_include_pad or h == 0 or x.is_meta:
            return F.avg_pool2d(xp, k, s, padding=0, count_include_pad=True)
        return self._to_global_divisors(
            F.avg_pool2d(xp, k, s, padding=0, count_include_pad=True), H_loc, W_loc
        )
