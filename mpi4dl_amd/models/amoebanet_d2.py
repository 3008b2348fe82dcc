"""AmoebaNet-D "Design 2" (fused halo) — one cell-level halo exchange
feeds all conv ops that read the same state.

Reference parity: src/models/amoebanet_d2.py (Cell_D2 :569-676 — it
pre-halos s3 = halo(s1, 3), s4 = halo(s2, 2), crops s5, and rewires the
op input indices; the _d2 op variants run with padding=0 :88-311).

The cell, the op bodies and the builder are those of models/amoebanet.py.
This module holds only what D2 changes: CellD2 is Cell with another op
factory and one step on an op's input (the fused exchange and its crop),
and a D2 op is make_op with three arguments replaced.

Our design keeps the same economics with exact semantics:
* for each input state consumed by stride-1 conv ops, ONE interior-side
  halo_pad_d2 with the max halo those ops need (3 when any 1x7/7x1 op
  reads it, else 1) replaces the per-op exchanges — e.g. the two
  conv_1x7_7x1 ops on state 0 of a normal cell share one exchange
  (4 messages -> 1);
* conv ops consume the surplus via outer-pad-only convs (HaloConv2d
  d2=True), so image-boundary behaviour stays exactly the serial conv;
* pools and stride-2 ops keep their D1 per-op exchange (pool divisor
  geometry under surplus is not worth the complexity — the reference's
  D2 pools silently change semantics instead);
* BNs that run on a tensor still carrying surplus (after the leading
  1x1 conv and after the 1x7) normalise every pixel but take their batch
  statistics from the nominal tile only (TileBatchNorm2d.stat_margin),
  so train mode computes the serial function too: forward, parameter
  gradients and running statistics match the undistributed model
  (tests/test_d2_exact.py).
"""

from __future__ import annotations

from typing import Optional

import torch.nn as nn

from ..ops.halo import exchanger_for, halo_pad_d2
from ..ops.plan import SpatialPlan
from ..ops.spatial_conv import HaloConv2d
from .amoebanet import (
    NORMAL_OPERATIONS,
    REDUCTION_OPERATIONS,
    Cell,
    build_amoebanetd,
    make_op,
)


def _op_halo_need(name: str) -> int:
    """Interior halo a stride-1 conv op consumes (0 = no exchange)."""
    if name == "conv_1x7_7x1":
        return 3
    if name == "conv_3x3":
        return 1
    return 0


def _d2_need(name, stride, ctx) -> int:
    """Halo that op ``name`` takes from its cell's fused exchange; 0 where
    the op is the D1 op (no tiles, stride 2, pools, 1x1)."""
    return _op_halo_need(name) if (ctx is not None and stride == 1) else 0


def _surplus(ctx, h):
    """(top, bottom, left, right) surplus a halo-h fused exchange leaves
    on THIS tile (HaloExchanger.pads_d2 semantics: interior sides get the
    halo, image-boundary sides 0; a single tile has none)."""
    ex = exchanger_for(**ctx) if ctx is not None else None
    return ex.pads_d2(h) if ex is not None else (0, 0, 0, 0)


def _d2conv(cin, cout, k, stride, padding, ctx):
    assert stride in (1, (1, 1)), "fused-halo convs are the stride-1 ones"
    # halo_len=(0,0): the CELL already exchanged the surplus; the conv
    # only applies fresh zero pads on image-boundary sides (outer_pad)
    return HaloConv2d(
        cin, cout, k, stride=1, padding=padding, bias=False, d2=True,
        halo_len=(0, 0), **ctx
    )


def _make_op_d2(name, c, stride, ctx, mknorm, ref_quirks=False):
    """conv ops in d2 mode (outer pads only); everything else D1.

    The BNs that run while the tensor still carries surplus pixels take
    their statistics from the nominal tile only (stat_margin): the
    surplus pixels are the neighbour's, which counts them itself."""
    need = _d2_need(name, stride, ctx)
    if not need:
        return make_op(name, c, stride, ctx, mknorm, ref_quirks=ref_quirks)
    t, b, l, r = _surplus(ctx, need)
    return make_op(
        name, c, stride, ctx, mknorm, ref_quirks=ref_quirks,
        # plain 1x1s where D1 has NativeConv2d: kept as found; whether D2
        # should follow D1 is a decision to take from a GPU measurement
        pw=nn.Conv2d,
        conv=_d2conv,
        # after the first k x k conv only the row surplus is left (1x7)
        margins=((t, b, l, r), (t, b, 0, 0)),
    )


class CellD2(Cell):
    """Cell with per-state fused halo exchange for its conv ops.

    Parameter layout matches amoebanet.Cell exactly (same ops in the
    same order)."""

    # Cell's fused glue (ops/fuse.py: state_fan, shared_relu) is off:
    # _op_input puts the fused halo exchange and its crops between a
    # state's ReLU and its ops, so a state's consumers are not the plain
    # aliases the fan hands out. The cell keeps a ReLU per reduction and
    # autograd's own gradient sums.
    uses_glue = False
    _make_op = staticmethod(_make_op_d2)

    def __init__(
        self,
        channels_prev_prev,
        channels_prev,
        channels,
        reduction,
        reduction_prev,
        ctx=None,
        mknorm=nn.BatchNorm2d,
        ref_quirks: bool = False,
    ):
        super().__init__(
            channels_prev_prev, channels_prev, channels, reduction,
            reduction_prev, ctx=ctx, mknorm=mknorm, ref_quirks=ref_quirks,
        )
        ops = REDUCTION_OPERATIONS if reduction else NORMAL_OPERATIONS
        # halo need per op (fused exchange only for stride-1 convs)
        self.op_need = [
            _d2_need(name, st, ctx) for (_, name), st in zip(ops, self.op_strides)
        ]
        # halo of a state's one exchange: the largest need among its ops
        self.state_need = {}
        for idx, need in zip(self.indices, self.op_need):
            self.state_need[idx] = max(need, self.state_need.get(idx, 0))
        self.grad_mode = (ctx or {}).get("grad_mode", "exact")
        self.exchanger = exchanger_for(**ctx) if ctx is not None else None

    def _op_input(self, pos, t, cache):
        need = self.op_need[pos]
        if not need or self.exchanger is None:
            return t
        idx = self.indices[pos]
        have = self.state_need[idx]
        if idx not in cache:
            cache[idx] = halo_pad_d2(t, have, self.exchanger, self.grad_mode)
        t = cache[idx]
        return self.exchanger.crop_d2(t, have - need) if have > need else t


def amoebanetd_d2(
    num_classes: int = 10,
    num_layers: int = 6,
    num_filters: int = 64,
    plan: Optional[SpatialPlan] = None,
    ref_quirks: bool = False,
) -> nn.Sequential:
    """D2 AmoebaNet-D; cell count/indices match amoebanet.amoebanetd
    (``ref_quirks`` as there)."""
    return build_amoebanetd(CellD2, num_classes, num_layers, num_filters,
                            plan, ref_quirks)
