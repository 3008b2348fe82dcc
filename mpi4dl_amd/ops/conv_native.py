"""NativeConv2d: hand-written gfx950 conv kernels behind an
nn.Conv2d-compatible module, with a fully MEASURED dispatch policy.

Kernel families (csrc/):
* conv_mfma.hip — implicit-GEMM MFMA conv (general R x S): forward,
  weight-grad; stride-1 data-grad = the forward kernel on C<->K
  transposed / 180-rotated weights; STRIDED data-grad = zero-stuffed
  transposed conv through the same stride-1 kernel.
* conv_pw.hip — the 1x1 family: the skinny streaming GEMM
  (pw_kernel), the fat one at a 128- or 256-square tile
  (pw_fat_kernel<4|8>), stride-2 gather + scatter backward-data, and
  the NT-GEMM bwd-weight with pixel-slab split-K at the same two
  tiles (pw_bwdw_kernel<4|8>).
* conv_wino.hip — fused Winograd F(2x2,3x3) for stride-1 3x3 (any pad in
  {0,1,2}, any N, C, K, H, W): filter transform to bf16 U, then one
  launch with the input transform, the 16 MFMA GEMMs and the output
  transform; its data-grad is the same kernel on the output gradient
  with the filter transform reading the forward weight transposed and
  rotated. Opt-in: MPI4DL_WINOGRAD=fused routes the forward and
  data-grad legs of every supported 3x3 there (weight-grad stays on
  conv_bwd_weight). The default dispatch does not use it yet.
* conv_tap.hip — tap-shift direct conv for stride-1 1x7, 7x1 and 3x3 (pads
  0..R-1 x 0..S-1, any N, C, K, H, W): a filter pre-pass to Wt[R*S][Kp][Cp],
  then one launch that stages each 32-channel input patch into LDS once,
  channel-innermost, and takes every tap as an address offset into it; its
  data-grad is the same kernel on the output gradient with the pre-pass
  reading the forward weight transposed and rotated. Opt-in:
  MPI4DL_TAPCONV=1 routes the forward and data-grad legs of every
  supported problem there (weight-grad stays on conv_bwd_weight; a 3x3
  stays on Winograd when MPI4DL_WINOGRAD=fused is set too). Measured
  (PERF_NOTES, "Tap-shift conv"): both legs beat MIOpen at the 512²,
  256² and 128² planes and lose at 64²; the switch as a whole is 0.89x
  end to end because of the weight-grad leg. The default dispatch does
  not use it. The third leg of the triple is tap_bwdw_kernel in the same
  file: go and x staged once per pixel tile, channel-innermost, MFMA k
  over pixels through transposing LDS reads, every tap an address offset
  into the x patch, fp32 atomicAdd into gw (so it feeds the gradient
  sink). Opt-in on top of the first switch: MPI4DL_TAPCONV_WGRAD=1 sends
  the weight-grad of every problem that MPI4DL_TAPCONV=1 routes to
  ge.tap_bwd_weight; alone it changes nothing (PERF_NOTES, "Tap-shift
  weight gradient"). MPI4DL_TAPCONV_WGRAD=ring sends it to
  ge.tap_bwd_weight_ring instead: tap_bwdw_ring_kernel, the same GEMM on a
  32 x 64 (or 32 x 32) channel tile, a block walking a strip of output
  rows with the x rows in an LDS ring, so a step stages only its new rows,
  two steps ahead, and two blocks fit a CU (PERF_NOTES, "Tap-shift weight
  gradient, rolling window"). MPI4DL_TAPCONV_WGRAD=px sends it to
  ge.tap_bwd_weight_px: tap_bwdw_px_kernel, which stages go and x as they
  lie in memory, pixel-innermost (a 16-byte copy, no transpose in or out
  of LDS), on a 128 x 32 channel tile, and takes the column taps as
  register shifts of a 24-pixel window (PERF_NOTES, "Tap-shift weight
  gradient, pixel-major"). MPI4DL_TAPCONV_SPLIT=auto, also on top of the
  first switch, runs the forward and data-grad legs as
  ge.tap_fwd(split=-1): where the grid of a problem is under two blocks a
  CU, tap_fwd_split_kernel deals the 32-channel chunks to up to 8 slices
  of blocks that leave fp32 partial sums in a workspace, and
  tap_split_reduce_kernel adds them in slice order, with the bias, and
  rounds once; elsewhere it is the unsplit kernel (PERF_NOTES, "Tap-shift
  conv, split channels"). MPI4DL_TAPCONV_STRIDED=1, also on top of the
  first switch, routes the strided problems of the same three filter
  shapes (1x7 at stride (1, 2), 7x1 at (2, 1), 3x3 at (2, 2): AmoebaNet's
  reduction cells and the head of every ResNet stage) to
  ge.tap_fwd_strided and ge.tap_bwd_data_strided:
  tap_strided_fwd_kernel stages the input patch in phase planes (column
  lc in plane lc % sw), so a tap of 16 output columns is again one
  contiguous run of LDS pixels, and tap_strided_bwd_data_kernel computes
  the data gradient by phase decomposition, every tap class of the filter
  against one staged patch of go: no zero-stuffed copy and none of its
  multiply-adds by zero. The weight-grad stays on conv_bwd_weight
  (PERF_NOTES, "Tap-shift conv, strided").

Per-shape, per-LEG policy (all crossovers measured on MI355X —
profiles/PERF_NOTES.md): stride-2 1x1s, K<=64 1x1s, stems, wide
1x7/7x1 and most weight-grads run on the hand-written kernels; the
fat stride-1 1x1 forward/data-grad legs that are plain library GEMMs
go to hipBLASLt (the brief's "libraries only for plain GEMMs" case;
MPI4DL_PW_BLASLT=0 restores all-native); everything else falls to
F.conv2d/MIOpen. MPI4DL_NATIVE_CONV=0 disables all native paths,
=1 forces them (A/B benchmarking).

The per-leg policy is written once, in ``conv_plan``: a pure function
of the problem's integers and the MPI4DL_PW_BLASLT,
MPI4DL_WINOGRAD=fused, MPI4DL_TAPCONV=1, MPI4DL_TAPCONV_WGRAD=1|ring|px,
MPI4DL_TAPCONV_SPLIT=auto and MPI4DL_TAPCONV_STRIDED=1 switches.
``ConvFn`` executes the plan and decides nothing itself; which kernel a native route then launches is the
extension's choice
(``conv_fwd_kernel_name``, ``pw_kernel_name``, ``pw_bwdw_kernel_name``,
``wino_kernel_name``, ``tap_kernel_name``, ``tap_split_kernel_name``,
``tap_bwdw_kernel_name``,
``tap_bwdw_ring_kernel_name``, ``tap_bwdw_px_kernel_name``,
``tap_strided_kernel_name`` answer it for a plan's problems).
"""

from __future__ import annotations

import os
from typing import NamedTuple

import torch
import torch.nn as nn

from . import backend
from .grad_sink import grad_sink

_MIN_OW = 64
_ONE_D_MIN_OW = 384


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _pw_geom_ok(H, W, sh, sw):
    """pw kernel constraints: per-image output pixels % 128 == 0; at
    stride 2 additionally even dims and OW % 8 (vector evens loads)."""
    oh = (H - 1) // sh + 1
    ow = (W - 1) // sw + 1
    if (oh * ow) % 128 != 0:
        return False
    if (sh, sw) != (1, 1):
        return (
            sh == 2 and sw == 2 and H % 2 == 0 and W % 2 == 0 and ow % 8 == 0
        )
    return True


def _blaslt_on():
    return os.environ.get("MPI4DL_PW_BLASLT", "1") != "0"


def _wino_fused_on():
    return os.environ.get("MPI4DL_WINOGRAD", "0") == "fused"


def _wino_ok(H, W, R, S, sh, sw, ph, pw):
    """What conv_wino.hip serves: 3x3, stride 1, pads in {0, 1, 2}, at
    least one output pixel (dilation 1 and groups 1 are the caller's)."""
    return (
        (R, S, sh, sw) == (3, 3, 1, 1) and ph in (0, 1, 2) and pw in (0, 1, 2)
        and H + 2 * ph >= 3 and W + 2 * pw >= 3
    )


def _tap_on():
    return os.environ.get("MPI4DL_TAPCONV", "0") == "1"


def _tap_wgrad_mode():
    """MPI4DL_TAPCONV_WGRAD as conv_plan's ``tap_wgrad``: True for "1",
    "ring" for "ring", "px" for "px", False for anything else."""
    v = os.environ.get("MPI4DL_TAPCONV_WGRAD", "0")
    return v if v in ("ring", "px") else v == "1"


def _tap_split_on():
    return os.environ.get("MPI4DL_TAPCONV_SPLIT", "0") == "auto"


def _tap_strided_on():
    return os.environ.get("MPI4DL_TAPCONV_STRIDED", "0") == "1"


def _tap_strided_ok(H, W, R, S, sh, sw, ph, pw):
    """What conv_tap.hip's strided kernels serve: 1x7 at stride (1, 2), 7x1
    at (2, 1) or 3x3 at (2, 2), pads in [0, R-1] x [0, S-1], at least one
    output pixel (dilation 1 and groups 1 are the caller's)."""
    return (
        (R, S, sh, sw) in ((1, 7, 1, 2), (7, 1, 2, 1), (3, 3, 2, 2))
        and 0 <= ph <= R - 1 and 0 <= pw <= S - 1
        and H + 2 * ph >= R and W + 2 * pw >= S
    )


def _tap_ok(H, W, R, S, sh, sw, ph, pw):
    """What conv_tap.hip serves: 1x7, 7x1 or 3x3, stride 1, pads in
    [0, R-1] x [0, S-1], at least one output pixel (dilation 1 and groups
    1 are the caller's)."""
    return (
        (R, S) in ((1, 7), (7, 1), (3, 3)) and (sh, sw) == (1, 1)
        and 0 <= ph <= R - 1 and 0 <= pw <= S - 1
        and H + 2 * ph >= R and W + 2 * pw >= S
    )


class Leg(NamedTuple):
    """How one of y, gx, gw is computed.

    ``route`` is one of
      matmul, bmm            hipBLASLt; problem = (rows, reduction, OHW)
      pw_fwd                 ge.pw_fwd; problem = pw_kernel_name's
      pw_bwd_data_strided    (C, K, OHW, sw, osw): C the reduction dim
                             and K the output channels of the launch
      pw_bwdw, pw_bwdw_sub   ge.pw_bwdw, _sub on x[:, :, ::sh, ::sw];
                             problem = pw_bwdw_kernel_name's (N, K, C, OHW)
      conv_fwd, conv_fwd_zs  ge.conv_fwd, _zs on the zero-stuffed
                             gradient; problem = conv_fwd_kernel_name's
                             (C, K, H, W, R, S, sh, sw, ph, pw)
      conv_bwd_weight        ge.conv_bwd_weight; problem = the forward
                             convolution's, as for conv_fwd
      wino_fwd               ge.wino_fwd (for gx: transposed, on the output
                             gradient); problem = wino_kernel_name's
                             (C, K, H, W, ph, pw): C the reduction dim and
                             K the output channels of the launch
      tap_fwd                ge.tap_fwd (for gx: transposed, on the output
                             gradient); problem = tap_kernel_name's
                             (C, K, H, W, R, S, ph, pw), C and K as for
                             wino_fwd
      tap_fwd_split          ge.tap_fwd(split=-1) (for gx: transposed, on the
                             output gradient); problem =
                             tap_split_kernel_name's (N, C, K, H, W, R, S,
                             ph, pw) without the CU count, C and K as for
                             wino_fwd
      tap_bwd_weight         ge.tap_bwd_weight; problem =
                             tap_bwdw_kernel_name's (N, C, K, H, W, R, S,
                             ph, pw), the forward convolution's
      tap_bwd_weight_ring    ge.tap_bwd_weight_ring; problem =
                             tap_bwdw_ring_kernel_name's, the same nine
      tap_bwd_weight_px      ge.tap_bwd_weight_px; problem =
                             tap_bwdw_px_kernel_name's, the same nine
      tap_fwd_strided        ge.tap_fwd_strided; problem =
                             tap_strided_kernel_name's
                             (C, K, H, W, R, S, sh, sw, ph, pw)
      tap_bwd_data_strided   ge.tap_bwd_data_strided; problem = (K, C, OH, OW,
                             H, W, R, S, sh, sw, ph, pw): K the reduction dim
                             and C the output channels of the launch, OH x OW
                             the extents of go, the rest the forward's
    """

    route: str
    problem: tuple


class ConvPlan(NamedTuple):
    y: Leg
    gx: Leg
    gw: Leg


def conv_plan(N, C, K, H, W, R, S, sh, sw, ph, pw, blaslt=None,
              winograd=None, tap=None, tap_wgrad=None, tap_split=None,
              tap_strided=None):
    """The route of each leg of the convolution x[N,C,H,W] * w[K,C,R,S]
    and the problem that route hands to its binding. ``blaslt`` defaults
    to the MPI4DL_PW_BLASLT switch, ``winograd`` to
    MPI4DL_WINOGRAD == "fused", ``tap`` to MPI4DL_TAPCONV == "1" and
    ``tap_wgrad`` (looked at only where ``tap`` routes the problem; True,
    False, "ring" or "px") to MPI4DL_TAPCONV_WGRAD == "1", "ring" or "px"
    and ``tap_split`` (looked at only where ``tap`` routes the problem) to
    MPI4DL_TAPCONV_SPLIT == "auto" and ``tap_strided`` (looked at only where
    ``tap`` is on) to MPI4DL_TAPCONV_STRIDED == "1"; nothing else is read."""
    if blaslt is None:
        blaslt = _blaslt_on()
    if winograd is None:
        winograd = _wino_fused_on()
    if tap is None:
        tap = _tap_on()
    OH = (H + 2 * ph - R) // sh + 1
    OW = (W + 2 * pw - S) // sw + 1
    ohw = OH * OW
    if R == 1 and S == 1 and ph == 0 and pw == 0 and _pw_geom_ok(H, W, sh, sw):
        if (sh, sw) != (1, 1):
            # strided 1x1 (FactorizedReduce): gather forward, scatter
            # data-grad; only the strided input pixels contribute to gw —
            # subsample once, then the fast NT GEMM (the general bwdw
            # kernel averaged ~870us on these shapes)
            return ConvPlan(
                Leg("pw_fwd", (C, K, ohw, sw, 1)),
                Leg("pw_bwd_data_strided", (K, C, ohw, 1, sw)),
                Leg("pw_bwdw_sub", (N, K, C, ohw)),
            )
        # Stride-1 1x1s ARE plain GEMMs; hipBLASLt measured 1.05-1.6x
        # our kernels on nearly every s1 shape EXCEPT K<=64 (where ours
        # wins 1.1-1.3x) — gpurun_out/matmul_ab2.log. The brief's
        # "libraries for plain library GEMMs" case. Our kernels keep
        # every shape where THEY win: stride-2 (2-7x), K<=64, most
        # bwd-weight shapes, stem/1x7/7x1, pools, BN, halo, SGD.
        y = (Leg("matmul", (K, C, ohw)) if blaslt and K > 64
             else Leg("pw_fwd", (C, K, ohw, 1, 1)))
        # gx is the mirror GEMM (C<->K): same library-vs-native
        # crossover as forward (output channels = C here)
        gx = (Leg("matmul", (C, K, ohw)) if blaslt and C > 64
              else Leg("pw_fwd", (K, C, ohw, 1, 1)))
        # big C*K output tiles over small P: the bmm-and-sum through
        # hipBLASLt wins (1.3-1.7x); everywhere else our NT GEMM
        # wins up to 3.5x (gpurun_out/matmul_ab2.log)
        gw = (Leg("bmm", (K, C, ohw))
              if blaslt and C * K >= 350_000 and ohw <= 32_768
              else Leg("pw_bwdw", (N, K, C, ohw)))
        return ConvPlan(y, gx, gw)
    fwd = (C, K, H, W, R, S, sh, sw, ph, pw)
    if winograd and _wino_ok(H, W, R, S, sh, sw, ph, pw):
        # opt-in fused Winograd: forward, and the data-grad as the same
        # kernel on go with pads 2-p; the weight-grad keeps its kernel
        return ConvPlan(
            Leg("wino_fwd", (C, K, H, W, ph, pw)),
            Leg("wino_fwd", (K, C, OH, OW, 2 - ph, 2 - pw)),
            Leg("conv_bwd_weight", fwd),
        )
    if tap and _tap_ok(H, W, R, S, sh, sw, ph, pw):
        # opt-in tap-shift kernel: forward, and the data-grad as the same
        # kernel on go with the complementary pads; the weight-grad keeps
        # its kernel unless the second switch sends it to tap_bwd_weight
        # or, as "ring" or "px", to tap_bwd_weight_ring or tap_bwd_weight_px
        if tap_wgrad is None:
            tap_wgrad = _tap_wgrad_mode()
        if tap_wgrad not in (True, False, "ring", "px"):
            raise ValueError(f"tap_wgrad must be a bool, 'ring' or 'px', "
                             f"got {tap_wgrad!r}")
        if tap_split is None:
            tap_split = _tap_split_on()
        tapw = (N, C, K, H, W, R, S, ph, pw)
        tapx = (K, C, OH, OW, R, S, R - 1 - ph, S - 1 - pw)
        return ConvPlan(
            # the third switch lets the extension split the channels of
            # both legs where their grids under-fill the device
            (Leg("tap_fwd_split", tapw) if tap_split
             else Leg("tap_fwd", tapw[1:])),
            (Leg("tap_fwd_split", (N,) + tapx) if tap_split
             else Leg("tap_fwd", tapx)),
            (Leg("tap_bwd_weight_ring", tapw) if tap_wgrad == "ring"
             else Leg("tap_bwd_weight_px", tapw) if tap_wgrad == "px"
             else Leg("tap_bwd_weight", tapw) if tap_wgrad
             else Leg("conv_bwd_weight", fwd)),
        )
    if tap and _tap_strided_ok(H, W, R, S, sh, sw, ph, pw):
        if tap_strided is None:
            tap_strided = _tap_strided_on()
        if tap_strided:
            # opt-in strided tap-shift kernels: the forward on a phase-split
            # patch, the data-grad by phase decomposition of go; the
            # weight-grad keeps its kernel, which is strided already
            return ConvPlan(
                Leg("tap_fwd_strided", fwd),
                Leg("tap_bwd_data_strided",
                    (K, C, OH, OW, H, W, R, S, sh, sw, ph, pw)),
                Leg("conv_bwd_weight", fwd),
            )
    if (sh, sw) == (1, 1):
        # stride-1 data-grad = the forward kernel on C<->K transposed,
        # 180-rotated weights
        gx = Leg("conv_fwd", (K, C, OH, OW, R, S, 1, 1, R - 1 - ph, S - 1 - pw))
    else:
        # strided data-grad = transposed conv: zero-stuff go to the
        # stride-1 grid (+output padding), then our stride-1 kernel
        # with flipped/transposed weights (VERDICT r1 item 9 — the
        # conv triple fully in-house)
        hs = (OH - 1) * sh + 1 + (H + 2 * ph - R) % sh
        ws = (OW - 1) * sw + 1 + (W + 2 * pw - S) % sw
        gx = Leg("conv_fwd_zs",
                 (K, C, hs, ws, R, S, 1, 1, R - 1 - ph, S - 1 - pw))
    return ConvPlan(Leg("conv_fwd", fwd), gx, Leg("conv_bwd_weight", fwd))


class ConvFn(torch.autograd.Function):
    """Executes ``conv_plan``. The plan is made once, in forward, and
    kept on ctx: backward reads none of MPI4DL_PW_BLASLT,
    MPI4DL_WINOGRAD, MPI4DL_TAPCONV, MPI4DL_TAPCONV_WGRAD,
    MPI4DL_TAPCONV_SPLIT and MPI4DL_TAPCONV_STRIDED again, so a change of
    a variable between a forward and its backward is ignored.

    Weight gradient: the routes that run our own kernels (pw_bwdw,
    pw_bwdw_sub, conv_bwd_weight, tap_bwd_weight, tap_bwd_weight_ring,
    tap_bwd_weight_px) add it straight into ``w.grad`` when ``grad_sink(w)``
    allows, and backward then returns None for ``w``; otherwise, and on the bmm route, it is
    returned for autograd to accumulate."""

    @staticmethod
    def forward(ctx, x, w, bias, sh, sw, ph, pw):
        ge = backend.ext()
        xb = x.contiguous().to(torch.bfloat16)
        wb = w.contiguous().to(torch.bfloat16)
        K, C, R, S = wb.shape
        N, _, H, W = xb.shape
        plan = conv_plan(N, C, K, H, W, R, S, sh, sw, ph, pw)
        if plan.y.route == "matmul":
            y = torch.matmul(wb.view(K, C), xb.view(N, C, H * W))
            if bias is not None:
                y += bias.to(y.dtype).view(1, K, 1)
            y = y.view(N, K, H, W)
        elif plan.y.route == "pw_fwd":
            y = ge.pw_fwd(xb, wb, bias, sh, sw)
        elif plan.y.route == "wino_fwd":
            y = ge.wino_fwd(xb, wb, bias, ph, pw)
        elif plan.y.route == "tap_fwd":
            y = ge.tap_fwd(xb, wb, bias, ph, pw)
        elif plan.y.route == "tap_fwd_split":
            y = ge.tap_fwd(xb, wb, bias, ph, pw, split=-1)
        elif plan.y.route == "tap_fwd_strided":
            y = ge.tap_fwd_strided(xb, wb, bias, sh, sw, ph, pw)
        else:
            y = ge.conv_fwd(xb, wb, bias, sh, sw, ph, pw)
        ctx.save_for_backward(xb, wb)
        ctx.geom = (sh, sw, ph, pw)
        ctx.wdtype = w.dtype
        ctx.has_bias = bias is not None
        ctx.plan = plan
        ctx.wparam = w  # the Parameter itself: backward asks grad_sink(w)
        return y

    @staticmethod
    def backward(ctx, go):
        ge = backend.ext()
        xb, wb = ctx.saved_tensors
        sh, sw, ph, pw = ctx.geom
        go = go.contiguous().to(torch.bfloat16)
        K, C, R, S = wb.shape
        N, _, H, W = xb.shape
        gw_route, gx_route = ctx.plan.gw.route, ctx.plan.gx.route
        if gw_route == "bmm":
            ohw = H * W
            gw = (
                torch.bmm(go.view(N, K, ohw),
                          xb.view(N, C, ohw).transpose(1, 2))
                .float().sum(dim=0).view(K, C, 1, 1).to(ctx.wdtype)
            )
        else:
            # our kernels finish with atomicAdd: with a sink they add into
            # p.grad itself (no zero fill, no AccumulateGrad add) and the
            # weight's gradient is returned as None
            sink = grad_sink(ctx.wparam)
            out = () if sink is None else (sink,)
            if gw_route == "conv_bwd_weight":
                gw = ge.conv_bwd_weight(go, xb, R, S, sh, sw, ph, pw, *out)
            elif gw_route == "tap_bwd_weight":
                gw = ge.tap_bwd_weight(go, xb, R, S, ph, pw, *out)
            elif gw_route == "tap_bwd_weight_ring":
                gw = ge.tap_bwd_weight_ring(go, xb, R, S, ph, pw, *out)
            elif gw_route == "tap_bwd_weight_px":
                gw = ge.tap_bwd_weight_px(go, xb, R, S, ph, pw, *out)
            else:
                xs = (xb if gw_route == "pw_bwdw"
                      else xb[:, :, ::sh, ::sw].contiguous())
                gw = ge.pw_bwdw(go, xs, *out)
            gw = None if sink is not None else (
                gw.view(K, C, R, S).to(ctx.wdtype))
        gb = go.sum(dim=(0, 2, 3)).to(ctx.wdtype) if ctx.has_bias else None
        if not ctx.needs_input_grad[0]:
            # first layer: the input is data — skip the whole gx leg
            # (the zero-stuffed stem data-grad alone was ~1.5% of the
            # r2 timed window before this gate)
            gx = None
        elif gx_route == "matmul":
            gx = torch.matmul(
                wb.view(K, C).t(), go.view(N, K, H * W)
            ).view(N, C, H, W).contiguous()
        elif gx_route == "pw_fwd":
            wt = wb.view(K, C).t().contiguous()
            gx = ge.pw_fwd(go, wt, None, 1, 1)
        elif gx_route == "pw_bwd_data_strided":
            wt = wb.view(K, C).t().contiguous()
            gx = ge.pw_bwd_data_strided(go, wt, H, W, sh, sw)
        elif gx_route == "wino_fwd":
            # the filter transform reads wb transposed and rotated itself
            gx = ge.wino_fwd(go, wb, None, 2 - ph, 2 - pw, True)
        elif gx_route == "tap_fwd":
            # the filter pre-pass reads wb transposed and rotated itself
            gx = ge.tap_fwd(go, wb, None, R - 1 - ph, S - 1 - pw, True)
        elif gx_route == "tap_fwd_split":
            gx = ge.tap_fwd(go, wb, None, R - 1 - ph, S - 1 - pw, True,
                            split=-1)
        elif gx_route == "tap_bwd_data_strided":
            # the filter pre-pass reads wb transposed and rotated itself
            gx = ge.tap_bwd_data_strided(go, wb, H, W, sh, sw, ph, pw)
        else:
            # conv_fwd on go, or on go zero-stuffed to the plan's extents
            _, _, hs, ws, _, _, _, _, tph, tpw = ctx.plan.gx.problem
            src = go
            if gx_route == "conv_fwd_zs":
                src = torch.zeros(N, K, hs, ws, device=go.device,
                                  dtype=go.dtype)
                src[:, :, ::sh, ::sw] = go
            wt = wb.transpose(0, 1).flip(2, 3).contiguous()
            gx = ge.conv_fwd(src, wt, None, 1, 1, tph, tpw)
        return gx, gw, gb, None, None, None, None


def native_conv2d(x, w, bias, stride, padding):
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    b32 = bias.float().contiguous() if bias is not None else None
    return ConvFn.apply(x, w, b32, sh, sw, ph, pw)


def _dispatchable(x, conv: nn.Conv2d) -> bool:
    mode = os.environ.get("MPI4DL_NATIVE_CONV", "auto")
    if mode == "0":
        return False
    if not (x.is_cuda and not x.is_meta):
        return False
    if conv.groups != 1 or _pair(conv.dilation) != (1, 1):
        return False
    bf16_ok = x.dtype == torch.bfloat16 or torch.is_autocast_enabled()
    if not bf16_ok:
        return False
    if mode == "1":
        return True
    sh, sw = _pair(conv.stride)
    ph, pw = _pair(conv.padding)
    kh, kw = _pair(conv.kernel_size)
    # 1x1: the conv_pw streaming GEMM (round 2) — pixel axis spans rows,
    # so no OW minimum; all three legs native
    if (
        kh == 1 and kw == 1 and ph == 0 and pw == 0
        and _pw_geom_ok(x.shape[-2], x.shape[-1], sh, sw)
    ):
        return True
    ow = (x.shape[-1] + 2 * pw - kw) // sw + 1
    if ow < _MIN_OW:
        return False
    # measured policy (profiles/r01_conv_microbench.txt): the implicit-GEMM
    # kernel beats hipBLASLt on degenerate small-C stems (im2col-dominated)
    # and matches it on wide 1x7/7x1 rows (AmoebaNet's hot convs, 1.03x /
    # 0.98x at 512^2); square 3x3+ shapes stay on the vendor GEMM until the
    # staging pipeline lands (round 2).
    if x.shape[1] <= 8:
        return True
    one_d = (kh == 1 and kw >= 7) or (kw == 1 and kh >= 7)
    return one_d and ow >= _ONE_D_MIN_OW and x.shape[1] <= 256


def _wino_dispatchable(x, conv: nn.Conv2d) -> bool:
    """MPI4DL_WINOGRAD=fused: a supported 3x3 on a CUDA tensor, under
    the bf16/autocast condition of ``_dispatchable``."""
    if not _wino_fused_on():
        return False
    if not (x.is_cuda and not x.is_meta) or x.dim() != 4:
        return False
    if conv.groups != 1 or _pair(conv.dilation) != (1, 1):
        return False
    if not (x.dtype == torch.bfloat16 or torch.is_autocast_enabled()):
        return False
    if isinstance(conv.padding, str) or conv.padding_mode != "zeros":
        return False
    return _wino_ok(x.shape[-2], x.shape[-1], *_pair(conv.kernel_size),
                    *_pair(conv.stride), *_pair(conv.padding))


def _tap_dispatchable(x, conv: nn.Conv2d) -> bool:
    """MPI4DL_TAPCONV=1: a supported 1x7, 7x1 or 3x3 on a CUDA tensor,
    under the bf16/autocast condition of ``_dispatchable``; with
    MPI4DL_TAPCONV_STRIDED=1 as well, also their strided problems."""
    if not _tap_on():
        return False
    if not (x.is_cuda and not x.is_meta) or x.dim() != 4:
        return False
    if conv.groups != 1 or _pair(conv.dilation) != (1, 1):
        return False
    if not (x.dtype == torch.bfloat16 or torch.is_autocast_enabled()):
        return False
    if isinstance(conv.padding, str) or conv.padding_mode != "zeros":
        return False
    geom = (x.shape[-2], x.shape[-1], *_pair(conv.kernel_size),
            *_pair(conv.stride), *_pair(conv.padding))
    return _tap_ok(*geom) or (_tap_strided_on() and _tap_strided_ok(*geom))


class NativeConv2d(nn.Conv2d):
    """nn.Conv2d that runs on the gemscore implicit-GEMM MFMA kernels
    when dispatchable (state-dict compatible with nn.Conv2d)."""

    def forward(self, x):
        if _wino_dispatchable(x, self) or _tap_dispatchable(x, self):
            return native_conv2d(x, self.weight, self.bias, self.stride, self.padding)
        if (
            os.environ.get("MPI4DL_WINOGRAD", "0") == "1"
            and self.kernel_size == (3, 3)
            and self.stride in ((1, 1), 1)
            and self.dilation in ((1, 1), 1)
            and self.groups == 1
            and not x.is_meta
        ):
            # round-2 staging: F(2x2,3x3) via batched hipBLASLt GEMM
            # (2.25x FLOP reduction; A/B against MIOpen with one env var)
            from .winograd_ref import filter_transform, winograd_bmm_conv2d

            pad = self.padding if isinstance(self.padding, int) else self.padding[0]
            return winograd_bmm_conv2d(
                x, filter_transform(self.weight), self.bias, padding=pad,
                out_dtype=x.dtype,
            )
        if _dispatchable(x, self):
            return native_conv2d(x, self.weight, self.bias, self.stride, self.padding)
        return super().forward(x)
