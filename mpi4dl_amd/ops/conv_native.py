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

Per-shape, per-LEG policy (all crossovers measured on MI355X —
profiles/PERF_NOTES.md): stride-2 1x1s, K<=64 1x1s, stems, wide
1x7/7x1 and most weight-grads run on the hand-written kernels; the
fat stride-1 1x1 forward/data-grad legs that are plain library GEMMs
go to hipBLASLt (the brief's "libraries only for plain GEMMs" case;
MPI4DL_PW_BLASLT=0 restores all-native); everything else falls to
F.conv2d/MIOpen. MPI4DL_NATIVE_CONV=0 disables all native paths,
=1 forces them (A/B benchmarking).

The per-leg policy is written once, in ``conv_plan``: a pure function
of the problem's integers and the MPI4DL_PW_BLASLT switch. ``ConvFn``
executes the plan and decides nothing itself; which kernel a native
route then launches is the extension's choice (``conv_fwd_kernel_name``,
``pw_kernel_name``, ``pw_bwdw_kernel_name`` answer it for a plan's
problems).
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
    """

    route: str
    problem: tuple


class ConvPlan(NamedTuple):
    y: Leg
    gx: Leg
    gw: Leg


def conv_plan(N, C, K, H, W, R, S, sh, sw, ph, pw, blaslt=None):
    """The route of each leg of the convolution x[N,C,H,W] * w[K,C,R,S]
    and the problem that route hands to its binding. ``blaslt`` defaults
    to the MPI4DL_PW_BLASLT switch; nothing else is read."""
    if blaslt is None:
        blaslt = _blaslt_on()
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
    kept on ctx: backward does not read MPI4DL_PW_BLASLT again, so a
    change of the variable between a forward and its backward is
    ignored.

    Weight gradient: the routes that run our own kernels (pw_bwdw,
    pw_bwdw_sub, conv_bwd_weight) add it straight into ``w.grad`` when
    ``grad_sink(w)`` allows, and backward then returns None for ``w``;
    otherwise, and on the bmm route, it is returned for autograd to
    accumulate."""

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


class NativeConv2d(nn.Conv2d):
    """nn.Conv2d that runs on the gemscore implicit-GEMM MFMA kernels
    when dispatchable (state-dict compatible with nn.Conv2d)."""

    def forward(self, x):
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
