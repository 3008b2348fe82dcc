"""Autograd wrappers over the gemscore CDNA4 kernels.

Each Function pairs a hand-written HIP forward with its hand-written
backward (no eager fallback on GPU — backend.py raises if the extension
is missing). CPU paths never reach these; the modules in
ops/spatial_conv.py and ops/norm.py dispatch here only for CUDA inputs.

BatchNormFn hands its parameter gradients to the gradient sink
(ops/grad_sink.py): where allowed, the backward kernel adds them into
``weight.grad`` / ``bias.grad`` itself and autograd gets None.
"""

from __future__ import annotations

import torch
import torch.distributed as dist

from . import backend
from .grad_sink import grad_sink


def _plane_dense(go):
    """go as the pool backward kernels take it: a channel slice of a
    contiguous NCHW tensor (dense planes and channels, any batch stride).
    Anything else is repacked."""
    if go.is_contiguous():
        return go
    _, _, oh, ow = go.shape
    st = go.stride()
    if st[3] == 1 and st[2] == ow and st[1] == oh * ow and st[0] >= 0:
        return go
    return go.contiguous()


class MaxPool2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        ge = backend.ext()
        x = x.contiguous()
        y, idx = ge.maxpool_fwd(x, k, s, p)
        ctx.save_for_backward(idx)
        ctx.geom = (x.shape[-2], x.shape[-1], k, s, p)
        return y

    @staticmethod
    def backward(ctx, go):
        (idx,) = ctx.saved_tensors
        H, W, k, s, p = ctx.geom
        gi = backend.ext().maxpool_bwd(_plane_dense(go), idx, H, W, k, s, p)
        return gi, None, None, None


def native_maxpool(x, k, s, p):
    return MaxPool2dFn.apply(x, k, s, p)


class AvgPool2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p, gr0, gc0, Hg, Wg, include_pad):
        ge = backend.ext()
        x = x.contiguous()
        y = ge.avgpool_fwd(x, k, s, p, gr0, gc0, Hg, Wg, include_pad)
        ctx.geom = (x.shape[-2], x.shape[-1], k, s, p, gr0, gc0, Hg, Wg, include_pad)
        return y

    @staticmethod
    def backward(ctx, go):
        H, W, k, s, p, gr0, gc0, Hg, Wg, include_pad = ctx.geom
        gi = backend.ext().avgpool_bwd(
            _plane_dense(go), H, W, k, s, p, gr0, gc0, Hg, Wg, include_pad
        )
        return (gi,) + (None,) * 8


def native_avgpool(x, k, s, p, gr0=None, gc0=None, Hg=None, Wg=None, include_pad=True):
    if gr0 is None:
        gr0, gc0 = -p, -p
        Hg, Wg = x.shape[-2], x.shape[-1]
    return AvgPool2dFn.apply(x, k, s, p, gr0, gc0, Hg, Wg, include_pad)


class BatchNormFn(torch.autograd.Function):
    """Fused (sync-capable) BatchNorm with optional ReLU.

    mean/invstd are precomputed constants (from bn_stats64 + optional
    group allreduce); backward implements the full sync-BN gradient:
    the gsum/gxsum reduction terms are allreduced over the tile group,
    weight/bias grads stay LOCAL (the engine's spatial-group SUM
    allreduce aggregates them with the other parameter grads).

    ``margin`` (top, bottom, left, right) != 0 says mean/invstd came from
    the region inside the margin only (n_global counts region pixels):
    the gsum/gxsum sums still run over every pixel, but their terms
    reach region pixels only (bn_bwd_apply_region).

    ``bwd_stats``: an fp64 [2C] buffer that holds zeros (bn_finalize
    zero-filled it for this forward); the first backward accumulates its
    statistics there instead of filling a fresh one.

    The parameter gradients are the fp32 cast of the LOCAL statistics.
    Block 0 of the bn_bwd_apply launch makes them: added in place into
    weight.grad / bias.grad where ``grad_sink`` allows (the Function then
    returns None for that parameter), else written to a fresh tensor that
    is returned. No cast kernel runs either way.
    """

    @staticmethod
    def forward(ctx, x, weight, bias, mean, invstd, group, n_global, training,
                relu, margin=(0, 0, 0, 0), bwd_stats=None):
        ge = backend.ext()
        x = x.contiguous()
        w32 = weight.detach().float().contiguous()
        b32 = bias.detach().float().contiguous()
        y = ge.bn_apply(x, mean, invstd, w32, b32, relu)
        ctx.save_for_backward(x, y, mean, invstd, w32)
        ctx.wdtype = weight.dtype
        ctx.group = group
        ctx.n_global = n_global
        ctx.training = training
        ctx.relu = relu
        ctx.margin = tuple(margin) if training else (0, 0, 0, 0)
        ctx.params = (weight, bias)  # the Parameters: backward asks grad_sink
        ctx.bwd_stats = bwd_stats    # zeroed; handed out once (backward)
        return y

    @staticmethod
    def backward(ctx, go):
        ge = backend.ext()
        x, y, mean, invstd, w32 = ctx.saved_tensors
        go = go.contiguous()
        C = x.shape[1]
        # the zeroed buffer serves one backward: after it the buffer is
        # dirty, and a second backward over a retained graph fills its own
        zeroed, ctx.bwd_stats = ctx.bwd_stats, None
        stats = ge.bn_bwd_stats(go, x, y, mean, invstd, ctx.relu,
                                out=zeroed)  # fp64 [gsum, gxsum], local
        gw_sink, gb_sink = (grad_sink(p) for p in ctx.params)
        pgrad = None
        if gw_sink is None or gb_sink is None:
            pgrad = torch.empty(2 * C, device=x.device, dtype=torch.float32)
        param_grads = dict(
            local=stats,
            gw=None if gw_sink is None else gw_sink.view(-1),
            gb=None if gb_sink is None else gb_sink.view(-1),
            pgrad=pgrad,
        )
        if ctx.training:
            if ctx.group is not None:
                g_global = stats.clone()
                dist.all_reduce(g_global, group=ctx.group)
            else:
                g_global = stats
            if any(ctx.margin):
                gi = ge.bn_bwd_apply_region(
                    go, x, y, mean, invstd, w32, g_global[:C], g_global[C:],
                    float(ctx.n_global), ctx.relu, list(ctx.margin),
                    **param_grads,
                )
            else:
                gi = ge.bn_bwd_apply(
                    go, x, y, mean, invstd, w32, g_global[:C], g_global[C:],
                    float(ctx.n_global), ctx.relu, **param_grads,
                )
        else:
            # eval: mean/var are constants -> gi = go_eff * w * invstd
            zeros = torch.zeros(2 * C, device=x.device, dtype=torch.float64)
            gi = ge.bn_bwd_apply(
                go, x, y, mean, invstd, w32, zeros[:C], zeros[C:],
                1.0, ctx.relu, **param_grads,
            )
        gw = None if gw_sink is not None else pgrad[C:].to(ctx.wdtype)
        gb = None if gb_sink is not None else pgrad[:C].to(ctx.wdtype)
        return (gi, gw, gb) + (None,) * 8


def native_batchnorm(x, weight, bias, mean, invstd, group, n_global, training,
                     relu=False, margin=(0, 0, 0, 0), bwd_stats=None):
    return BatchNormFn.apply(
        x, weight, bias, mean, invstd, group, n_global, training, relu, margin,
        bwd_stats,
    )
