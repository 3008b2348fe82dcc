"""Gradient sink: let a backward kernel add a weight gradient straight
into ``param.grad`` (gradient-accumulation fusion).

``comm.FlatGrads`` makes every ``p.grad`` a persistent view of one flat
fp32 buffer. A hand-written backward kernel that already accumulates
(the conv weight-gradient kernels finish with atomicAdd; the BN backward
reads the sums it casts) can therefore target that view directly: no
zero fill of a scratch tensor, no cast, and no AccumulateGrad add per
parameter. The Function then returns ``None`` for that input, so autograd
runs nothing for it.

``grad_sink(param)`` decides, per backward call, whether that is allowed.
Anything that depends on AccumulateGrad running (hooks), on the gradient
being a graph value (create_graph), or on the gradient NOT reaching
``.grad`` (``torch.autograd.grad``, ``backward(inputs=...)`` without the
parameter) gets ``None`` and keeps the returned-tensor path.
"""

from __future__ import annotations

import torch
from torch.autograd.graph import get_gradient_edge

from . import backend

_FLAG = "_mpi4dl_grad_sink"


def opt_in(param: torch.Tensor) -> None:
    """Allow backward kernels to accumulate into ``param.grad`` in place.
    Called by the owner of a persistent gradient buffer (FlatGrads)."""
    setattr(param, _FLAG, True)


def opt_out(param: torch.Tensor) -> None:
    if getattr(param, _FLAG, False):
        delattr(param, _FLAG)


def _engine_accumulates(param) -> bool:
    """Inside a backward pass: will this pass accumulate into param.grad?
    False under torch.autograd.grad and backward(inputs=...) that leave the
    parameter out. Outside any backward pass there is nothing to ask."""
    if torch._C._current_graph_task_id() == -1:
        return True
    try:
        return torch._C._will_engine_execute_node(get_gradient_edge(param).node)
    except RuntimeError:
        # autograd.grad with the parameter among its inputs: the gradient
        # is captured and returned, never accumulated
        return False


def grad_sink(param):
    """``param.grad`` if a backward kernel may add into it, else ``None``."""
    if not getattr(param, _FLAG, False) or not backend.grad_sink_enabled():
        return None
    g = param.grad
    if (
        g is None
        or g.dtype != torch.float32
        or g.device != param.device
        or g.shape != param.shape
        or not g.is_contiguous()
    ):
        return None
    if param._backward_hooks or param._post_accumulate_grad_hooks:
        return None  # these run with AccumulateGrad, which the sink skips
    if torch.is_grad_enabled():
        return None  # create_graph: the gradient must stay a graph value
    if not param.requires_grad or not _engine_accumulates(param):
        return None
    return g
