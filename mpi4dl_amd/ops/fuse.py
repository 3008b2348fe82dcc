"""Fused elementwise glue for the AmoebaNet cell epilogue.

Reference behaviour replaced: the cell's per-pair sums and final
concat (/root/reference/src/models/amoebanet.py:449-533, Cell.forward's
``torch.cat(states[...])``). The reference (and round-1) cell does
``states.append(h1 + h2)`` per genotype pair and then
``torch.cat([states[i] for i in concat], 1)`` —
at 2048^2 that cat alone re-reads and re-writes the whole cell output
(~9% of the step was such eager glue in profiles/r01_*). AddCat writes
each concat slice ONCE: sum slices compute ``h1 + h2`` directly into
their channel range of the output buffer, passthrough slices copy.
Backward is free: every input's gradient is a channel-narrow VIEW of
the incoming gradient (no kernels).

Works on CPU and GPU (torch.add into a strided out); autograd-correct
including states that feed both the concat and later ops (grad
contributions accumulate via the normal autograd sum).
"""

from __future__ import annotations

import contextlib
import weakref
from typing import List, Optional, Tuple

import torch

from . import backend
from .native import _plane_dense

_SENTINEL = None


class _AddCatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, *tensors):
        # spec: list of (a_idx, b_idx_or_-1, channels)
        first = tensors[0]
        n, _, h, w = first.shape
        ctot = sum(c for _, _, c in spec)
        dtype = tensors[0].dtype
        for t in tensors:
            dtype = torch.promote_types(dtype, t.dtype)
        out = torch.empty(n, ctot, h, w, device=first.device, dtype=dtype)
        off = 0
        for a_i, b_i, c in spec:
            sl = out.narrow(1, off, c)
            a = tensors[a_i]
            if b_i < 0:
                sl.copy_(a)
            else:
                torch.add(a, tensors[b_i], out=sl)
            off += c
        ctx.spec = spec
        ctx.n_inputs = len(tensors)
        return out

    @staticmethod
    def backward(ctx, go):
        grads: List[Optional[torch.Tensor]] = [None] * ctx.n_inputs
        off = 0
        for a_i, b_i, c in ctx.spec:
            g = go.narrow(1, off, c)
            grads[a_i] = g if grads[a_i] is None else grads[a_i] + g
            if b_i >= 0:
                grads[b_i] = g if grads[b_i] is None else grads[b_i] + g
            off += c
        return (None, *grads)


glue_enabled = backend.cell_glue_enabled


# ---------------------------------------------------------------------------
# State fan: one autograd node for a state with several consumers
# ---------------------------------------------------------------------------

def _fold_torch(raw, rel, r, slot):
    m = None
    for t in rel:
        m = t if m is None else m + t
    if m is not None:
        m = torch.ops.aten.threshold_backward(m, r, 0)
    acc = None
    for k in range(len(raw) + 1):
        if m is not None and k == slot:
            acc = m if acc is None else acc + m
        if k < len(raw):
            acc = raw[k] if acc is None else acc + raw[k]
    return acc


def fan_fold(raw, rel, r, slot):
    """g = fold(raw[:slot], select(r <= 0, 0, fold(rel)), raw[slot:]) with
    every partial sum rounded to the tensors' dtype (a left fold of torch
    adds). On the GPU one gemscore kernel reads every term once."""
    first = raw[0] if raw else rel[0]
    if not rel and len(raw) == 1:
        return first
    terms = list(raw) + list(rel)
    if not first.is_cuda:
        return _fold_torch(raw, rel, r, slot)
    ge = backend.ext()
    if (
        first.dim() != 4
        or len(raw) > ge.FAN_MAX  # terms of a kind the kernel takes
        or len(rel) > ge.FAN_MAX
        or any(t.dtype != first.dtype or t.shape != first.shape for t in terms)
        or (rel and r.dtype != first.dtype)
    ):
        return _fold_torch(raw, rel, r, slot)
    return ge.fan_bwd(
        [_plane_dense(t) for t in raw],
        [_plane_dense(t) for t in rel],
        r.contiguous() if rel else None,
        slot,
    )


class _StateFanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, kinds):
        r = torch.relu(y) if any(kinds) else None
        ctx.kinds = kinds
        ctx.set_materialize_grads(False)  # an unused alias arrives as None
        if r is not None:
            ctx.save_for_backward(r)
        outs = []
        for k in kinds:
            src = r if k else y
            outs.append(src.view_as(src))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        kinds = ctx.kinds
        # unfused, every consumer is a node of its own, and the engine runs
        # them latest-created first: the gradients arrive in reverse order
        live = [i for i in reversed(range(len(kinds))) if gs[i] is not None]
        if not live:
            return None, None
        raw = [gs[i] for i in live if not kinds[i]]
        rel = [gs[i] for i in live if kinds[i]]
        r, slot = None, 0
        if rel:
            (r,) = ctx.saved_tensors
            # the unfused ReLU node comes into being with its first consumer
            relu_born = min(i for i in live if kinds[i])
            slot = sum(1 for i in live if not kinds[i] and i > relu_born)
        return fan_fold(raw, rel, r, slot), None


def state_fan(y: torch.Tensor, kinds: Tuple[bool, ...]):
    """One alias of ``y`` (kind False) or of ``relu(y)`` (kind True) per
    consumer, in the order in which the consumers' autograd nodes will be
    created; each alias goes to exactly one of them. ``relu(y)`` is
    computed once.

    Backward is one pass over the consumers' gradients (fan_fold) where
    autograd would run a ``threshold_backward`` and a chain of pairwise
    adds, each a kernel with a tensor of its own. The result has the same
    bits: unfused, ``y``'s consumers are the raw ones and one ReLU node
    created with its first consumer; the engine runs nodes latest-created
    first and left-folds what arrives, rounding to the dtype after every
    add. ``kinds`` carries that order, the fold reproduces it. Several
    ReLU nodes on one tensor (one per consumer, as the cells' input
    reductions had) fold to the same bits as one shared node, since the
    mask commutes with the rounded sum.

    An alias that more than one node consumes (a spatial op that also
    exchanges halos, say) is summed by autograd before the fold sees it:
    still the right gradient, not necessarily the unfused bits."""
    return _StateFanFn.apply(y, tuple(bool(k) for k in kinds))


# ---------------------------------------------------------------------------
# Shared ReLU of a tensor that several modules consume through a ReLU
# ---------------------------------------------------------------------------

# A cell's output feeds the next two cells, each through a ReLU of its own
# in the reference; the stem's output feeds three. id(tensor) -> (weak
# reference, (version, grad mode), aliases not handed out yet). The
# reference's finaliser drops the entry with the tensor, so the table keeps
# nothing alive and a recycled id never meets a stale entry.
_SHARE = 3
_relu_memo: dict = {}
_sharing = True


@contextlib.contextmanager
def relu_sharing(on: bool):
    """Sharing off: every shared_relu call makes a ReLU of its own. A
    checkpointed cell needs that, as its recompute must save the same
    tensors in the same order as its forward did, which a hit in the
    table (nothing computed) would break."""
    global _sharing
    prev, _sharing = _sharing, on
    try:
        yield
    finally:
        _sharing = prev


def shared_relu(t: torch.Tensor) -> torch.Tensor:
    """relu(t), computed once per tensor OBJECT and differentiated by one
    state_fan node: the first request makes the fan, later ones take the
    next alias. A different object with the same values, a tensor modified
    since, another grad mode, or a fourth request simply start afresh,
    which costs a ReLU and changes no value."""
    # a leaf that requires grad is held by its own AccumulateGrad node,
    # which an alias waiting in the table would hold in turn: such tensors
    # (a pipeline stage's received input) get a ReLU per request
    if not _sharing or (t.is_leaf and t.requires_grad):
        return state_fan(t, (True,))[0]
    key = id(t)
    stamp = (t._version, torch.is_grad_enabled())
    ent = _relu_memo.get(key)
    if ent is not None and ent[0]() is t and ent[1] == stamp and ent[2]:
        return ent[2].pop(0)
    first, *rest = state_fan(t, (True,) * _SHARE)
    ref = weakref.ref(t, lambda _, key=key: _relu_memo.pop(key, None))
    _relu_memo[key] = (ref, stamp, rest)
    return first


def add_cat(entries: List[Tuple[torch.Tensor, Optional[torch.Tensor]]]):
    """entries: per concat slice, (a, b) -> slice = a + b, or (a, None)
    -> slice = a. Returns the channel-concatenated tensor."""
    tensors: List[torch.Tensor] = []
    index = {}

    def idx(t):
        k = id(t)
        if k not in index:
            index[k] = len(tensors)
            tensors.append(t)
        return index[k]

    spec = tuple(
        (idx(a), idx(b) if b is not None else -1, a.shape[1]) for a, b in entries
    )
    return _AddCatFn.apply(spec, *tensors)
