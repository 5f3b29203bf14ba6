"""SwiGLU on the packed gate/up projection, autograd-wrapped.

``gu`` is ``(..., 2F)`` as one GEMM writes it: ``gate = gu[..., :F]``,
``up = gu[..., F:]``; ``swiglu(gu) = silu(gate) * up`` of shape ``(..., F)``.
On GPU forward and backward are one HIP kernel each (``swiglu.hip``: both
halves read in one pass, the backward writing the packed ``dgu`` and
recomputing from ``gu``, the only tensor saved), dispatched against the torch
composite through the runtime autotuner as ``ops/gelu.py`` does.
"""

import torch

from . import _ext
from .autotuner import dispatch


def _check(gu):
    """An odd last dim is no packed projection."""
    if gu.dim() < 1 or gu.shape[-1] % 2:
        raise ValueError(f"swiglu: the last dim of gu must be even (gate and "
                         f"up halves), got shape {tuple(gu.shape)}")


def _rows(gu):
    """gu as contiguous (M, 2F)."""
    _check(gu)
    return gu.contiguous().view(-1, gu.shape[-1])


def swiglu_fwd_hip(gu):
    y = _ext.get_ext().swiglu_fwd(_rows(gu))
    return y.view(*gu.shape[:-1], gu.shape[-1] // 2)


def swiglu_fwd_torch(gu):
    g, u = _rows(gu).float().chunk(2, dim=-1)
    y = g * torch.sigmoid(g) * u
    return y.to(gu.dtype).view(*gu.shape[:-1], gu.shape[-1] // 2)


def swiglu_fwd(gu, tuner=None):
    _check(gu)
    return dispatch("swiglu_fwd", [swiglu_fwd_hip, swiglu_fwd_torch], (gu,),
                    gu, tuner, supported=gu.numel() > 0)


def swiglu_bwd_hip(dy, gu):
    return _ext.get_ext().swiglu_bwd(dy.contiguous(), _rows(gu)).view(gu.shape)


def swiglu_bwd_torch(dy, gu):
    g, u = _rows(gu).float().chunk(2, dim=-1)
    dyf = dy.float().reshape(g.shape)
    s = torch.sigmoid(g)
    ds = dyf * s
    dgu = torch.cat([ds * u * (1.0 + g * (1.0 - s)), ds * g], dim=-1)
    return dgu.to(gu.dtype).view(gu.shape)


def swiglu_bwd(dy, gu, tuner=None):
    _check(gu)
    return dispatch("swiglu_bwd", [swiglu_bwd_hip, swiglu_bwd_torch], (dy, gu),
                    gu, tuner, supported=gu.numel() > 0)


class _SwigluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        return swiglu_fwd(gu)

    @staticmethod
    def backward(ctx, dy):
        (gu,) = ctx.saved_tensors
        return swiglu_bwd(dy, gu)


def swiglu(gu):
    return _SwigluFn.apply(gu)
