"""Embedding module: callbacks over overridable hooks (see linear.py).

Parity with ``/root/reference/tiny_deepspeed/core/module/embedding.py:15-98``
(padding_idx plumbing; backward returns (None, grad_weight)). max_norm is
not supported (it mutates the weight in forward — the reference plumbs but
never exercises it; we raise instead of silently ignoring).
"""

import torch
import torch.nn as nn

from .. import ops
from .linear import _ParamHooks, _check_grad_shape


class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, weight, module):
        ctx.module = module
        ctx.save_for_backward(idx)
        return module.forward_callback(idx)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dw = ctx.module.backward_callback(dy, idx)
        return None, dw, None


class Embedding(_ParamHooks, nn.Embedding):
    def __init__(self, num_embeddings, embedding_dim, padding_idx=None,
                 max_norm=None, norm_type=2.0, scale_grad_by_freq=False,
                 sparse=False, _weight=None, device=None, dtype=None,
                 auto_tune=False):
        if max_norm is not None or scale_grad_by_freq or sparse:
            raise NotImplementedError(
                "max_norm/scale_grad_by_freq/sparse are not supported"
            )
        super().__init__(num_embeddings, embedding_dim, padding_idx=padding_idx,
                         _weight=_weight, device=device, dtype=dtype)
        self.tuner = ops.RuntimeAutoTuner() if auto_tune else None

    # --- callbacks of _EmbeddingFn ---------------------------------------
    def forward_callback(self, idx):
        weight, _ = self._params_fwd()
        return ops.embedding_forward(weight, idx, padding_idx=self.padding_idx,
                                     tuner=self.tuner)

    def backward_callback(self, dy, idx):
        if not self.weight.requires_grad:
            return None
        dw = ops.embedding_weight_grad(idx, dy, self.num_embeddings,
                                       padding_idx=self.padding_idx,
                                       tuner=self.tuner)
        _check_grad_shape(self.weight, dw)
        return self._publish(self.weight, dw)

    def forward(self, idx):
        return _EmbeddingFn.apply(idx, self.weight, self)
