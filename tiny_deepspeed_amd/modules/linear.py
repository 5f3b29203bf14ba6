"""Linear module: forward/backward callbacks over overridable hooks.

Same load-bearing design as the reference's callback indirection
(``/root/reference/tiny_deepspeed/core/module/linear.py:16-92``): forward
and backward route through a torch.autograd.Function whose bodies are
instance methods, which is what lets the parallel strategies (parallel/)
inject RCCL collectives between the dW computation and the dX computation
for compute/comm overlap.

Backward contract: `backward_callback(dy, x)` returns (dx, dweight, dbias),
each gradient being whatever `_publish` made of it. The callbacks are
written once, here; a strategy changes only the three `_ParamHooks`.
"""

import os

import torch
import torch.nn as nn

from .. import ops


class _ParamHooks:
    """Where a module's callbacks get their parameters and what becomes of a
    finished gradient: the two decisions a parallel strategy takes. The base
    answers are the module's own parameters and plain autograd."""

    def _params_fwd(self):
        """(weight, bias) to compute the forward with."""
        return self.weight, getattr(self, "bias", None)

    def _weight_bwd(self):
        """Weight for the input gradient; called first in backward."""
        return self.weight

    def _publish(self, param, grad):
        """Dispose of param's finished gradient; autograd gets the result."""
        return grad


def _check_grad_shape(param, grad):
    # a ZeRO-3 non-owner's storage is empty: compare with the full shape
    full = getattr(param, "_tdsa_full_shape", param.shape)
    assert tuple(grad.shape) == tuple(full), (
        f"grad shape {tuple(grad.shape)} != parameter {tuple(full)}")


def _ce_chunk_rows(V):
    """Row-chunk size for the fused projection+loss: the largest chunk whose
    bf16 logits block (~C*V*2 bytes) stays within the MI355X LLC (256 MB
    Infinity Cache) with headroom, so the GEMM-written logits are consumed
    by the CE kernel without a round trip through HBM3E. Rounded UP to 256
    so the chunk GEMMs keep full wave efficiency."""
    env = os.environ.get("TDSA_CE_CHUNK")
    if env:
        return int(env)
    c = (112 << 20) // max(V, 1)
    return max(1024, ((c + 255) // 256) * 256)


class _LinearCEFn(torch.autograd.Function):
    """Fused lm_head projection + softmax cross-entropy, row-chunked.

    The reference materializes full (B*T, V) logits and runs F.cross_entropy
    on them (/root/reference/example/model.py:152-156): at b32/gpt2-medium
    that is a 3.3 GB tensor held for backward plus ~13 GB of HBM traffic
    through the fwd write / CE read / dlogits write / dX+dW reads. Here the
    projection GEMM and the CE kernels run per row-chunk (logits chunk stays
    LLC-resident) and backward RECOMPUTES each chunk's logits from (x, lse),
    so only the per-row logsumexp (4 bytes/row) survives the forward.

    Weight handling goes through the module's ``_ParamHooks``, as in
    _LinearFn's callbacks, so every parallel strategy keeps its semantics:
    the (possibly JIT-gathered, ZeRO-3) full weight in both directions, and
    dW routed into the strategy's collective or handed back to autograd.
    """

    @staticmethod
    def forward(ctx, x, weight, targets, module, ignore_index):
        x2 = x.reshape(-1, x.shape[-1])
        tg = targets.reshape(-1)
        w, _ = module._params_fwd()
        R = x2.shape[0]
        V = w.shape[0]
        C = _ce_chunk_rows(V)
        lse = torch.empty(R, dtype=torch.float32, device=x.device)
        loss_sum = None
        n_valid = None
        for s in range(0, R, C):
            e = min(s + C, R)
            logits_c = ops.linear_forward(x2[s:e], w)
            ls, lse_c, nv = ops.cross_entropy_fwd(logits_c, tg[s:e],
                                                  ignore_index,
                                                  tuner=module.tuner)
            lse[s:e] = lse_c
            loss_sum = ls if loss_sum is None else loss_sum + ls
            n_valid = nv if n_valid is None else n_valid + nv
        ctx.save_for_backward(x2, tg, lse, n_valid)
        ctx.module = module
        ctx.ignore_index = ignore_index
        ctx.x_shape = x.shape
        return loss_sum / n_valid.clamp(min=1)

    @staticmethod
    def backward(ctx, dloss):
        x2, tg, lse, n_valid = ctx.saved_tensors
        module = ctx.module
        w = module._weight_bwd()
        R, E = x2.shape
        V = w.shape[0]
        C = _ce_chunk_rows(V)
        nv = int(n_valid)
        # recompute logits per chunk, but materialize the FULL bf16 dlogits
        # (transient, freed at return) so dX and dW run as single
        # full-reduction GEMMs — a first per-chunk-accumulation version paid
        # ~10 ms/step in fp32 dW add/cast elementwise traffic (profiled)
        dlogits = torch.empty(R, V, dtype=x2.dtype, device=x2.device)
        for s in range(0, R, C):
            e = min(s + C, R)
            logits_c = ops.linear_forward(x2[s:e], w)
            ops.cross_entropy_bwd(
                dloss, logits_c, tg[s:e], lse[s:e], nv, ctx.ignore_index,
                tuner=module.tuner, out=dlogits[s:e])
        dx2 = ops.linear_input_grad(dlogits, w)
        dw = module._publish(module.weight,
                             ops.linear_weight_grad(dlogits, x2))
        return dx2.view(ctx.x_shape), dw, None, None, None


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, module):
        ctx.module = module
        # weight and bias are inputs for autograd's sake; the callback reads
        # them through the module's hooks
        y = module.forward_callback(x)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx, dw, db = ctx.module.backward_callback(dy, x)
        return dx, dw, db, None


class Linear(_ParamHooks, nn.Linear):
    """Drop-in nn.Linear whose fwd/bwd go through the op layer."""

    def __init__(self, in_features, out_features, bias=True, device=None,
                 dtype=None, auto_tune=False):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        self.tuner = ops.RuntimeAutoTuner() if auto_tune else None

    # --- callbacks of _LinearFn ------------------------------------------
    def forward_callback(self, x):
        weight, bias = self._params_fwd()
        return ops.linear_forward(x, weight, bias, tuner=self.tuner)

    def backward_callback(self, dy, x):
        # the order is what comm/compute overlap rests on: a strategy's
        # _publish launches the gradient's collective, so dW and db are
        # published as they appear and dX, last, runs underneath them
        w = self._weight_bwd()
        dw = db = None
        if self.weight.requires_grad:
            dw = ops.linear_weight_grad(dy, x, tuner=self.tuner)
            _check_grad_shape(self.weight, dw)
            dw = self._publish(self.weight, dw)
        if self.bias is not None and self.bias.requires_grad:
            db = ops.linear_bias_grad(dy, tuner=self.tuner)
            _check_grad_shape(self.bias, db)
            db = self._publish(self.bias, db)
        dx = ops.linear_input_grad(dy, w, tuner=self.tuner)
        return dx, dw, db

    def project_cross_entropy(self, x, targets, ignore_index=-100):
        """loss = cross_entropy(x @ W.T, targets), row-chunked so the full
        logits tensor is never materialized or saved. bias-free only (the
        GPT-2 lm_head; reference example/model.py:135)."""
        if self.bias is not None:
            raise NotImplementedError("fused lm_head+CE requires bias=False")
        return _LinearCEFn.apply(x, self.weight, targets, self, ignore_index)

    def forward(self, x):
        return _LinearFn.apply(x, self.weight, self.bias, self)
