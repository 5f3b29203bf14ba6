"""LayerNorm module: callbacks over overridable hooks (see linear.py).

Parity with ``/root/reference/tiny_deepspeed/core/module/normalization.py:19-109``
including its restrictions: elementwise affine with bias required, and only
last-dimension normalization is supported. Forward saves (x, mean, rstd);
backward computes dx (+ dw/db stripe partials) via the CDNA4 kernel pair.
RMSNorm (weight only) follows the same scheme and saves (x, rstd).
"""

import torch
import torch.nn as nn

from .. import ops
from ..ops.attention import _draw_seed
from .linear import _ParamHooks, _check_grad_shape


class _LayerNormResFn(torch.autograd.Function):
    """Fused residual-add + LayerNorm: returns (h, y) with h = x + res.
    Backward folds the residual-stream gradient dh into dx (one kernel)."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, module):
        ctx.module = module
        # don't materialize an all-zeros dh when h is unused (ln_f discards
        # it) — backward treats dh=None as the plain no-fold path
        ctx.set_materialize_grads(False)
        h, y, mean, rstd = module.forward_res_callback(x, res)
        ctx.save_for_backward(h, mean, rstd)
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        h, mean, rstd = ctx.saved_tensors
        if dy is None:  # y unused: gradient flows through h alone
            return dh, dh, None, None, None
        dx, dw, db = ctx.module.backward_callback(dy, h, mean, rstd, dh=dh)
        return dx, dx, dw, db, None


class _LayerNormResDropoutFn(torch.autograd.Function):
    """_LayerNormResFn with dropout on the residual branch:
    h = x + dropout(res, p). The mask is a function of (p, seed) alone
    (ops.dropout_keep_mask); backward regenerates it, nothing is saved."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, module, p, seed):
        ctx.module = module
        ctx.dropout = (p, seed)
        ctx.set_materialize_grads(False)
        h, y, mean, rstd = module.forward_res_callback(x, res, (p, seed))
        ctx.save_for_backward(h, mean, rstd)
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        h, mean, rstd = ctx.saved_tensors
        if dy is None:  # y unused: gradient flows through h alone
            return (dh, ops.dropout_grad(dh, *ctx.dropout), None, None, None,
                    None, None)
        dx, dres, dw, db = ctx.module.backward_callback(
            dy, h, mean, rstd, dh=dh, dropout=ctx.dropout)
        return dx, dres, dw, db, None, None, None


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, module):
        ctx.module = module
        y, mean, rstd = module.forward_callback(x)
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        dx, dw, db = ctx.module.backward_callback(dy, x, mean, rstd)
        return dx, dw, db, None


class LayerNorm(_ParamHooks, nn.LayerNorm):
    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True,
                 bias=True, device=None, dtype=None, auto_tune=False):
        if not elementwise_affine or not bias:
            raise NotImplementedError(
                "tiny_deepspeed_amd.LayerNorm requires elementwise_affine=True "
                "and bias=True (reference parity: normalization.py:34-38)"
            )
        super().__init__(normalized_shape, eps=eps,
                         elementwise_affine=elementwise_affine, bias=bias,
                         device=device, dtype=dtype)
        if len(self.normalized_shape) != 1:
            raise NotImplementedError(
                "only last-dim LayerNorm is supported (reference parity: "
                "normalization.py:62-63)"
            )
        self.tuner = ops.RuntimeAutoTuner() if auto_tune else None

    # --- callbacks of the Functions above (parameters come through the
    # module's hooks; the Functions take them for autograd's sake) ---------
    def forward_callback(self, x):
        weight, bias = self._params_fwd()
        return ops.layernorm_fwd(x, weight, bias, eps=self.eps, tuner=self.tuner)

    def forward_res_callback(self, x, res, dropout=None):
        """dropout: (p, seed) of the residual-branch dropout, or None."""
        weight, bias = self._params_fwd()
        if dropout is not None:
            return ops.layernorm_fwd_res_dropout(x, res, weight, bias,
                                                 *dropout, eps=self.eps)
        return ops.layernorm_fwd_res(x, res, weight, bias, eps=self.eps,
                                     tuner=self.tuner)

    def backward_callback(self, dy, x, mean, rstd, dh=None, dropout=None):
        """(dx, dw, db); with dropout = (p, seed), (dx, dres, dw, db)."""
        w = self._weight_bwd()
        dres = ()
        if dropout is not None:
            dx, dr, ws = ops.layernorm_dx_dropout(dy, x, w, mean, rstd, dh,
                                                  *dropout)
            dres = (dr,)
        else:
            dx, ws = ops.layernorm_dx(dy, x, w, mean, rstd, dh=dh,
                                      tuner=self.tuner)
        dw = db = None
        if self.weight.requires_grad:
            dw, db = ops.layernorm_dwdb(ws, dtype=self.weight.dtype, tuner=self.tuner)
            _check_grad_shape(self.weight, dw)
            _check_grad_shape(self.bias, db)
            dw = self._publish(self.weight, dw)
            db = self._publish(self.bias, db)
        return (dx, *dres, dw, db)

    def forward(self, x):
        return _LayerNormFn.apply(x, self.weight, self.bias, self)

    def forward_fused(self, x, res, dropout_p=0.0):
        """(h, y) = (x + res, LN(x + res)) with the add fused in-kernel.
        In training mode dropout_p > 0 drops the residual branch first,
        h = x + dropout(res, dropout_p), in the same kernel, with a fresh seed
        from the torch CPU RNG as attention dropout draws it."""
        if self.training and dropout_p > 0.0:
            return _LayerNormResDropoutFn.apply(
                x, res, self.weight, self.bias, self, dropout_p,
                _draw_seed())
        return _LayerNormResFn.apply(x, res, self.weight, self.bias, self)


class _RMSNormResFn(torch.autograd.Function):
    """Fused residual-add + RMSNorm: returns (h, y) with h = x + res.
    Backward folds the residual-stream gradient dh into dx (one kernel)."""

    @staticmethod
    def forward(ctx, x, res, weight, module):
        ctx.module = module
        # as _LayerNormResFn: no all-zeros dh when h is unused
        ctx.set_materialize_grads(False)
        h, y, rstd = module.forward_res_callback(x, res)
        ctx.save_for_backward(h, rstd)
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        h, rstd = ctx.saved_tensors
        if dy is None:  # y unused: gradient flows through h alone
            return dh, dh, None, None
        dx, dw = ctx.module.backward_callback(dy, h, rstd, dh=dh)
        return dx, dx, dw, None


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, module):
        ctx.module = module
        y, rstd = module.forward_callback(x)
        ctx.save_for_backward(x, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, rstd = ctx.saved_tensors
        dx, dw = ctx.module.backward_callback(dy, x, rstd)
        return dx, dw, None


class RMSNorm(_ParamHooks, nn.RMSNorm):
    """nn.RMSNorm over the last dim through the op layer: HIP kernels for
    bf16 rows of 8 <= N <= 8192 (N % 8 == 0), the fp32 composite elsewhere.
    There is no fused residual-dropout RMSNorm kernel: forward_fused drops
    the branch with nn.functional.dropout and then takes the fused add."""

    def __init__(self, normalized_shape, eps=None, elementwise_affine=True,
                 device=None, dtype=None, auto_tune=False):
        if not elementwise_affine:
            raise NotImplementedError(
                "tiny_deepspeed_amd.RMSNorm requires elementwise_affine=True")
        super().__init__(normalized_shape, eps=eps,
                         elementwise_affine=elementwise_affine,
                         device=device, dtype=dtype)
        if len(self.normalized_shape) != 1:
            raise NotImplementedError("only last-dim RMSNorm is supported")
        self.tuner = ops.RuntimeAutoTuner() if auto_tune else None

    def _eps(self, x):
        """eps=None is the machine epsilon of the input dtype, as in torch."""
        return self.eps if self.eps is not None else torch.finfo(x.dtype).eps

    # --- callbacks of the Functions above --------------------------------
    def forward_callback(self, x):
        weight, _ = self._params_fwd()
        return ops.rmsnorm_fwd(x, weight, eps=self._eps(x), tuner=self.tuner)

    def forward_res_callback(self, x, res):
        weight, _ = self._params_fwd()
        return ops.rmsnorm_fwd_res(x, res, weight, eps=self._eps(x),
                                   tuner=self.tuner)

    def backward_callback(self, dy, x, rstd, dh=None):
        """(dx, dw)."""
        w = self._weight_bwd()
        dx, ws = ops.rmsnorm_dx(dy, x, w, rstd, dh=dh, tuner=self.tuner)
        dw = None
        if self.weight.requires_grad:
            dw = ops.rmsnorm_dw(ws, dtype=self.weight.dtype, tuner=self.tuner)
            _check_grad_shape(self.weight, dw)
            dw = self._publish(self.weight, dw)
        return dx, dw

    def forward(self, x):
        return _RMSNormFn.apply(x, self.weight, self)

    def forward_fused(self, x, res, dropout_p=0.0):
        """(h, y) = (x + res, RMSNorm(x + res)) with the add fused in-kernel.
        In training mode dropout_p > 0 first drops the residual branch with
        nn.functional.dropout (a pass of its own: the fused residual-dropout
        kernels exist for LayerNorm only)."""
        if self.training and dropout_p > 0.0:
            res = nn.functional.dropout(res, dropout_p, True)
        return _RMSNormResFn.apply(x, res, self.weight, self)
