"""RMSNorm op functions (last-dim normalization, weight only, no bias).

CDNA4 HIP kernels (csrc/kernels/rmsnorm.hip) for bf16 rows of
8 <= N <= 8192 with N % 8 == 0:

  rmsnorm_fwd     : rstd = rsqrt(mean(x^2) + eps) in fp32, y = x * rstd * w
  rmsnorm_fwd_res : h = x + res written once (bf16), then y = RMSNorm(h)
  rmsnorm_dx      : g = w*dy, c = mean(g*x) * rstd^2, dx = (g - x*c) * rstd
                    (+ dh), plus the dw partials in one fp32 stripe buffer
  rmsnorm_dw      : column-reduce of the stripe buffer -> dw[N]

Dispatch is ops/layernorm.py's: routed GPU shapes offer {HIP kernel, torch
fp32 composite} to the tuner; CPU, fp32 and unrouted shapes (N > 8192,
N % 8 != 0) take the composite only. There is no fused residual-dropout
RMSNorm kernel: modules.RMSNorm drops the branch with torch first.
"""

import torch

from . import _ext
from .autotuner import dispatch


def _routed(x):
    """True where the HIP kernels take x's rows (span 1 or 4 reported)."""
    if not _ext.use_native(x) or x.dtype != torch.bfloat16:
        return False
    N = x.shape[-1]
    if N == 0:
        return False
    return _ext.get_ext().rmsnorm_geometry(x.numel() // N, N, True)[4] > 0


# --- forward candidates ----------------------------------------------------
def rms_fwd_hip(x, weight, eps):
    y, rstd = _ext.get_ext().rmsnorm_fwd(x.contiguous(), weight, eps)
    return y, rstd


def rms_fwd_torch(x, weight, eps):
    xf = x.float()
    rstd = (xf.square().mean(dim=-1) + eps).rsqrt()
    y = xf * rstd.unsqueeze(-1) * weight.float()
    return y.to(x.dtype), rstd


def rmsnorm_fwd(x, weight, eps=1e-5, tuner=None):
    """Returns (y, rstd); rstd is an fp32 per-row tensor."""
    return dispatch("rms_fwd", [rms_fwd_hip, rms_fwd_torch],
                    (x, weight, eps), x, tuner, supported=_routed(x))


def rms_fwd_res_hip(x, res, weight, eps):
    y, rstd, h = _ext.get_ext().rmsnorm_fwd(x.contiguous(), weight, eps,
                                            res.contiguous())
    return h, y, rstd


def rms_fwd_res_torch(x, res, weight, eps):
    h = x + res
    y, rstd = rms_fwd_torch(h, weight, eps)
    return h, y, rstd


def rmsnorm_fwd_res(x, res, weight, eps=1e-5, tuner=None):
    """Fused residual + RMSNorm: h = x + res; y = RMSNorm(h).
    Returns (h, y, rstd) — h is the residual stream, written once by the
    kernel instead of a separate elementwise add pass."""
    return dispatch("rms_fwd_res", [rms_fwd_res_hip, rms_fwd_res_torch],
                    (x, res, weight, eps), x, tuner, supported=_routed(x))


# --- backward-dx candidates ------------------------------------------------
def rms_dx_hip(dy, x, weight, rstd, dh):
    dx, pdw = _ext.get_ext().rmsnorm_bwd_dx(dy.contiguous(), x.contiguous(),
                                            weight, rstd, dh)
    return dx, (pdw,)


def rms_dx_torch(dy, x, weight, rstd, dh):
    xf = x.float()
    g = weight.float() * dy.float()
    rs = rstd.unsqueeze(-1)
    c = (g * xf).mean(dim=-1, keepdim=True) * rs * rs
    dx = (g - xf * c) * rs
    if dh is not None:
        dx = dx + dh.float()
    return dx.to(x.dtype), (dy, x, rstd)


def rmsnorm_dx(dy, x, weight, rstd, dh=None, tuner=None):
    """Input gradient (+ optional fused add of the residual-stream grad dh).
    x is what the forward normalised (its h in the residual form). Returns
    (dx, workspace): the HIP path's workspace is the fp32 stripe buffer of dw
    partials, the composite's the saved tensors; rmsnorm_dw takes either."""
    return dispatch("rms_dx", [rms_dx_hip, rms_dx_torch],
                    (dy, x, weight, rstd, dh), dy, tuner,
                    supported=_routed(x))


def rmsnorm_dw(workspace, dtype=None, tuner=None):
    """Reduce a rmsnorm_dx workspace to dw."""
    if len(workspace) == 1:  # HIP dx path: fp32 stripe buffer
        (pdw,) = workspace
        if _ext.use_native(pdw):
            ext = _ext.get_ext()
            if dtype in (None, torch.float32, torch.bfloat16):
                # the reduce kernel writes the parameter dtype itself
                return ext.rmsnorm_bwd_dw(pdw, dtype)
            return ext.rmsnorm_bwd_dw(pdw).to(dtype)
        dw = pdw.sum(dim=0)
    else:  # torch dx path: recompute from saved tensors
        dy, x, rstd = workspace
        N = x.shape[-1]
        xhat = x.float().reshape(-1, N) * rstd.reshape(-1, 1)
        dw = (dy.float().reshape(-1, N) * xhat).sum(dim=0)
    return dw if dtype is None else dw.to(dtype)
