"""Linear (affine) op functions: forward, input-grad, weight-grad, bias-grad.

Capability parity with the reference ops
(``/root/reference/tiny_deepspeed/core/module/ops/linear.py:9-75``), and the
same candidate-list dispatch architecture (reference ``ops/linear.py:9-17``):
each op owns a list of implementations and routes through the runtime
autotuner, which times them per shape and caches the winner.

  fwd : out[M,N] = x[M,K] @ W[N,K]^T (+ b)      (NT GEMM — hipBLASLt)
  dX  : dx[M,K]  = dy[M,N] @ W[N,K]             ({CDNA4 transpose of W +
                                                 the forward's NT GEMM,
                                                 NN GEMM — hipBLASLt}, tuned)
  dW  : dw[N,K]  = dy[M,N]^T @ x[M,K]           (TN GEMM — {CDNA4 MFMA
                                                 kernel, hipBLASLt}, tuned)
  db  : db[N]    = sum_M dy[M,N]                ({CDNA4 column_sum, torch})

MI355X design note: the forward NT GEMM stays on the library path —
measured at the practical MFMA ceiling (profiles/gemm_shapes_hipblaslt.txt,
fwd NT 1436 TF/s) — while dW (TN, the weakest library shape) carries a
hand-written split-M MFMA kernel as a tuner candidate so the question is
settled by measurement per shape, not by assertion. dX as an NN GEMM gets
the library's smaller tiles; with W^T made row-major first (one native
transpose per call, never cached, so no strategy can see a stale copy) it is
the forward's layout again, and the tuner times both per shape, transpose
included (profiles/linear_dx.txt).
"""

import os

import torch

from . import _ext
from .autotuner import default_tuner, dispatch


def _flatten_batch(t):
    # (B, T, E) -> (B*T, E); 2-D tensors pass through.
    return t.reshape(-1, t.shape[-1])


def linear_forward(x, weight, bias=None, tuner=None):
    out = torch.matmul(x, weight.t())
    if bias is not None:
        out = out + bias
    return out


# --- dX candidates ---------------------------------------------------------
def dx_library(dy2, weight):
    """hipBLASLt NN GEMM via torch.matmul."""
    return torch.matmul(dy2, weight)


def dx_nt(dy2, weight):
    """W^T by the CDNA4 transpose kernel (csrc/kernels/transpose.hip), made
    for this call only, then the library's forward-layout GEMM."""
    return _ext.get_ext().linear_dx_nt(dy2.contiguous(), weight)


def _dx_nt_supported(dy2, weight):
    if os.environ.get("TDSA_LINEAR_DX", "1") == "0":
        return False
    if not _ext.ext_available() or not hasattr(_ext.get_ext(), "linear_dx_nt"):
        return False
    # kernel contract (csrc/kernels/transpose.hip): bf16 [N, K] contiguous
    # with N % 64 == 0 and K % 64 == 0 — every GPT-2 preset's widths and the
    # padded vocabulary
    return (
        dy2.dtype == torch.bfloat16
        and weight.dtype == torch.bfloat16
        and weight.dim() == 2
        and weight.is_contiguous()
        and weight.shape[0] % 64 == 0
        and weight.shape[1] % 64 == 0
    )


def linear_input_grad(dy, weight, tuner=None):
    if not dy.is_cuda or weight.dim() != 2:
        return torch.matmul(dy, weight)
    dy2 = _flatten_batch(dy)
    candidates = [dx_library]
    if _ext.use_native(dy2) and _dx_nt_supported(dy2, weight):
        candidates.insert(0, dx_nt)
    tuner = tuner if tuner is not None else default_tuner()
    if tuner is not None:
        dx2 = tuner.choose("linear_dx", candidates, dy2, weight)
    else:
        dx2 = candidates[0](dy2, weight)
    return dx2.view(*dy.shape[:-1], weight.shape[-1])


# --- dW candidates ---------------------------------------------------------
def dw_library(dy2, x2):
    """hipBLASLt TN GEMM via torch.matmul."""
    return torch.matmul(dy2.t(), x2)


def dw_hip(dy2, x2):
    """Hand-written CDNA4 split-M MFMA TN kernel (csrc/kernels/gemm_tn.hip)."""
    return _ext.get_ext().gemm_tn(dy2.contiguous(), x2.contiguous())


def _dw_hip_supported(dy2, x2):
    if os.environ.get("TDSA_GEMM_TN", "1") == "0":
        return False
    if not _ext.ext_available() or not hasattr(_ext.get_ext(), "gemm_tn"):
        return False
    # kernel contract (csrc/kernels/gemm_tn.hip): bf16, M % 64 == 0,
    # N/K % 128 == 0 — covers the GPT-2 small/medium/large GEMM families
    # (xl's 1600-wide shapes fall to the library candidate)
    return (
        dy2.dtype == torch.bfloat16
        and x2.dtype == torch.bfloat16
        and dy2.shape[0] % 64 == 0
        and dy2.shape[1] % 128 == 0
        and x2.shape[1] % 128 == 0
    )


def linear_weight_grad(dy, x, tuner=None):
    dy2 = _flatten_batch(dy)
    x2 = _flatten_batch(x)
    candidates = [dw_library]
    if dy2.is_cuda and _ext.use_native(dy2) and _dw_hip_supported(dy2, x2):
        candidates.insert(0, dw_hip)
    tuner = tuner if tuner is not None else default_tuner()
    if tuner is not None and dy2.is_cuda:
        return tuner.choose("linear_dw", candidates, dy2, x2)
    return candidates[0](dy2, x2)


# --- db candidates ---------------------------------------------------------
def db_hip(dy2):
    return _ext.get_ext().column_sum(dy2.contiguous())


def db_torch(dy2):
    return dy2.sum(dim=0)


def linear_bias_grad(dy, tuner=None):
    dy2 = _flatten_batch(dy)
    return dispatch("linear_db", [db_hip, db_torch], (dy2,), dy2, tuner)
