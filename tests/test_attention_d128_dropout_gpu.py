"""Fused dropout in the head-dim-128 attention kernels (the DROP kernels of
csrc/kernels/attention_d128.hip): the mask is the head-dim-64 one, values
against fp64 with that mask as in test_attention_ragged_dropout_gpu.

T = 64 is one 2-wave block, 320 five 2-wave blocks, 384 three 4-wave blocks
(dkv with K and V in LDS; the middle tile of a pair runs alone), 200 ragged
with two 4-wave blocks, 300 ragged with five 2-wave blocks; each under
TDSA_ATTN_BALANCE unset and -1 (tile pairs: two passes per block, where a
per-row index kept from the first pass would show). Outputs go in as NaN.
"""

import functools
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.ops import _ext

attention = importlib.import_module("tiny_deepspeed_amd.ops.attention")

BF16 = torch.bfloat16
D = 128
SCALE = 1.0 / math.sqrt(D)
P_DROP = 0.3
SEED = 987654321
NAMES = ("o", "lse", "dq", "dk", "dv")
# Largest ratio to plain over the cases below on the MI355X: 2.92 (dk, T = 300;
# dq 2.85 at T = 384, dv 2.61 at T = 320, o 2.37 at T = 200). Twice that,
# rounded up to a power of two.
K_ATTN_D128_DROP = 8


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=BF16)


@functools.lru_cache(maxsize=None)
def _inputs(B, H, T, d=D):
    g = torch.Generator().manual_seed(T + H + d)
    q, k, v, do = (torch.randn(B, H, T, d, generator=g).to(BF16)
                   for _ in range(4))
    do = (do.float() * 4.0).to(BF16)
    return tuple(t.cuda() for t in (q, k, v, do))


def _entry(T, d=D):
    """The extension's (fwd, bwd) for T: aligned or ragged entry points."""
    ext = _ext.get_ext()
    stem = "attention_" + ("d128_" if d == 128 else "")
    stem += "ragged_" if T % 64 else ""
    return getattr(ext, stem + "fwd"), getattr(ext, stem + "bwd")


def _kernel(q, k, v, do, *drop):
    """Forward and backward into NaN-filled buffers; drop: (), or (p, seed)."""
    fwd, bwd = _entry(q.shape[2])
    o, lse = fwd(q, k, v, SCALE, _nan(*q.shape), *drop)
    grads = bwd(q, k, v, o, lse, do, SCALE,
                *(_nan(*q.shape) for _ in range(3)), *drop)
    return (o, lse) + tuple(grads)


def _extract_pd(q, k, p, seed):
    """Post-dropout probabilities Pd (B,H,T,T): one forward call per block of
    d = q.shape[-1] keys with V a one-hot block, the last block clipped."""
    B, H, T, d = q.shape
    fwd = _entry(T, d)[0]
    pd = torch.empty(B, H, T, T, device="cuda", dtype=BF16)
    eye = torch.eye(d, device="cuda", dtype=BF16)
    for j in range(0, T, d):
        n = min(d, T - j)
        vj = torch.zeros(B, H, T, d, device="cuda", dtype=BF16)
        vj[:, :, j:j + n] = eye[:n]
        pd[..., j:j + n] = fwd(q, k, vj, 1.0 / math.sqrt(d), None, p,
                               seed)[0][..., :n]
    return pd


@functools.lru_cache(maxsize=None)
def _keep_d64(B, H, T):
    """The keep mask of the head-dim-64 kernels at (B, H, T, P_DROP, SEED)."""
    q, k, _, _ = _inputs(B, H, T, 64)
    return (_extract_pd(q, k, P_DROP, SEED) != 0) & KC.causal_mask(T, "cuda")


@pytest.mark.parametrize("balance", [None, "-1"])
@pytest.mark.parametrize("B,H,T", [(2, 6, 64), (2, 8, 320), (2, 6, 384),
                                   (2, 8, 200), (1, 6, 300)])
def test_attention_d128_dropout_mask_and_values_gpu(B, H, T, balance,
                                                    monkeypatch):
    if balance is not None:
        monkeypatch.setenv("TDSA_ATTN_BALANCE", balance)
    q, k, v, do = _inputs(B, H, T)
    causal = KC.causal_mask(T, "cuda")
    pd = _extract_pd(q, k, P_DROP, SEED)
    assert not torch.isnan(pd).any()
    assert (pd.float() >= 0).all() and (pd.float()[..., ~causal] == 0).all()
    keep = (pd != 0) & causal
    assert torch.equal(keep, _keep_d64(B, H, T)), "not the head-dim-64 mask"

    o, lse, dq, dk, dv = _kernel(q, k, v, do, P_DROP, SEED)
    name = f"d128 drop B{B} H{H} T{T} balance {balance}"
    o64 = KC.attn_fwd_formula(q, k, v, SCALE, torch.float64, keep, P_DROP)[0]
    o_p = KC.attn_fwd_formula(q, k, v, SCALE, torch.float32, keep,
                              P_DROP)[0].to(BF16)
    K = K_ATTN_D128_DROP
    KC.assert_tracks(o, o_p, o64, -1, K, KC.CAP_FWD, name + " o")
    # the row sum is unmasked: lse is the no-dropout lse
    assert torch.equal(lse, _kernel(q, k, v, do)[1])

    args = (q, k, v, o, lse, do, SCALE)
    g64 = KC.attn_bwd_formula(*args, torch.float64, keep, P_DROP)
    g_p = [t.to(BF16) for t in
           KC.attn_bwd_formula(*args, torch.float32, keep, P_DROP)]
    # token 0's dot products have 128 terms: twice the 64-term bound
    KC.assert_dq_tracks(dq, g_p[0], g64[0],
                        2 * KC.dq_token0_bound(k, v, do, SCALE, P_DROP), K,
                        KC.CAP_ATTN_GRAD, name + " dq")
    for g, gp, gr, n in zip((dk, dv), g_p[1:], g64[1:], NAMES[3:]):
        KC.assert_tracks(g, gp, gr, -1, K, KC.CAP_ATTN_GRAD, f"{name} {n}")


@pytest.mark.parametrize("T", [128, 200])
def test_attention_d128_dropout_plumbing_bits_gpu(T):
    inputs = _inputs(1, 2, T)
    plain = _kernel(*inputs)
    for name, a, b in zip(NAMES, plain, _kernel(*inputs, 0.0, SEED)):
        assert torch.equal(a, b), f"dropout_p = 0: {name}"
    first = _kernel(*inputs, P_DROP, SEED)
    for name, a, b in zip(NAMES, first, _kernel(*inputs, P_DROP, SEED)):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), f"same seed: {name}"
    assert not torch.equal(first[0], _kernel(*inputs, P_DROP, SEED + 1)[0])


@pytest.mark.parametrize("T", [128, 200])
def test_attention_d128_dropout_routing_gpu(T, monkeypatch):
    """Both public ops hand (p, their drawn seed) to the kernels."""
    monkeypatch.setenv("TDSA_AUTOTUNE", "0")
    B, H, s = 1, 2, 1234
    q, k, v, do = _inputs(B, H, T)
    torch.manual_seed(s)
    seed = attention._draw_seed()
    want = _kernel(q, k, v, do, P_DROP, seed)

    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    torch.manual_seed(s)
    o = ops.causal_attention(*leaves, dropout_p=P_DROP, training=True)
    o.backward(do)
    assert torch.equal(o, want[0])
    for leaf, ref, n in zip(leaves, want[2:], NAMES[2:]):
        assert torch.equal(leaf.grad, ref), n

    # the packed projection of the same values: (B, T, 3*H*D)
    qkv = torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], dim=2)
    qkv = qkv.reshape(B, T, 3 * H * D).requires_grad_(True)
    torch.manual_seed(s)
    y = ops.fused_causal_attention(qkv, H, dropout_p=P_DROP, training=True)
    y.backward(do.permute(0, 2, 1, 3).reshape(B, T, H * D))
    assert torch.equal(y.view(B, T, H, D).permute(0, 2, 1, 3), want[0])
    g4 = qkv.grad.view(B, T, 3, H, D)
    for i, ref in enumerate(want[2:]):
        assert torch.equal(g4[:, :, i].permute(0, 2, 1, 3), ref), NAMES[2 + i]

    plain = _kernel(q, k, v, do)[0]   # training=False: no dropout
    assert torch.equal(ops.causal_attention(q, k, v, dropout_p=P_DROP), plain)
    y = ops.fused_causal_attention(qkv.detach(), H, dropout_p=P_DROP)
    assert torch.equal(y.view(B, T, H, D).permute(0, 2, 1, 3), plain)


def test_attention_d128_dropout_rejects_gpu():
    ext = _ext.get_ext()
    q, k, v, do = _inputs(1, 2, 64)
    before = _kernel(q, k, v, do, P_DROP, SEED)
    o, lse = before[:2]
    for p in (1.0, -0.1):
        for stem in ("attention_d128_", "attention_d128_ragged_"):
            with pytest.raises(RuntimeError, match="bad dropout_p"):
                getattr(ext, stem + "fwd")(q, k, v, SCALE, None, p, SEED)
            with pytest.raises(RuntimeError, match="bad dropout_p"):
                getattr(ext, stem + "bwd")(q, k, v, o, lse, do, SCALE,
                                           dropout_p=p, seed=SEED)
    for name, a, b in zip(NAMES, before, _kernel(q, k, v, do, P_DROP, SEED)):
        assert torch.equal(a, b), name
