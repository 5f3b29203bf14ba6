"""Grouped-query attention at head dim 128 (the attn_d128_gqa_* kernels)
through attention_d128_gqa_fwd / _bwd and the op layer.

Shapes (B, H, Hkv, T), the smallest that reach a distinct path each:
  2, 4, 2, 128  one 4-wave block, G = 2
  2, 4, 1, 256  MQA, G = 4, one tile pair
  2, 6, 2, 192  G = 3, 2-wave kernels (K/V in LDS), grid y no multiple of 8
  2, 8, 2, 65   4-wave tail, a wave with one row and one with none; the
                forward's grid y is 16 (XCD remap on, B*Hkv = 4)
  4, 8, 2, 200  4-wave tail, dkv grid y 8 (remap on)
  1, 4, 2, 300  2-wave tail, five blocks
Every bf16 tensor is a [:, :, :T] view of a NaN buffer with 64 more rows
(_guarded of the ragged tests): a read of a row >= T poisons a result, a
write to one clears a guard row.
"""

import functools
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tests.test_attention_d128_gpu import (
    BF16, D, GRADS, K_ATTN_D128, SCALE, _inputs)
from tests.test_attention_d128_ragged_gpu import _guarded
from tiny_deepspeed_amd.ops import _ext

attention = importlib.import_module("tiny_deepspeed_amd.ops.attention")

SHAPES = [(2, 4, 2, 128), (2, 4, 1, 256), (2, 6, 2, 192), (2, 8, 2, 65),
          (4, 8, 2, 200), (1, 4, 2, 300)]


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


@functools.lru_cache(maxsize=None)
def _gqa_inputs(B, H, Hkv, T, spike=False):
    """q, do of _inputs(B, H, T); k, v its first Hkv heads. spike: key row
    T*5//8 of each K/V head points along its group's mean query."""
    q, k, v, do = _inputs(B, H, T)
    k, v = (t[:, :Hkv].clone() for t in (k, v))
    if spike:
        qm = q.float().view(B, Hkv, H // Hkv, T, D).mean(dim=(2, 3))
        k[:, :, T * 5 // 8] = (4.0 * torch.sign(qm)).to(BF16)
    return q, k, v, do


def _expand(t, H):
    return t.repeat_interleave(H // t.shape[1], dim=1)


def _gqa(q, k, v, do):
    """Forward and backward through the grouped-query entry points, every
    bf16 tensor guarded; asserts the guard rows, returns o, lse, dq, dk, dv."""
    ext = _ext.get_ext()
    T = q.shape[2]
    q, k, v, do = (_guarded(t) for t in (q, k, v, do))
    o, dq = (_guarded(like=q) for _ in range(2))
    dk, dv = (_guarded(like=k) for _ in range(2))
    lse = ext.attention_d128_gqa_fwd(q, k, v, SCALE, o)[1]
    ext.attention_d128_gqa_bwd(q, k, v, o, lse, do, SCALE, dq, dk, dv)
    assert lse.shape == q.shape[:3] and torch.isfinite(lse).all()
    for name, view in zip(("o",) + GRADS, (o, dq, dk, dv)):
        assert torch.isnan(view._base[:, :, T:]).all(), \
            f"{name}: a row >= T was written"
        assert torch.isfinite(view.float()).all(), f"{name}: not finite"
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("B,H,Hkv,T,balance", [s + (None,) for s in SHAPES] + [
    s + (b,) for s in (SHAPES[1], SHAPES[4]) for b in ("-1", "0")])
def test_attention_d128_gqa_bits_of_expanded_call_gpu(B, H, Hkv, T, balance,
                                                      monkeypatch):
    """o, lse and dq carry the bits of the multi-head kernels on K/V expanded
    G-fold; no guard row is written and no NaN past T is read."""
    if balance is not None:
        monkeypatch.setenv("TDSA_ATTN_BALANCE", balance)
    ext = _ext.get_ext()
    q, k, v, do = _gqa_inputs(B, H, Hkv, T)
    o, lse, dq, _, _ = _gqa(q, k, v, do)
    ke, ve = _expand(k, H), _expand(v, H)
    o_e, lse_e = ext.attention_d128_ragged_fwd(q, ke, ve, SCALE)
    dq_e = ext.attention_d128_ragged_bwd(q, ke, ve, o_e, lse_e, do, SCALE)[0]
    assert torch.equal(o, o_e) and torch.equal(lse, lse_e)
    assert torch.equal(dq, dq_e)


@pytest.mark.parametrize("B,H,Hkv,T,spike",
                         [s + (False,) for s in SHAPES] + [(2, 4, 1, 256, True)])
def test_attention_d128_gqa_dkv_tracks_fp64_gpu(B, H, Hkv, T, spike):
    """dk, dv against the fp64 formula on expanded K/V summed over the group,
    given the kernel's own o and lse; plain is the fp32 composite, which like
    the kernel sums the group in fp32 and rounds once."""
    q, k, v, do = _gqa_inputs(B, H, Hkv, T, spike)
    o, lse, _, dk, dv = _gqa(q, k, v, do)
    g64 = KC.attn_bwd_formula(q, _expand(k, H), _expand(v, H), o, lse, do,
                              SCALE, torch.float64)
    g_p = attention._composite_bwd(q, k, v, o, lse, do, SCALE)
    for g, gp, gr, n in zip((dk, dv), g_p[1:], g64[1:], GRADS[1:]):
        gr = gr.view(B, Hkv, H // Hkv, T, D).sum(2)
        KC.assert_tracks(g, gp, gr, -1, K_ATTN_D128, KC.CAP_ATTN_GRAD,
                         f"d128 gqa B{B} H{H} Hkv{Hkv} T{T} spike {spike} {n}")


@pytest.mark.parametrize("B,H,Hkv,T", [(2, 4, 2, 128), (1, 4, 1, 200)])
def test_attention_d128_gqa_packed_layout_gpu(B, H, Hkv, T, monkeypatch):
    """fused_causal_attention on the (H + 2*Hkv)*D projection: the bits of the
    (B, H, T, D) call, and what reaches the extension are views of qkv, y and
    dqkv themselves."""
    monkeypatch.setenv("TDSA_AUTOTUNE", "0")
    q, k, v, do = _gqa_inputs(B, H, Hkv, T)
    want = _gqa(q, k, v, do)
    qkv = torch.cat([t.permute(0, 2, 1, 3).flatten(2) for t in (q, k, v)], 2)
    qkv = qkv.contiguous().requires_grad_(True)
    seen = []   # the arguments of the forward, then of the backward
    for name in ("attn_gqa_fwd_packed_hip", "attn_gqa_bwd_packed_hip"):
        monkeypatch.setattr(
            attention, name, lambda *a, real=getattr(attention, name):
            (seen.append(a), real(*a))[1])
    y = attention.fused_causal_attention(qkv, H, n_kv_head=Hkv)
    y.backward(do.permute(0, 2, 1, 3).flatten(2))

    E = (H + 2 * Hkv) * D
    fa, ba = seen
    # q, k, v inside qkv; dq, dk, dv inside one buffer of qkv's size
    assert ba[7].untyped_storage().nbytes() == 2 * qkv.numel()
    for i, off in enumerate((0, H * D, (H + Hkv) * D)):
        for t, first in ((fa[i], qkv), (ba[i], qkv), (ba[7 + i], ba[7])):
            assert t.data_ptr() == first.data_ptr() + 2 * off
            assert t.stride() == (T * E, D, E, 1)
    assert fa[4].data_ptr() == y.data_ptr()
    assert torch.equal(y.view(B, T, H, D).permute(0, 2, 1, 3), want[0])
    parts = qkv.grad.split([H * D, Hkv * D, Hkv * D], dim=2)
    for part, ref, n in zip(parts, want[2:], GRADS):
        assert torch.equal(part.view(B, T, -1, D).permute(0, 2, 1, 3), ref), n


def test_attention_d128_gqa_routing_gpu(monkeypatch):
    """Hkv < H reaches the grouped-query entry points (composite closed, bits
    of the direct call); Hkv == H does not; head dim 64 takes the composite
    and agrees with fp64 inside the project's caps."""
    monkeypatch.setenv("TDSA_AUTOTUNE", "0")
    def closed(*a, **kw):
        raise AssertionError("closed attention path taken")
    B, H, Hkv, T = 1, 4, 2, 200
    q, k, v, do = _gqa_inputs(B, H, Hkv, T)
    want = _gqa(q, k, v, do)
    with monkeypatch.context() as m:
        m.setattr(attention, "_composite_fwd", closed)
        m.setattr(attention, "_composite_bwd", closed)
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        o = attention.causal_attention(*leaves)
        o.backward(do)
        assert torch.equal(o, want[0])
        for leaf, ref, n in zip(leaves, want[2:], GRADS):
            assert torch.equal(leaf.grad, ref), n
    with monkeypatch.context() as m:
        for name in ("attn_gqa_fwd_hip", "attn_gqa_bwd_hip"):
            m.setattr(attention, name, closed)
        leaves = [t.clone().requires_grad_(True)
                  for t in (q, _expand(k, H), _expand(v, H))]
        attention.causal_attention(*leaves).backward(do)   # Hkv == H
        # head dim 64, Hkv < H: the composite
        q6, k6, v6, do6 = KC.attn_inputs(B, H, T, "cuda")
        k6, v6 = k6[:, :Hkv].contiguous(), v6[:, :Hkv].contiguous()
        leaves = [t.clone().requires_grad_(True) for t in (q6, k6, v6)]
        o6 = attention.causal_attention(*leaves)
        o6.backward(do6)
    ref = KC.attn_autograd(q6, _expand(k6, H), _expand(v6, H), do6, 0.125,
                           torch.float64)
    assert KC.rel_err(o6.detach(), ref[0], -1)[0] <= KC.CAP_FWD
    for leaf, g64, n in zip(leaves[1:], ref[3:], GRADS[1:]):
        g64 = g64.view(B, Hkv, H // Hkv, T, 64).sum(2)
        assert KC.rel_err(leaf.grad, g64, -1)[0] <= KC.CAP_ATTN_GRAD, n


def test_attention_d128_gqa_binding_rejects_gpu():
    """The binding names op and argument before anything is launched."""
    ext = _ext.get_ext()
    B, H, Hkv, T = 1, 4, 2, 64
    q, k, v, do = _gqa_inputs(B, H, Hkv, T)
    z = lambda *shape: torch.zeros(shape, device="cuda", dtype=BF16)
    rejected = [
        (r"attention_d128_gqa_fwd: k has 3 heads, which do not divide q's 4",
         lambda: ext.attention_d128_gqa_fwd(q, z(B, 3, T, D), z(B, 3, T, D),
                                            SCALE)),
        (r"attention_d128_gqa_fwd: v: k/v and dk/dv must each share strides",
         lambda: ext.attention_d128_gqa_fwd(q, k, _guarded(v), SCALE)),
        (r"attention_d128_gqa_fwd: k must be bf16",
         lambda: ext.attention_d128_gqa_fwd(q, k.float(), v, SCALE)),
        (r"attention_d128_gqa_bwd: dv: k/v and dk/dv must have one Hkv",
         lambda: ext.attention_d128_gqa_bwd(
             q, k, v, q, z(B, H, T).float(), do, SCALE, dv=z(B, 1, T, D))),
    ]
    for message, call in rejected:
        with pytest.raises(RuntimeError, match=message):
            call()
