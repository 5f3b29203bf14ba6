"""The head-dim-128 attention kernels at sequence lengths that are no multiple
of 64 (the tail kernels of csrc/kernels/attention_d128.hip), through
attention_d128_ragged_fwd / _bwd and through the op layer.

q, k, v and dO are [:, :, :T] views of (B,H,T+64,128) buffers whose other
rows are NaN, the outputs such views of all-NaN buffers: a read of a row >= T
poisons a result (0 * NaN in an MFMA is NaN), a write to one clears a guard
row. Inputs, references and bounds are those of test_attention_d128_gpu.py.

Blocks are ceil(T / (32 * waves)), 4 waves where 128 divides T rounded up to
64, else 2: T = 1 and 63 one 2-wave block; 65 and 96 one 4-wave block (at 65
wave 2 has one row and wave 3 none, at 96 the tail ends on a wave boundary);
129 three 2-wave blocks (the last has one row, and stages one row of its own
K and V); 200 two 4-wave blocks; 300 five 2-wave blocks; 1000 eight 4-wave
blocks. Balance "-1" forces tile pairs (odd middle tile at 300; the XCD remap
is on at B*H = 16).
"""

import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tests.test_attention_d128_gpu import (
    BF16, D, GRADS, K_ATTN_D128, SCALE, _fwd_refs, _inputs, _kernel)
from tiny_deepspeed_amd.ops import _ext

attention = importlib.import_module("tiny_deepspeed_amd.ops.attention")

PAD = 64
NAMES = ("o", "lse") + GRADS


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _guarded(t=None, like=None):
    """[:, :, :T] view of a (B,H,T+64,128) NaN buffer, holding t if given."""
    B, H, T, _ = (t if t is not None else like).shape
    buf = torch.full((B, H, T + PAD, D), float("nan"), device="cuda", dtype=BF16)
    if t is not None:
        buf[:, :, :T] = t
    return buf[:, :, :T]


def _ragged(q, k, v, do):
    """Forward and backward through the ragged entry points, every bf16
    tensor guarded; asserts the guard rows and returns o, lse, dq, dk, dv."""
    ext = _ext.get_ext()
    T = q.shape[2]
    q, k, v, do = (_guarded(t) for t in (q, k, v, do))
    o, dq, dk, dv = (_guarded(like=q) for _ in range(4))
    lse = ext.attention_d128_ragged_fwd(q, k, v, SCALE, o)[1]
    ext.attention_d128_ragged_bwd(q, k, v, o, lse, do, SCALE, dq, dk, dv)
    assert lse.shape == q.shape[:3]
    for name, view in zip(("o",) + GRADS, (o, dq, dk, dv)):
        guard = view._base[:, :, T:]
        assert torch.isnan(guard).all(), f"{name}: a row >= T was written"
        assert torch.isfinite(view.float()).all(), f"{name}: not finite"
    assert torch.isfinite(lse).all(), "lse: not finite"
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("B,H,T,balance", [
    (1, 2, 1, None), (2, 6, 63, None), (2, 8, 65, None), (1, 8, 96, None),
    (1, 6, 129, None), (2, 6, 200, None), (1, 8, 300, None),
    (1, 8, 300, "-1"), (1, 16, 1000, "-1"),
])
def test_attention_d128_ragged_reference_and_guard_rows_gpu(B, H, T, balance,
                                                            monkeypatch):
    """Judged as test_attention_d128_tracks_fp64_gpu judges the aligned
    kernels. At T = 1 the references of dq AND dk are zero (dS = dO.v0 - dO.o0
    cancels, dk = dS * scale * q0), so there both are held to the token-0
    bound, dk with q0 in k0's place."""
    if balance is not None:
        monkeypatch.setenv("TDSA_ATTN_BALANCE", balance)
    q, k, v, do = _inputs(B, H, T)
    o, lse, dq, dk, dv = _ragged(q, k, v, do)
    name = f"d128 ragged B{B} H{H} T{T} balance {balance}"
    o64, lse64, o_p, lse_p = _fwd_refs(B, H, T, False)
    KC.assert_tracks(o, o_p, o64, -1, K_ATTN_D128, KC.CAP_FWD, name + " o")
    KC.assert_lse_tracks(lse, lse_p, lse64, q, k, SCALE, name + " lse")
    # backward: the operation on (q, k, v, o, lse, do), kernel's o and lse
    g64 = KC.attn_bwd_formula(q, k, v, o, lse, do, SCALE, torch.float64)
    g_p = attention._composite_bwd(q, k, v, o, lse, do, SCALE)
    KC.assert_tracks(dv, g_p[2], g64[2], -1, K_ATTN_D128, KC.CAP_ATTN_GRAD,
                     name + " dv")
    if T == 1:
        for g, other, n in ((dq, k, "dq"), (dk, q, "dk")):
            bound = 2 * KC.dq_token0_bound(other, v, do, SCALE)
            worst = (g[:, :, 0].double().abs().amax(-1) / bound).max().item()
            print(f"TRACK {name} {n} token 0: |{n}| / bound = {worst:.3e}")
            assert worst <= 1.0, f"{name} {n}: {worst:.3e} x its bound"
        return
    # token 0's dot products have 128 terms: twice the 64-term bound
    KC.assert_dq_tracks(dq, g_p[0], g64[0],
                        2 * KC.dq_token0_bound(k, v, do, SCALE), K_ATTN_D128,
                        KC.CAP_ATTN_GRAD, name + " dq")
    KC.assert_tracks(dk, g_p[1], g64[1], -1, K_ATTN_D128, KC.CAP_ATTN_GRAD,
                     name + " dk")


@pytest.mark.parametrize("B,H,T", [(2, 8, 65), (2, 6, 200), (1, 8, 300)])
def test_attention_d128_ragged_bits_of_padded_aligned_call_gpu(B, H, T):
    """Rows < T carry the bits of the aligned kernels on the problem
    zero-padded to ceil64(T): padded rows only ever add exact zeros."""
    inputs = _inputs(B, H, T)
    T64 = (T + 63) // 64 * 64
    padded = [torch.zeros(B, H, T64, D, device="cuda", dtype=BF16)
              for _ in range(4)]
    for z, t in zip(padded, inputs):
        z[:, :, :T] = t
    for name, a, b in zip(NAMES, _ragged(*inputs), _kernel(*padded)):
        assert torch.equal(a, b[:, :, :T]), name


def test_attention_d128_ragged_routing_gpu(monkeypatch):
    """Both public ops reach the tail kernels at ragged T: the composite path
    is closed and the results carry the bits of the direct extension call."""
    def closed(*a, **kw):
        raise AssertionError("composite attention path taken")
    monkeypatch.setenv("TDSA_AUTOTUNE", "0")
    monkeypatch.setattr(attention, "_composite_fwd", closed)
    monkeypatch.setattr(attention, "_composite_bwd", closed)
    B, H, T = 1, 2, 200
    q, k, v, do = _inputs(B, H, T)
    want = _ragged(q, k, v, do)

    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o = attention.causal_attention(*leaves)
    o.backward(do)
    assert torch.equal(o, want[0])
    for leaf, ref, n in zip(leaves, want[2:], GRADS):
        assert torch.equal(leaf.grad, ref), n

    # the packed projection of the same values: (B, T, 3*H*D)
    qkv = torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], dim=2)
    qkv = qkv.reshape(B, T, 3 * H * D).requires_grad_(True)
    y = attention.fused_causal_attention(qkv, H)
    y.backward(do.permute(0, 2, 1, 3).reshape(B, T, H * D))
    assert torch.equal(y.view(B, T, H, D).permute(0, 2, 1, 3), want[0])
    g4 = qkv.grad.view(B, T, 3, H, D)
    for i, ref in enumerate(want[2:]):
        assert torch.equal(g4[:, :, i].permute(0, 2, 1, 3), ref), GRADS[i]


def test_attention_d128_ragged_entry_points_gpu():
    """T % 64 == 0 through the ragged entry points runs the aligned kernels;
    they name the argument they reject, and a valid call afterwards repeats
    the earlier one bit for bit."""
    ext = _ext.get_ext()
    B, H, T = 2, 8, 256
    q, k, v, do = _inputs(B, H, T)
    before = _ragged(q, k, v, do)
    for name, a, b in zip(NAMES, before, _kernel(q, k, v, do)):
        assert torch.equal(a, b), name

    with pytest.raises(RuntimeError,
                       match=r"k: attention kernel requires \(B,H,T,128\)"):
        ext.attention_d128_ragged_fwd(
            q, torch.zeros(B, H, T, 64, device="cuda", dtype=BF16), v, SCALE)

    for name, a, b in zip(NAMES, before, _ragged(q, k, v, do)):
        assert torch.equal(a, b), name
