"""The attention kernels at sequence lengths that are no multiple of 64 (the
TAIL variants of csrc/kernels/attention.hip), through the extension's
attention_ragged_fwd / attention_ragged_bwd and through the op layer.

q, k, v and dO are [:, :, :T] views of (B,H,T+64,64) buffers whose other rows
are NaN, the outputs such views of all-NaN buffers: a read of a row >= T
poisons a result (0 * NaN in an MFMA is NaN), a write to one clears a guard
row. References, bounds and slices are those of tests/kernel_check.py and of
test_attention_geometry_gpu.py.

Blocks are ceil(T / (32 * waves)), waves chosen for T rounded up to 64: T = 63
one 2-wave block; 65 and 96 one 4-wave block (at 65 wave 2 has one row and
wave 3 none, at 96 the tail ends on a wave boundary); 200 one 8-wave block
(wave 6 has 8 rows, wave 7 none); 300 five 2-wave blocks; 1000 four 8-wave
blocks.
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
SCALE = 1.0 / math.sqrt(64)
P_DROP = 0.3
SEED = 987654321
PAD = 64
NAMES = ("o", "lse", "dq", "dk", "dv")


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _guarded(t=None, like=None):
    """[:, :, :T] view of a (B,H,T+64,64) NaN buffer, holding t if given."""
    B, H, T, _ = (t if t is not None else like).shape
    buf = torch.full((B, H, T + PAD, 64), float("nan"), device="cuda", dtype=BF16)
    if t is not None:
        buf[:, :, :T] = t
    return buf[:, :, :T]


def _ragged(q, k, v, do, p=0.0, seed=0):
    """Forward and backward through the ragged entry points, every bf16
    tensor guarded; asserts the guard rows and returns o, lse, dq, dk, dv."""
    ext = _ext.get_ext()
    T = q.shape[2]
    q, k, v, do = (_guarded(t) for t in (q, k, v, do))
    o, dq, dk, dv = (_guarded(like=q) for _ in range(4))
    lse = ext.attention_ragged_fwd(q, k, v, SCALE, o, p, seed)[1]
    ext.attention_ragged_bwd(q, k, v, o, lse, do, SCALE, dq, dk, dv, p, seed)
    assert lse.shape == q.shape[:3]
    for name, view in zip(("o", "dq", "dk", "dv"), (o, dq, dk, dv)):
        guard = view._base[:, :, T:]
        assert torch.isnan(guard).all(), f"{name}: a row >= T was written"
        assert torch.isfinite(view.float()).all(), f"{name}: not finite"
    assert torch.isfinite(lse).all(), "lse: not finite"
    return o, lse, dq, dk, dv


@functools.lru_cache(maxsize=None)
def _case(B, H, T):
    """Inputs, fp64 forward reference and plain forward, once per shape."""
    q, k, v, do = KC.attn_inputs(B, H, T, "cuda", seed=T + H)
    o64, lse64, _ = KC.attn_fwd_formula(q, k, v, SCALE, torch.float64)
    o_p, lse_p = attention._composite_fwd(q, k, v, SCALE)
    return (q, k, v, do), (o64, lse64), (o_p, lse_p)


def _check(case, outs, name):
    """_check of test_attention_geometry_gpu.py. At T = 1 the references of
    dq AND dk are zero (dS = dO.v0 - dO.o0 cancels, dk = dS * scale * q0), so
    there both are held to dq_token0_bound, dk with q0 in k0's place."""
    (q, k, v, do), (o64, lse64), (o_p, lse_p) = case
    o, lse, dq, dk, dv = outs
    KC.assert_tracks(o, o_p, o64, -1, KC.K_ATTN, KC.CAP_FWD, name + " o")
    KC.assert_lse_tracks(lse, lse_p, lse64, q, k, SCALE, name + " lse")
    g64 = KC.attn_bwd_formula(q, k, v, o, lse, do, SCALE, torch.float64)
    g_p = attention._composite_bwd(q, k, v, o, lse, do, SCALE)
    KC.assert_tracks(dv, g_p[2], g64[2], -1, KC.K_ATTN, KC.CAP_ATTN_GRAD,
                     name + " dv")
    if q.shape[2] == 1:
        for g, other, n in ((dq, k, "dq"), (dk, q, "dk")):
            bound = KC.dq_token0_bound(other, v, do, SCALE)
            worst = (g[:, :, 0].double().abs().amax(-1) / bound).max().item()
            print(f"TRACK {name} {n} token 0: |{n}| / bound = {worst:.3e}")
            assert worst <= 1.0, f"{name} {n}: {worst:.3e} x its bound"
        return
    KC.assert_dq_tracks(dq, g_p[0], g64[0], KC.dq_token0_bound(k, v, do, SCALE),
                        KC.K_ATTN, KC.CAP_ATTN_GRAD, name + " dq")
    KC.assert_tracks(dk, g_p[1], g64[1], -1, KC.K_ATTN, KC.CAP_ATTN_GRAD,
                     name + " dk")


@pytest.mark.parametrize("B,H,T,balance", [
    (1, 2, 1, None), (2, 6, 63, None), (2, 8, 65, None), (1, 8, 96, None),
    (2, 6, 200, None), (1, 8, 300, None), (1, 8, 1000, None),
    (1, 8, 300, -1), (1, 8, 1000, -1),   # forced pairs; odd middle tile at 300
])
def test_attention_ragged_reference_and_guard_rows_gpu(B, H, T, balance,
                                                       monkeypatch):
    if balance is not None:
        monkeypatch.setenv("TDSA_ATTN_BALANCE", str(balance))
    case = _case(B, H, T)
    _check(case, _ragged(*case[0]), f"ragged B{B} H{H} T{T} bal{balance}")


@pytest.mark.parametrize("B,H,T", [(2, 8, 65), (2, 6, 200), (1, 8, 1000)])
def test_attention_ragged_bits_of_padded_aligned_call_gpu(B, H, T):
    """Rows < T carry the bits of the aligned kernels on the problem
    zero-padded to ceil64(T): padded rows only ever add exact zeros."""
    ext = _ext.get_ext()
    inputs = _case(B, H, T)[0]
    T64 = (T + 63) // 64 * 64
    qz, kz, vz, doz = (torch.zeros(B, H, T64, 64, device="cuda", dtype=BF16)
                       for _ in range(4))
    for z, t in zip((qz, kz, vz, doz), inputs):
        z[:, :, :T] = t
    oz, lsez = ext.attention_fwd(qz, kz, vz, SCALE)
    grads = ext.attention_bwd(qz, kz, vz, oz, lsez, doz, SCALE)
    for name, a, b in zip(NAMES, _ragged(*inputs), (oz, lsez) + tuple(grads)):
        assert torch.equal(a, b[:, :, :T]), name


def _extract_pd(q, k, p, seed):
    """Post-dropout probabilities Pd (B,H,T,T) by ceil(T/64) forward calls
    with an identity block in V (_extract_pd of the geometry test), the last
    block clipped to T."""
    ext = _ext.get_ext()
    B, H, T, _ = q.shape
    pd = torch.empty(B, H, T, T, device="cuda", dtype=BF16)
    eye = torch.eye(64, device="cuda", dtype=BF16)
    for j in range(0, T, 64):
        n = min(64, T - j)
        vj = torch.zeros(B, H, T, 64, device="cuda", dtype=BF16)
        vj[:, :, j:j + n] = eye[:n]
        pd[..., j:j + n] = ext.attention_ragged_fwd(
            q, k, vj, SCALE, None, p, seed)[0][..., :n]
    return pd


@pytest.mark.parametrize("B,H,T", [(2, 8, 200), (1, 6, 300)])
def test_attention_ragged_dropout_gpu(B, H, T):
    (q, k, v, do), (_, lse64), (_, lse_p) = _case(B, H, T)
    causal = KC.causal_mask(T, "cuda")
    pd = _extract_pd(q, k, P_DROP, SEED)
    assert not torch.isnan(pd).any()
    assert (pd.float() >= 0).all() and (pd.float()[..., ~causal] == 0).all()
    keep = (pd != 0) & causal
    rate = 1 - keep.sum().item() / (causal.sum().item() * B * H)
    print(f"drop rate {rate:.4f}")
    assert abs(rate - P_DROP) < 0.02, rate

    o, lse, dq, dk, dv = _ragged(q, k, v, do, P_DROP, SEED)
    name = f"ragged drop B{B} H{H} T{T}"
    o64 = KC.attn_fwd_formula(q, k, v, SCALE, torch.float64, keep, P_DROP)[0]
    o_p = KC.attn_fwd_formula(q, k, v, SCALE, torch.float32, keep,
                              P_DROP)[0].to(BF16)
    KC.assert_tracks(o, o_p, o64, -1, KC.K_ATTN_DROP, KC.CAP_FWD, name + " o")
    # the row sum is unmasked: lse is the no-dropout lse
    assert torch.equal(lse, _ragged(q, k, v, do)[1])

    args = (q, k, v, o, lse, do, SCALE)
    g64 = KC.attn_bwd_formula(*args, torch.float64, keep, P_DROP)
    g_p = [t.to(BF16) for t in
           KC.attn_bwd_formula(*args, torch.float32, keep, P_DROP)]
    KC.assert_dq_tracks(dq, g_p[0], g64[0],
                        KC.dq_token0_bound(k, v, do, SCALE, P_DROP),
                        KC.K_ATTN_DROP, KC.CAP_ATTN_GRAD, name + " dq")
    KC.assert_tracks(dk, g_p[1], g64[1], -1, KC.K_ATTN_DROP, KC.CAP_ATTN_GRAD,
                     name + " dk")
    KC.assert_tracks(dv, g_p[2], g64[2], -1, KC.K_ATTN_DROP, KC.CAP_ATTN_GRAD,
                     name + " dv")


@pytest.mark.parametrize("B,T,H", [(2, 200, 8), (1, 1000, 16)])
def test_fused_causal_attention_ragged_runs_the_kernels_gpu(B, T, H,
                                                            monkeypatch):
    """ops.fused_causal_attention on a packed qkv of ragged T: the composite
    path is closed, the result carries the bits of the contiguous extension
    call, and no score matrix is allocated."""
    def closed(*a, **kw):
        raise AssertionError("composite attention path taken")
    monkeypatch.setenv("TDSA_AUTOTUNE", "0")
    monkeypatch.setattr(attention, "_composite_fwd", closed)
    monkeypatch.setattr(attention, "_composite_bwd", closed)
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B, T, 3 * H * 64, generator=g).to(BF16).cuda()
    dy = torch.randn(B, T, H * 64, generator=g).to(BF16).cuda()
    qkv.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = ops.fused_causal_attention(qkv, H)
    y.backward(dy)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak growth {grown} B, one bf16 score matrix {B * H * T * T * 2} B")
    if T == 1000:
        assert grown < B * H * T * T * 2

    unpack = lambda t, n: t.detach().view(B, T, n, H, 64).permute(0, 3, 1, 2, 4)
    q, k, v = (unpack(qkv, 3)[:, :, :, i].contiguous() for i in range(3))
    do = unpack(dy, 1)[:, :, :, 0].contiguous()
    o, _, dq, dk, dv = _ragged(q, k, v, do)
    assert torch.equal(unpack(y, 1)[:, :, :, 0], o)
    for i, ref in enumerate((dq, dk, dv)):
        assert torch.equal(unpack(qkv.grad, 3)[:, :, :, i], ref), NAMES[2 + i]


def test_attention_ragged_entry_points_at_aligned_T_gpu():
    """T % 64 == 0 through the ragged entry points: the aligned kernels."""
    ext = _ext.get_ext()
    q, k, v, do = _case(2, 8, 512)[0]
    o, lse = ext.attention_fwd(q, k, v, SCALE)
    ref = (o, lse) + tuple(ext.attention_bwd(q, k, v, o, lse, do, SCALE))
    o_r, lse_r = ext.attention_ragged_fwd(q, k, v, SCALE)
    got = (o_r, lse_r) + tuple(
        ext.attention_ragged_bwd(q, k, v, o_r, lse_r, do, SCALE))
    for name, a, b in zip(NAMES, got, ref):
        assert torch.equal(a, b), name
