"""The attention kernels, called directly, at the launch geometry training
uses: several blocks in x with the XCD block remap on (B*H a multiple of 8)
and off, every wave-count template under the remap, the packed
(B,T,3,H,D) strides, fused dropout over more than one K/V tile, and the
online-softmax rescale in the backward.

Every call goes through the extension's attention_fwd/attention_bwd. The
reference is fp64 on the same bf16 values, the baseline ('plain') the
project's fp32 composite on the same inputs; bounds and slices are those of
tests/kernel_check.py. Every output buffer is handed in filled with NaN, so a
block that a wrong remap never schedules shows up as NaN.

Blocks in x are T / (32 * waves): 2 and 3 at T = 512 and 768 (8 waves), 5 at
T = 320 (2 waves, an odd count against the remap's window of 8), 1 at T = 64.
"""

import functools
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tiny_deepspeed_amd.ops import _ext

attention = importlib.import_module("tiny_deepspeed_amd.ops.attention")

BF16 = torch.bfloat16
SCALE = 1.0 / math.sqrt(64)
P_DROP = 0.3
SEED = 987654321
GRADS = ("dq", "dk", "dv")


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=BF16)


def _kernel(q, k, v, do, p=0.0, seed=0):
    """Forward and backward through the extension into NaN-filled buffers."""
    ext = _ext.get_ext()
    o, lse = ext.attention_fwd(q, k, v, SCALE, _nan(*q.shape), p, seed)
    dq, dk, dv = ext.attention_bwd(q, k, v, o, lse, do, SCALE, _nan(*q.shape),
                                   _nan(*q.shape), _nan(*q.shape), p, seed)
    return o, lse, dq, dk, dv


@functools.lru_cache(maxsize=None)
def _case(B, H, T, spike=False):
    """Inputs, fp64 forward reference and plain forward, computed once per
    shape and shared by the tests that use it (never modified)."""
    q, k, v, do = KC.attn_inputs(B, H, T, "cuda", seed=T + H, spike=spike)
    o64, lse64, _ = KC.attn_fwd_formula(q, k, v, SCALE, torch.float64)
    o_p, lse_p = attention._composite_fwd(q, k, v, SCALE)
    return (q, k, v, do), (o64, lse64), (o_p, lse_p)


def _check(case, outs, name):
    (q, k, v, do), (o64, lse64), (o_p, lse_p) = case
    o, lse, dq, dk, dv = outs
    KC.assert_tracks(o, o_p, o64, -1, KC.K_ATTN, KC.CAP_FWD, name + " o")
    KC.assert_lse_tracks(lse, lse_p, lse64, q, k, SCALE, name + " lse")
    # backward: the operation on (q, k, v, o, lse, do), kernel's o and lse
    g64 = KC.attn_bwd_formula(q, k, v, o, lse, do, SCALE, torch.float64)
    g_p = attention._composite_bwd(q, k, v, o, lse, do, SCALE)
    KC.assert_dq_tracks(dq, g_p[0], g64[0], KC.dq_token0_bound(k, v, do, SCALE),
                        KC.K_ATTN, KC.CAP_ATTN_GRAD, name + " dq")
    KC.assert_tracks(dk, g_p[1], g64[1], -1, KC.K_ATTN, KC.CAP_ATTN_GRAD,
                     name + " dk")
    KC.assert_tracks(dv, g_p[2], g64[2], -1, KC.K_ATTN, KC.CAP_ATTN_GRAD,
                     name + " dv")


# (2,8) and (3,8): remap on, two and three windows of 8 heads; (2,6): remap
# off with several blocks in x. T = 64 is the single-tile case.
@pytest.mark.parametrize("B,H,T", [
    (B, H, T) for T in (512, 768, 320) for B, H in ((2, 8), (3, 8), (2, 6))
] + [(2, 8, 64)])
def test_attention_remap_geometry_gpu(B, H, T):
    case = _case(B, H, T)
    _check(case, _kernel(*case[0]), f"attn B{B} H{H} T{T}")


@pytest.mark.parametrize("nw", [4, 2])
def test_attention_small_templates_under_remap_gpu(nw, monkeypatch):
    """The 4-wave and 2-wave templates (4 and 8 blocks in x at T = 512) with
    the remap on; the variables are read at every launch."""
    monkeypatch.setenv("TDSA_ATTN_FWD_NW", str(nw))
    monkeypatch.setenv("TDSA_ATTN_BWD_NW", str(nw))
    case = _case(2, 8, 512)
    _check(case, _kernel(*case[0]), f"attn NW{nw} B2 H8 T512")


def test_attention_packed_strides_bit_equal_gpu():
    """q/k/v as permuted views of one (B,T,3,H,64) buffer, o/do as views of
    (B,T,H*64) buffers, dq/dk/dv as views of one NaN-filled (B,T,3*H*64)
    buffer. Strides change addresses only: bit-equal to the contiguous call."""
    ext = _ext.get_ext()
    B, T, H = 2, 512, 8
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, T, 3, H, 64, generator=g).to(BF16).cuda()
    dy = torch.randn(B, T, H * 64, generator=g).to(BF16).cuda()
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    view = lambda t: t.view(B, T, H, 64).permute(0, 2, 1, 3)
    assert not q.is_contiguous()
    y = _nan(B, T, H * 64)
    o, lse = ext.attention_fwd(q, k, v, SCALE, view(y))
    dqkv = _nan(B, T, 3 * H * 64)
    d4 = dqkv.view(B, T, 3, H, 64)
    dq, dk, dv = ext.attention_bwd(
        q, k, v, view(y), lse, view(dy), SCALE,
        *(d4[:, :, i].permute(0, 2, 1, 3) for i in range(3)))
    assert o.data_ptr() == y.data_ptr() and dq.data_ptr() == dqkv.data_ptr()
    assert not torch.isnan(y).any()
    assert not torch.isnan(dqkv).any(), "packed gradient buffer has NaN"

    qc, kc, vc, doc = (t.contiguous() for t in (q, k, v, view(dy)))
    oc, lsec, dqc, dkc, dvc = _kernel(qc, kc, vc, doc)
    assert torch.equal(view(y), oc) and torch.equal(lse, lsec)
    for i, ref in enumerate((dqc, dkc, dvc)):
        assert torch.equal(d4[:, :, i].permute(0, 2, 1, 3), ref), GRADS[i]


def _extract_pd(q, k, p, seed):
    """The post-dropout probabilities Pd (B,H,T,T), by T/64 forward calls:
    in call j, V is the 64x64 identity in key rows 64j..64j+63 and zero
    elsewhere, so O = Pd[:, 64j:64j+64]."""
    ext = _ext.get_ext()
    B, H, T, _ = q.shape
    pd = torch.empty(B, H, T, T, device="cuda", dtype=BF16)
    eye = torch.eye(64, device="cuda", dtype=BF16)
    for j in range(T // 64):
        vj = torch.zeros(B, H, T, 64, device="cuda", dtype=BF16)
        vj[:, :, 64 * j:64 * j + 64] = eye
        pd[..., 64 * j:64 * j + 64] = ext.attention_fwd(
            q, k, vj, SCALE, _nan(B, H, T, 64), p, seed)[0]
    return pd


@pytest.mark.parametrize("B,H,T", [(2, 8, 512), (1, 6, 320)])
def test_attention_dropout_beyond_one_tile_gpu(B, H, T, monkeypatch):
    """Fused dropout with the 8-wave relaxed-cap forward under the remap
    (2,8,512) and the 2-wave template with five tiles (1,6,320): the realised
    mask is extracted, and forward and backward must match the same masked
    math; the mask does not depend on the tiling."""
    case = _case(B, H, T)
    (q, k, v, do), (o64_nodrop, lse64), (_, lse_p) = case
    causal = KC.causal_mask(T, "cuda")

    pd = _extract_pd(q, k, P_DROP, SEED)
    assert not torch.isnan(pd).any()
    assert (pd.float() >= 0).all() and (pd.float()[..., ~causal] == 0).all()
    keep = (pd != 0) & causal            # kept entries are strictly positive
    rate = 1 - keep.sum().item() / (causal.sum().item() * B * H)
    print(f"drop rate {rate:.4f}")
    assert abs(rate - P_DROP) < 0.02, rate

    # the RNG key is (seed, bh, row, key), not the tiling
    monkeypatch.setenv("TDSA_ATTN_FWD_NW", "2")
    keep_nw2 = (_extract_pd(q, k, P_DROP, SEED) != 0) & causal
    monkeypatch.delenv("TDSA_ATTN_FWD_NW")
    assert torch.equal(keep, keep_nw2)
    # and every (batch, head) draws its own mask
    flat = keep.reshape(B * H, -1)
    assert all(not torch.equal(flat[0], flat[i]) for i in range(1, B * H))

    # Pd = P * keep / (1-p), one query row per slice
    _, _, P64 = KC.attn_fwd_formula(q, k, v, SCALE, torch.float64)
    pd64 = P64 * keep / (1 - P_DROP)
    pd_p = (KC.attn_fwd_formula(q, k, v, SCALE, torch.float32)[2]
            * keep / (1 - P_DROP)).to(BF16)
    KC.assert_tracks(pd, pd_p, pd64, -1, KC.K_ATTN_DROP, KC.CAP_FWD, "drop Pd")
    del P64, pd64, pd_p

    o, lse, dq, dk, dv = _kernel(q, k, v, do, P_DROP, SEED)
    name = f"drop B{B} H{H} T{T}"
    o64, _, _ = KC.attn_fwd_formula(q, k, v, SCALE, torch.float64, keep, P_DROP)
    o_p = KC.attn_fwd_formula(q, k, v, SCALE, torch.float32, keep,
                              P_DROP)[0].to(BF16)
    KC.assert_tracks(o, o_p, o64, -1, KC.K_ATTN_DROP, KC.CAP_FWD, name + " o")
    # the row sum is unmasked: lse is the no-dropout lse
    KC.assert_lse_tracks(lse, lse_p, lse64, q, k, SCALE, name + " lse")
    lse_nodrop = _ext.get_ext().attention_fwd(q, k, v, SCALE)[1]
    e, i = KC.rel_err(lse, lse_nodrop.double(), None)
    print(f"lse vs no-dropout lse: worst rel diff {e:.2e} at {i}")
    assert torch.equal(lse, lse_nodrop), (e, i)

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


def test_attention_rescale_spike_backward_gpu():
    """The input of test_attention_rescale_spike_gpu at T = 256: one key row
    (160) dominates many later queries, so the running max jumps at a late
    tile. Forward and, new here, dq/dk/dv."""
    case = _case(1, 2, 256, spike=True)
    _check(case, _kernel(*case[0]), "attn spike T256")


def test_attention_binding_rejects_wrong_buffers_gpu():
    """The binding names the argument it rejects instead of launching with
    another tensor's strides and extents. Every wrong buffer is at least as
    large as the right one. A valid call after the rejected ones repeats the
    call made before them bit for bit."""
    ext = _ext.get_ext()
    B, H, T = 1, 2, 64
    q, k, v, do = KC.attn_inputs(B, H, T, "cuda", seed=T + H)
    before = _kernel(q, k, v, do)
    o, lse = before[:2]

    def bwd(**wrong):
        kw = dict(q=q, k=k, v=v, o=o, lse=lse, dout=do, scale=SCALE,
                  dq=_nan(B, H, T, 64), dk=_nan(B, H, T, 64),
                  dv=_nan(B, H, T, 64))
        kw.update(wrong)
        return ext.attention_bwd(**kw)

    def bwd_t96():
        t96 = [_nan(B, H, 96, 64).zero_() for _ in range(8)]
        lse96 = torch.zeros(B, H, 96, device="cuda")
        return ext.attention_bwd(*t96[:4], lse96, t96[4], SCALE, *t96[5:])

    rejected = [
        (r"out must have q's sizes",
         lambda: ext.attention_fwd(q, k, v, SCALE, _nan(B, H, 128, 64))),
        (r"dq must be bf16", lambda: bwd(dq=_nan(B, H, T, 64).float())),
        (r"dk last dim must be contiguous",
         lambda: bwd(dk=_nan(B, H, T, 128)[..., ::2])),
        (r"dv must have q's sizes", lambda: bwd(dv=_nan(B, 3, T, 64))),
        (r"lse must be fp32 on GPU with B\*H\*T elements",
         lambda: bwd(lse=torch.zeros(B, H, 65, device="cuda"))),
        (r"requires T % 64 == 0", bwd_t96),
        (r"bad dropout_p", lambda: bwd(dropout_p=1.0)),
    ]
    for message, call in rejected:
        with pytest.raises(RuntimeError, match=message):
            call()

    after = _kernel(q, k, v, do)
    for name, a, b in zip(("o", "lse") + GRADS, before, after):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), name
