"""Grouped-query attention without a GPU: the composite path of
ops.causal_attention with fewer K/V heads than query heads, and
GPTConfig.n_kv_head."""

import pytest
import torch

from tests import kernel_check as KC
from tiny_deepspeed_amd.models import GPTConfig, GPT2Model
from tiny_deepspeed_amd.ops import causal_attention


@pytest.mark.parametrize("H,Hkv", [(4, 2), (4, 1), (6, 2)])
def test_causal_attention_gqa_tracks_expanded_fp64(H, Hkv):
    """fp32 on the CPU against fp64 autograd on K/V expanded G-fold, whose
    autograd sums dK/dV over the group. T = 33 and D = 16: every sum has at
    most 33 fp32 terms, far inside the project's fp32 cap. Errors are taken
    per head: dq of token 0 is zero in exact arithmetic."""
    B, T, D = 2, 33, 16
    g = torch.Generator().manual_seed(H + Hkv)
    q, do = (torch.randn(B, H, T, D, generator=g) for _ in range(2))
    k, v = (torch.randn(B, Hkv, T, D, generator=g) for _ in range(2))
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o = causal_attention(*leaves)
    o.backward(do)

    ref = KC.attn_autograd(q, k.repeat_interleave(H // Hkv, dim=1),
                           v.repeat_interleave(H // Hkv, dim=1), do,
                           D ** -0.5, torch.float64)
    # dK/dV of the expansion, summed over each group
    dk64, dv64 = (t.view(B, Hkv, H // Hkv, T, D).sum(2) for t in ref[3:])
    for name, out, want in (("o", o.detach(), ref[0]),
                            ("dq", leaves[0].grad, ref[2]),
                            ("dk", leaves[1].grad, dk64),
                            ("dv", leaves[2].grad, dv64)):
        err = KC.rel_err(out, want, (-2, -1))[0]
        assert err <= KC.CAP_F32, f"{name}: {err:.3e}"


def _tiny(**kw):
    return GPTConfig(block_size=32, vocab_size=128, n_layer=2, n_head=4,
                     n_embd=64, **kw)


def test_gpt_n_kv_head_projection_and_gradients():
    torch.manual_seed(0)
    model = GPT2Model(_tiny(n_kv_head=2))
    c_attn = next(v for k, v in model.state_dict().items()
                  if k.endswith("c_attn.weight"))
    assert c_attn.shape == ((4 + 2 * 2) * 16, 64)
    x = torch.randint(0, 128, (2, 32))
    _, loss = model(x, x)
    loss.backward()
    assert torch.isfinite(loss)
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    with pytest.raises(ValueError, match="n_kv_head"):
        GPT2Model(_tiny(n_kv_head=2, attention="math"))
    with pytest.raises(ValueError, match="must divide"):
        GPT2Model(_tiny(n_kv_head=3))


def test_gpt_n_kv_head_none_is_the_multi_head_model():
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    base = shapes(GPT2Model(_tiny()))
    assert shapes(GPT2Model(_tiny(n_kv_head=None))) == base
    assert any(k.endswith("c_attn.weight") and s == (3 * 64, 64)
               for k, s in base.items())
