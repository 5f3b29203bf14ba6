"""ops.swiglu on CPU against fp64 autograd of silu(gate) * up, and the
``mlp="swiglu"`` model: widths, parameter shapes, one step, and the default
model's unchanged state dict."""

import pytest
import torch
import torch.nn.functional as F

from tests import kernel_check as KC
from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.models import GPTConfig, GPT2Model


@pytest.mark.parametrize("dtype,cap", [(torch.float32, KC.CAP_F32),
                                       (torch.bfloat16, KC.CAP_POINT_BF16)])
@pytest.mark.parametrize("shape", [(3, 2 * 5), (2, 3, 2 * 8)])
def test_swiglu_cpu_matches_fp64_autograd(dtype, cap, shape):
    g = torch.Generator().manual_seed(len(shape))
    gu = torch.randn(*shape, generator=g).to(dtype).requires_grad_(True)
    dy = torch.randn(*shape[:-1], shape[-1] // 2, generator=g).to(dtype)
    y = ops.swiglu(gu)
    y.backward(dy)
    gu64 = gu.detach().double().requires_grad_(True)
    gate, up = gu64.chunk(2, dim=-1)
    y64 = F.silu(gate) * up
    y64.backward(dy.double())
    assert y.shape == y64.shape and y.dtype == dtype
    whole = tuple(range(len(shape)))  # one slice: the whole tensor
    assert not KC.rejected(y.detach(), y64.detach(), whole, cap)
    assert not KC.rejected(gu.grad, gu64.grad, whole, cap)


def test_swiglu_odd_last_dim_raises():
    with pytest.raises(ValueError, match=r"\(4, 7\)"):
        ops.swiglu(torch.randn(4, 7))


def _cfg(**kw):
    return GPTConfig(mlp="swiglu", n_embd=64, n_head=4, n_layer=2,
                     block_size=32, vocab_size=128, **kw)


@pytest.mark.parametrize("hidden,expect", [(None, 256), (40, 40)])
def test_swiglu_model_shapes_and_step(hidden, expect):
    cfg = _cfg(mlp_hidden=hidden)
    assert cfg.mlp_width() == expect
    model = GPT2Model(cfg)
    mlp = model.transformer.h[0].mlp
    assert mlp.c_fc.weight.shape == (2 * expect, 64)
    assert mlp.c_proj.weight.shape == (64, expect)
    idx = torch.randint(0, 128, (2, 32), generator=torch.Generator().manual_seed(0))
    _, loss = model(idx, idx)
    loss.backward()
    assert torch.isfinite(loss)
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_default_model_state_dict_unchanged():
    cfg = GPTConfig(n_embd=64, n_head=4, n_layer=2, block_size=32,
                    vocab_size=128)
    assert (cfg.mlp, cfg.mlp_hidden, cfg.mlp_width()) == ("gelu", None, 256)
    sd = {k: tuple(v.shape) for k, v in GPT2Model(cfg).state_dict().items()}
    block = {"ln_1.weight": (64,), "ln_1.bias": (64,),
             "attn.c_attn.weight": (192, 64), "attn.c_proj.weight": (64, 64),
             "ln_2.weight": (64,), "ln_2.bias": (64,),
             "mlp.c_fc.weight": (256, 64), "mlp.c_proj.weight": (64, 256)}
    want = {"transformer.wte.weight": (128, 64),
            "transformer.wpe.weight": (32, 64),
            "transformer.ln_f.weight": (64,), "transformer.ln_f.bias": (64,),
            "lm_head.weight": (128, 64)}
    want.update({f"transformer.h.{i}.{k}": v for i in range(2)
                 for k, v in block.items()})
    assert sd == want


@pytest.mark.parametrize("kw", [dict(mlp="relu"), dict(mlp_hidden=0)])
def test_bad_mlp_config_raises(kw):
    with pytest.raises(ValueError):
        GPT2Model(GPTConfig(n_embd=64, n_head=4, n_layer=1, **kw))
