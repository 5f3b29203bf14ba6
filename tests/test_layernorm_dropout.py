"""Residual dropout without a GPU: the torch replica of the kernels' mask hash
against plain Python integers, its keep fraction, and the model switch."""

import math

import torch

from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.models import GPTConfig, GPT2Model
from tiny_deepspeed_amd.ops import layernorm as L

P = 0.3


def _keep_int(idx, p, seed):
    """Dropout::keep (csrc/kernels/attn_common.h) in Python integers."""
    m = 0xFFFFFFFF
    thr = min(int((1.0 - torch.tensor(p, dtype=torch.float32).item()) * 2**32), m)
    h = (idx ^ (idx >> 32)) & m
    h = (h + (seed & m)) & m
    h ^= (seed >> 32) & m
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    h ^= h >> 16
    return h < thr


def test_replica_matches_python_integers():
    idx = list(range(0, 3000, 13)) + [2**32 - 2 + i for i in range(5)] + \
        [(1 << 33) + 7919 * i for i in range(100)] + [(1 << 40) + 3, (1 << 46) - 1]
    for seed in (7, (1 << 45) + 12345):
        for p in (P, 0.0):
            got = L._keep_at(torch.tensor(idx, dtype=torch.int64), p, seed)
            assert got.tolist() == [_keep_int(i, p, seed) for i in idx]
    # the (M, N) mask is that function at row * N + col
    mask = ops.dropout_keep_mask(5, 24, P, 7)
    assert mask.flatten().tolist() == [_keep_int(i, P, 7) for i in range(120)]


def test_keep_fraction():
    M, N = 64, 1024
    frac = ops.dropout_keep_mask(M, N, P, 2024).float().mean().item()
    assert abs(frac - (1 - P)) <= 5 * math.sqrt(P * (1 - P) / (M * N))


def test_model_resid_dropout_cpu():
    cfg = dict(block_size=16, vocab_size=64, n_layer=2, n_head=2, n_embd=16)
    torch.manual_seed(0)
    model = GPT2Model(GPTConfig(resid_dropout=P, **cfg))
    plain = GPT2Model(GPTConfig(**cfg))
    plain.load_state_dict(model.state_dict())
    idx = torch.randint(0, 64, (2, 16))
    tgt = torch.randint(0, 64, (2, 16))
    loss_train = model.train()(idx, tgt)[1]
    loss_eval = model.eval()(idx, tgt)[1]
    assert loss_train.item() != loss_eval.item()
    assert torch.equal(loss_eval, plain.eval()(idx, tgt)[1])


def test_module_composite_matches_autograd_cpu():
    """LayerNorm.forward_fused with dropout on the CPU (the composite path):
    outputs and all four gradients against torch autograd with the replica
    mask of the seed the module drew."""
    from tiny_deepspeed_amd.modules.normalization import LayerNorm
    from tiny_deepspeed_amd.ops.attention import _draw_seed

    M, N, s = 6, 40, 5
    torch.manual_seed(1)
    ln = LayerNorm(N).train()
    x, res, gh, gy = (torch.randn(M, N) for _ in range(4))
    x.requires_grad_(True)
    res.requires_grad_(True)
    torch.manual_seed(s)
    seed = _draw_seed()
    torch.manual_seed(s)
    h, y = ln.forward_fused(x, res, dropout_p=P)
    got = torch.autograd.grad([h, y], [x, res, ln.weight, ln.bias], [gh, gy])
    keep = ops.dropout_keep_mask(M, N, P, seed)
    h_ref = x + keep * res / (1 - P)
    y_ref = torch.nn.functional.layer_norm(h_ref, (N,), ln.weight, ln.bias, ln.eps)
    want = torch.autograd.grad([h_ref, y_ref], [x, res, ln.weight, ln.bias],
                               [gh, gy])
    for a, b in zip((h, y) + got, (h_ref, y_ref) + want):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
