"""Op-level numerics: the op functions (torch fallback path on CPU) against
plain torch references. The same suite runs the HIP kernels on GPU via
tests/test_gpu_kernels.py."""

import math

import pytest
import torch
import torch.nn.functional as F

from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.ops import attention as attn_ops


def test_linear_ops_match_autograd():
    torch.manual_seed(0)
    x = torch.randn(4, 7, 16, requires_grad=True)
    w = torch.randn(24, 16, requires_grad=True)
    b = torch.randn(24, requires_grad=True)
    y = ops.linear_forward(x, w, b)
    ref = F.linear(x, w, b)
    assert torch.allclose(y, ref, atol=1e-6)
    dy = torch.randn_like(ref)
    ref.backward(dy)
    assert torch.allclose(ops.linear_input_grad(dy, w), x.grad, atol=1e-5)
    assert torch.allclose(ops.linear_weight_grad(dy, x), w.grad, atol=1e-5)
    assert torch.allclose(ops.linear_bias_grad(dy), b.grad, atol=1e-5)


def test_layernorm_ops_match_autograd():
    torch.manual_seed(0)
    x = torch.randn(6, 5, 32, requires_grad=True)
    w = torch.randn(32, requires_grad=True)
    b = torch.randn(32, requires_grad=True)
    y, mean, rstd = ops.layernorm_fwd(x, w, b)
    ref = F.layer_norm(x, (32,), w, b)
    assert torch.allclose(y, ref, atol=1e-5)
    dy = torch.randn_like(ref)
    ref.backward(dy)
    dx, ws = ops.layernorm_dx(dy, x, w, mean, rstd)
    dw, db = ops.layernorm_dwdb(ws)
    assert torch.allclose(dx, x.grad, atol=1e-4)
    assert torch.allclose(dw, w.grad, atol=1e-4)
    assert torch.allclose(db, b.grad, atol=1e-4)


def test_embedding_ops_match_autograd():
    torch.manual_seed(0)
    w = torch.randn(50, 16, requires_grad=True)
    idx = torch.randint(0, 50, (3, 9))
    y = ops.embedding_forward(w, idx)
    ref = F.embedding(idx, w)
    assert torch.allclose(y, ref)
    dy = torch.randn_like(ref)
    ref.backward(dy)
    dw = ops.embedding_weight_grad(idx, dy, 50)
    assert torch.allclose(dw, w.grad, atol=1e-5)


def test_embedding_padding_idx():
    w = torch.randn(10, 4)
    idx = torch.tensor([[1, 2, 2, 3]])
    dy = torch.ones(1, 4, 4)
    dw = ops.embedding_weight_grad(idx, dy, 10, padding_idx=2)
    assert dw[2].abs().sum() == 0
    assert dw[1].abs().sum() > 0


def test_gelu_matches_torch_tanh_gelu():
    torch.manual_seed(0)
    x = torch.randn(100, requires_grad=True)
    y = ops.gelu(x)
    ref = F.gelu(x, approximate="tanh")
    assert torch.allclose(y, ref, atol=1e-6)
    dy = torch.randn_like(y)
    y.backward(dy)
    g1 = x.grad.clone()
    x.grad = None
    ref.backward(dy)
    assert torch.allclose(g1, x.grad, atol=1e-5)


def test_cross_entropy_matches_torch():
    torch.manual_seed(0)
    logits = torch.randn(12, 33, requires_grad=True)
    tgt = torch.randint(0, 33, (12,))
    loss = ops.cross_entropy(logits, tgt)
    ref_logits = logits.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(ref_logits, tgt)
    assert torch.allclose(loss, ref, atol=1e-5)
    loss.backward()
    ref.backward()
    assert torch.allclose(logits.grad, ref_logits.grad, atol=1e-5)


def test_cross_entropy_ignore_index():
    torch.manual_seed(0)
    logits = torch.randn(8, 11, requires_grad=True)
    tgt = torch.randint(0, 11, (8,))
    tgt[2] = -100
    tgt[5] = -100
    loss = ops.cross_entropy(logits, tgt)
    ref = F.cross_entropy(logits.detach(), tgt, ignore_index=-100)
    assert torch.allclose(loss, ref, atol=1e-5)
    loss.backward()
    assert logits.grad[2].abs().sum() == 0


def test_causal_attention_matches_math():
    torch.manual_seed(0)
    B, H, T, D = 2, 3, 16, 8
    q = torch.randn(B, H, T, D, requires_grad=True)
    k = torch.randn(B, H, T, D, requires_grad=True)
    v = torch.randn(B, H, T, D, requires_grad=True)
    out = ops.causal_attention(q, k, v)
    scale = 1.0 / math.sqrt(D)
    ref_q = q.detach().clone().requires_grad_(True)
    ref_k = k.detach().clone().requires_grad_(True)
    ref_v = v.detach().clone().requires_grad_(True)
    ref = F.scaled_dot_product_attention(ref_q, ref_k, ref_v, is_causal=True,
                                         scale=scale)
    assert torch.allclose(out, ref, atol=1e-5)
    do = torch.randn_like(out)
    out.backward(do)
    ref.backward(do)
    assert torch.allclose(q.grad, ref_q.grad, atol=1e-4)
    assert torch.allclose(k.grad, ref_k.grad, atol=1e-4)
    assert torch.allclose(v.grad, ref_v.grad, atol=1e-4)


def test_autotuner_picks_and_caches():
    calls = {"a": 0, "b": 0}

    def fa(x):
        calls["a"] += 1
        return x + 1

    def fb(x):
        calls["b"] += 1
        return x + 1

    tuner = ops.RuntimeAutoTuner(warmup=1, iters=2)
    x = torch.randn(4)
    out = tuner.choose("op", [fa, fb], x)
    assert torch.allclose(out, x + 1)
    before = dict(calls)
    tuner.choose("op", [fa, fb], x)
    # cached choice: exactly one more call total
    assert calls["a"] + calls["b"] == before["a"] + before["b"] + 1


def test_fused_attention_dropout_path_runs():
    torch.manual_seed(0)
    B, T, H, D = 2, 32, 2, 8
    qkv = torch.randn(B, T, 3 * H * D, requires_grad=True)
    y = ops.fused_causal_attention(qkv, H, dropout_p=0.5, training=True)
    assert y.shape == (B, T, H * D)
    y.sum().backward()
    assert qkv.grad is not None and torch.isfinite(qkv.grad).all()


def test_model_math_and_fused_backends_agree():
    from tiny_deepspeed_amd.models import GPTConfig, GPT2Model

    torch.manual_seed(0)
    cfg_f = GPTConfig(n_layer=2, n_head=2, n_embd=32, block_size=32,
                      vocab_size=128, attention="fused")
    m_f = GPT2Model(cfg_f)
    torch.manual_seed(0)
    cfg_m = GPTConfig(n_layer=2, n_head=2, n_embd=32, block_size=32,
                      vocab_size=128, attention="math")
    m_m = GPT2Model(cfg_m)
    x = torch.randint(0, 128, (2, 16))
    y = torch.randint(0, 128, (2, 16))
    _, lf = m_f(x, y)
    _, lm = m_m(x, y)
    assert torch.allclose(lf, lm, atol=1e-5), (lf.item(), lm.item())


class _CompositeAttnExt:
    """Stands in for the extension on CPU: the two attention entry points,
    computed by the composite, recording the dropout arguments they get."""

    def __init__(self):
        self.dropout = []

    def attention_fwd(self, q, k, v, scale, out=None, dropout_p=0.0, seed=0):
        self.dropout.append((dropout_p, seed))
        o, lse = attn_ops._composite_fwd(q.contiguous(), k.contiguous(),
                                         v.contiguous(), scale)
        return (o if out is None else out.copy_(o)), lse

    def attention_bwd(self, q, k, v, o, lse, dout, scale, dq=None, dk=None,
                      dv=None, dropout_p=0.0, seed=0):
        self.dropout.append((dropout_p, seed))
        grads = attn_ops._composite_bwd(
            q.contiguous(), k.contiguous(), v.contiguous(), o.contiguous(),
            lse, dout.contiguous(), scale)
        if dq is None:
            return grads
        return tuple(buf.copy_(g) for buf, g in zip((dq, dk, dv), grads))


class _RecordingTuner:
    def __init__(self):
        self.calls = []

    def choose(self, op, candidates, *args):
        self.calls.append((op, [c.__name__ for c in candidates], args))
        return candidates[0](*args)


@pytest.fixture
def attn_kernel_path_on_cpu(monkeypatch):
    """ops/attention.py takes its kernel path on CPU tensors: the `_ext` seam
    reports a native extension, and the tuner is a recording stub."""
    ext, tuner = _CompositeAttnExt(), _RecordingTuner()
    monkeypatch.setattr(attn_ops._ext, "use_native", lambda *t: True)
    monkeypatch.setattr(attn_ops._ext, "get_ext", lambda: ext)
    monkeypatch.setattr(attn_ops, "default_tuner", lambda: tuner)
    return ext, tuner


def _attn_leaves():
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(1, 64, 3 * 2 * 64, generator=g).to(torch.bfloat16)
    q, k, v = (t.contiguous().requires_grad_()
               for t in attn_ops._packed_views(qkv, 2))
    return qkv.requires_grad_(), q, k, v


def test_attention_tuner_ops_candidates_and_argument_order(
        attn_kernel_path_on_cpu):
    """What the tuner cache file stores: the four op names, the candidates'
    names with HIP first, and the order of the arguments given to choose."""
    _, tuner = attn_kernel_path_on_cpu
    qkv, q, k, v = _attn_leaves()
    ops.causal_attention(q, k, v).sum().backward()
    ops.fused_causal_attention(qkv, 2).sum().backward()
    assert [(op, names) for op, names, _ in tuner.calls] == [
        ("attn_fwd", ["attn_fwd_hip", "attn_fwd_composite"]),
        ("attn_bwd", ["attn_bwd_hip", "attn_bwd_composite"]),
        ("attn_fwd_packed",
         ["attn_fwd_packed_hip", "attn_fwd_packed_composite"]),
        ("attn_bwd_packed",
         ["attn_bwd_packed_hip", "attn_bwd_packed_composite"]),
    ]
    scale = 1.0 / math.sqrt(64)
    bhtd, bht = (1, 2, 64, 64), (1, 2, 64)

    def kinds(args):
        return [a if isinstance(a, float) else (tuple(a.shape), a.dtype)
                for a in args]

    t16, lse = (bhtd, torch.bfloat16), (bht, torch.float32)
    fwd, bwd, fwd_p, bwd_p = (args for _, _, args in tuner.calls)
    assert kinds(fwd) == [t16] * 3 + [scale]
    assert all(a is b for a, b in zip(fwd[:3], (q, k, v)))
    assert kinds(bwd) == [t16] * 4 + [lse, t16, scale]
    assert kinds(fwd_p) == [t16] * 3 + [scale, t16]
    assert kinds(bwd_p) == [t16] * 4 + [lse, t16, scale] + [t16] * 3
    # packed: q, k, v and dq, dk, dv are the three slices of one buffer each
    step = 2 * 64 * qkv.element_size()
    for a, b, c in (fwd_p[:3], bwd_p[:3], bwd_p[7:]):
        assert not a.is_contiguous()
        assert b.data_ptr() - a.data_ptr() == c.data_ptr() - b.data_ptr() == step
    assert fwd_p[0].data_ptr() == qkv.data_ptr()


def test_attention_dropout_bypasses_tuner(attn_kernel_path_on_cpu):
    """With dropout the HIP candidate runs directly (the composite has another
    mask), and backward gets the forward's p and seed."""
    ext, tuner = attn_kernel_path_on_cpu
    qkv, q, k, v = _attn_leaves()
    ops.causal_attention(q, k, v, dropout_p=0.25, training=True).sum().backward()
    ops.fused_causal_attention(qkv, 2, dropout_p=0.25,
                               training=True).sum().backward()
    assert tuner.calls == []
    (p0, s0), (p1, s1), (p2, s2), (p3, s3) = ext.dropout
    assert p0 == p1 == p2 == p3 == 0.25
    assert s0 == s1 and s2 == s3 and s0 != s2
    # not training: no dropout, the tuner is asked
    ops.causal_attention(q, k, v, dropout_p=0.25, training=False)
    assert [op for op, _, _ in tuner.calls] == ["attn_fwd"]
    assert ext.dropout[-1] == (0.0, 0)
