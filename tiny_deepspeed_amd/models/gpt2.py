"""GPT-2 example model (nanoGPT-style), written for the MI355X op stack.

Capability parity with ``/root/reference/example/model.py:15-157`` (same
architecture family and config fields: 12L/12H/768d GPT-2 small by default,
vocab 50304, block 1024, bias=False, selectable attention backend, returns
(logits, loss)). Differences by design:

- attention, GELU (or SwiGLU, ``mlp="swiglu"``) and the loss go through
  tiny_deepspeed_amd.ops — on GPU these are the hand-written CDNA4 kernels
  (fused causal attention, elementwise GELU / SwiGLU, fused cross-entropy);
  on CPU the torch fallbacks.
- nn.Linear / nn.LayerNorm / nn.Embedding are used raw so the parallel
  wrappers can swap them for strategy modules (SURVEY.md component #14).
- presets for small/medium/large/xl support the BASELINE.json configs.
"""

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from .. import ops


@dataclass
class GPTConfig:
    block_size: int = 1024
    vocab_size: int = 50304
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    # attention probabilities (fused into the attention kernels) and the
    # embedding sum
    dropout: float = 0.0
    # each block's two residual branches (after the attention and the MLP
    # c_proj), fused into the next residual LayerNorm kernel: no extra pass,
    # no stored mask
    resid_dropout: float = 0.0
    bias: bool = False
    # "fused": CDNA4 flash-style kernel (composite torch on CPU);
    # "math": composite torch attention everywhere.
    attention: str = "fused"
    # row-chunked fused lm_head projection + cross-entropy: the full
    # (B*T, V) logits tensor is never materialized (-2.75 GB peak at
    # gpt2-medium b32) at the cost of recomputing chunk logits in backward
    # (+4 ms/step, ~3.6% — same-box A/B in BASELINE.md). Default off: the
    # throughput headline wins; flip on when memory-bound. Loss-only path
    # returns logits=None; inference with targets=None is unaffected.
    fused_lm_head: bool = False
    # grouped-query attention: K/V heads, a divisor of n_head; query head h
    # attends K/V head h // (n_head // n_kv_head). None: multi-head, today's
    # model. "fused" backend only (HIP kernels at head dim 128 in bf16 without
    # attention dropout, the composite elsewhere).
    n_kv_head: Optional[int] = None
    # "layernorm": nn.LayerNorm (today's model and state-dict keys);
    # "rmsnorm": nn.RMSNorm(n_embd, eps=1e-5) for ln_1, ln_2 and ln_f (weight
    # only; HIP kernels for bf16 widths up to 8192 once wrapped).
    norm: str = "layernorm"
    # "gelu": c_fc -> GELU -> c_proj (today's model and state-dict shapes);
    # "swiglu": the gated SiLU MLP. c_fc projects to 2 * hidden, rows
    # [0, hidden) the gate and [hidden, 2 * hidden) the up projection, and
    # c_proj takes silu(gate) * up (one HIP kernel each way on GPU).
    mlp: str = "gelu"
    # MLP width. None: 4 * n_embd for "gelu"; for "swiglu" 8 * n_embd / 3
    # rounded up to a multiple of 256 (768 -> 2048, 1024 -> 2816,
    # 4096 -> 11008), about the parameter count of the GELU MLP.
    mlp_hidden: Optional[int] = None

    def mlp_width(self):
        if self.mlp not in ("gelu", "swiglu"):
            raise ValueError(f"unknown mlp \"{self.mlp}\": expected "
                             "\"gelu\" or \"swiglu\"")
        if self.mlp_hidden is not None:
            if self.mlp_hidden < 1:
                raise ValueError(f"mlp_hidden must be >= 1, got "
                                 f"{self.mlp_hidden}")
            return self.mlp_hidden
        if self.mlp == "gelu":
            return 4 * self.n_embd
        return -(-8 * self.n_embd // (3 * 256)) * 256

    def make_norm(self):
        if self.norm == "layernorm":
            return nn.LayerNorm(self.n_embd)
        if self.norm == "rmsnorm":
            return nn.RMSNorm(self.n_embd, eps=1e-5)
        raise ValueError(f"unknown norm \"{self.norm}\": expected "
                         "\"layernorm\" or \"rmsnorm\"")

    @classmethod
    def gpt2_small(cls, **kw):
        return cls(n_layer=12, n_head=12, n_embd=768, **kw)

    @classmethod
    def gpt2_medium(cls, **kw):
        return cls(n_layer=24, n_head=16, n_embd=1024, **kw)

    @classmethod
    def gpt2_large(cls, **kw):
        return cls(n_layer=36, n_head=20, n_embd=1280, **kw)

    @classmethod
    def gpt2_xl(cls, **kw):
        return cls(n_layer=48, n_head=25, n_embd=1600, **kw)

    @classmethod
    def named(cls, name, **kw):
        presets = {
            "gpt2-small": cls.gpt2_small,
            "gpt2-medium": cls.gpt2_medium,
            "gpt2-large": cls.gpt2_large,
            "gpt2-xl": cls.gpt2_xl,
        }
        return presets[name](**kw)


class CausalSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        assert config.n_embd % config.n_head == 0
        self.n_head = config.n_head
        self.head_dim = config.n_embd // config.n_head
        self.attention = config.attention
        self.dropout = config.dropout
        self.n_kv_head = config.n_kv_head
        qkv_dim = 3 * config.n_embd
        if self.n_kv_head is not None:
            if self.n_kv_head < 1 or self.n_head % self.n_kv_head:
                raise ValueError(f"n_kv_head {self.n_kv_head} must divide "
                                 f"n_head {self.n_head}")
            if self.attention != "fused":
                raise ValueError(
                    f"n_kv_head needs the \"fused\" attention backend; "
                    f"\"{self.attention}\" splits c_attn into three equal parts")
            # [q heads | k heads | v heads]
            qkv_dim = (self.n_head + 2 * self.n_kv_head) * self.head_dim
        self.c_attn = nn.Linear(config.n_embd, qkv_dim, bias=config.bias)
        self.c_proj = nn.Linear(config.n_embd, config.n_embd, bias=config.bias)

    def forward(self, x):
        B, T, E = x.shape
        qkv = self.c_attn(x)
        if self.attention == "fused":
            # packed-qkv path: the stride-aware kernel reads qkv directly,
            # no transpose-copies (saves 8 (B,T,E)-sized copies per layer
            # vs the reference's split+transpose+contiguous dance)
            return self.c_proj(ops.fused_causal_attention(
                qkv, self.n_head, dropout_p=self.dropout,
                training=self.training, n_kv_head=self.n_kv_head))
        q, k, v = qkv.split(E, dim=2)
        # (B, T, E) -> (B, H, T, D)
        q = q.view(B, T, self.n_head, self.head_dim).transpose(1, 2).contiguous()
        k = k.view(B, T, self.n_head, self.head_dim).transpose(1, 2).contiguous()
        v = v.view(B, T, self.n_head, self.head_dim).transpose(1, 2).contiguous()
        if self.attention == "math":
            scale = 1.0 / math.sqrt(self.head_dim)
            mask = torch.ones(T, T, dtype=torch.bool, device=x.device).tril()
            s = torch.matmul(q, k.transpose(-2, -1)) * scale
            s = s.masked_fill(~mask, float("-inf"))
            p = torch.softmax(s.float(), dim=-1).to(q.dtype)
            if self.dropout > 0:
                p = nn.functional.dropout(p, self.dropout, self.training)
            y = torch.matmul(p, v)
        else:
            raise ValueError(f"unknown attention backend {self.attention}")
        y = y.transpose(1, 2).contiguous().view(B, T, E)
        return self.c_proj(y)


class MLP(nn.Module):
    def __init__(self, config):
        super().__init__()
        hidden = config.mlp_width()
        self.gated = config.mlp == "swiglu"
        fc_out = 2 * hidden if self.gated else hidden
        self.c_fc = nn.Linear(config.n_embd, fc_out, bias=config.bias)
        self.c_proj = nn.Linear(hidden, config.n_embd, bias=config.bias)

    def forward(self, x):
        act = ops.swiglu if self.gated else ops.gelu
        return self.c_proj(act(self.c_fc(x)))


class Block(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.ln_1 = config.make_norm()
        self.attn = CausalSelfAttention(config)
        self.ln_2 = config.make_norm()
        self.mlp = MLP(config)
        self.resid_dropout = config.resid_dropout

    def _drop(self, delta):
        """Residual dropout on the raw nn.LayerNorm path."""
        if self.resid_dropout > 0:
            return nn.functional.dropout(delta, self.resid_dropout,
                                         self.training)
        return delta

    def forward(self, x, delta=None):
        """Residual stream threading: takes (x, pending delta) and returns
        (h, pending delta) so each residual add fuses into the next
        LayerNorm kernel (wrapped modules expose forward_fused; the raw
        nn.LayerNorm path does the adds explicitly — same math)."""
        if delta is None:
            y1 = self.ln_1(x)
            h = x
        elif hasattr(self.ln_1, "forward_fused"):
            h, y1 = self.ln_1.forward_fused(x, delta, self.resid_dropout)
        else:
            h = x + self._drop(delta)
            y1 = self.ln_1(h)
        a = self.attn(y1)
        if hasattr(self.ln_2, "forward_fused"):
            h2, y2 = self.ln_2.forward_fused(h, a, self.resid_dropout)
        else:
            h2 = h + self._drop(a)
            y2 = self.ln_2(h2)
        return h2, self.mlp(y2)


class GPT2Model(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(config.vocab_size, config.n_embd),
            wpe=nn.Embedding(config.block_size, config.n_embd),
            h=nn.ModuleList(Block(config) for _ in range(config.n_layer)),
            ln_f=config.make_norm(),
        ))
        self.lm_head = nn.Linear(config.n_embd, config.vocab_size, bias=False)
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.Linear):
            nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if module.bias is not None:
                nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            nn.init.normal_(module.weight, mean=0.0, std=0.02)

    def forward(self, idx, targets=None):
        B, T = idx.shape
        assert T <= self.config.block_size, (
            f"sequence length {T} > block_size {self.config.block_size}"
        )
        pos = torch.arange(T, dtype=torch.long, device=idx.device)
        tok = self.transformer.wte(idx)
        posemb = self.transformer.wpe(pos)
        x = tok + posemb
        if self.config.dropout > 0:
            x = nn.functional.dropout(x, self.config.dropout, self.training)
        delta = None
        for block in self.transformer.h:
            x, delta = block(x, delta)
        ln_f = self.transformer.ln_f
        if delta is None:
            y = ln_f(x)
        elif hasattr(ln_f, "forward_fused"):
            _, y = ln_f.forward_fused(x, delta, self.config.resid_dropout)
        else:
            if self.config.resid_dropout > 0:
                delta = nn.functional.dropout(
                    delta, self.config.resid_dropout, self.training)
            y = ln_f(x + delta)
        if (targets is not None and self.config.fused_lm_head
                and hasattr(self.lm_head, "project_cross_entropy")):
            # fused row-chunked projection+loss: full (B*T, V) logits are
            # never materialized (the reference holds the 3.3 GB tensor for
            # backward, example/model.py:152-156). Training callers read
            # only the loss; logits are None on this path by design.
            return None, self.lm_head.project_cross_entropy(y, targets)
        logits = self.lm_head(y)
        loss = None
        if targets is not None:
            loss = ops.cross_entropy(logits, targets)
        return logits, loss

    def num_params(self):
        return sum(p.numel() for p in self.parameters())
