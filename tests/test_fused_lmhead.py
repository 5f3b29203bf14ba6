"""Row-chunked fused lm_head projection + cross-entropy (_LinearCEFn):
loss and gradients must match the unfused lm_head -> cross_entropy path,
chunking must not change results, and the strategy hooks must publish dW
through the parallel machinery (covered at world>1 by the existing
loss-parity suites, since GPT2Model routes through the fused path)."""

import pytest
import torch

from tiny_deepspeed_amd import modules, ops
from tiny_deepspeed_amd.models import GPTConfig, GPT2Model
from tiny_deepspeed_amd import Single, AdamW


def _fused_vs_unfused(R, E, V, chunk, monkeypatch, ignore_index=-100,
                      with_ignored=False):
    monkeypatch.setenv("TDSA_CE_CHUNK", str(chunk))
    torch.manual_seed(0)
    lin = modules.Linear(E, V, bias=False)
    x = torch.randn(2, R // 2, E, requires_grad=True)
    tg = torch.randint(0, V, (2, R // 2))
    if with_ignored:
        tg[0, : R // 4] = ignore_index
    loss = lin.project_cross_entropy(x, tg, ignore_index=ignore_index)
    loss.backward()

    x_ref = x.detach().clone().requires_grad_(True)
    w_ref = lin.weight.detach().clone().requires_grad_(True)
    logits = torch.nn.functional.linear(x_ref, w_ref)
    ref = torch.nn.functional.cross_entropy(
        logits.reshape(-1, V), tg.reshape(-1), ignore_index=ignore_index)
    ref.backward()
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x.grad, x_ref.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lin.weight.grad, w_ref.grad,
                               rtol=1e-4, atol=1e-5)


def test_fused_lmhead_single_chunk(monkeypatch):
    _fused_vs_unfused(64, 32, 97 * 4, 4096, monkeypatch)


def test_fused_lmhead_multi_chunk(monkeypatch):
    # chunk < R forces the chunked accumulation paths (lse stitching,
    # fp32 dW accumulation, per-chunk recompute)
    _fused_vs_unfused(64, 32, 97 * 4, 16, monkeypatch)


def test_fused_lmhead_uneven_tail_chunk(monkeypatch):
    _fused_vs_unfused(60, 32, 97 * 4, 16, monkeypatch)


def test_fused_lmhead_ignore_index(monkeypatch):
    _fused_vs_unfused(64, 32, 97 * 4, 16, monkeypatch, with_ignored=True)


def test_fused_lmhead_bias_rejected():
    lin = modules.Linear(8, 16, bias=True)
    with pytest.raises(NotImplementedError):
        lin.project_cross_entropy(torch.randn(4, 8), torch.randint(0, 16, (4,)))


def test_model_uses_fused_path_and_trains(monkeypatch):
    monkeypatch.setenv("TDSA_CE_CHUNK", "16")
    cfg = GPTConfig(n_layer=2, n_head=2, n_embd=32, block_size=32,
                    vocab_size=64, fused_lm_head=True)
    torch.manual_seed(0)
    model = Single(GPT2Model(cfg))
    opt = AdamW(model.named_parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 64, (2, 32), generator=g)
    y = torch.randint(0, 64, (2, 32), generator=g)
    losses = []
    for _ in range(4):
        logits, loss = model(x, y)
        assert logits is None  # fused path materializes no logits
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0]
    # inference path still returns logits
    logits, loss = model(x)
    assert logits is not None and loss is None
    assert logits.shape == (2, 32, 64)


@pytest.mark.parametrize("strategy", ["ddp", "zero2", "zero3", "zero2flat"])
def test_fused_lmhead_strategy_parity_world2(strategy):
    """dW of the fused path must flow through each strategy's collective
    (the _publish hook): world-2 losses == single-device fused losses."""
    from tests.dist_utils import run_distributed
    from tests import _dist_workers as w

    single = w.fused_lmhead_single_losses()
    results = run_distributed(w.fused_lmhead_strategy_losses, world=2,
                              args=(strategy,))
    for rank, losses in results.items():
        assert losses == pytest.approx(single, rel=1e-4), (rank, losses)


def test_fused_path_matches_unfused_model(monkeypatch):
    """End-to-end: fused_lm_head on/off produce identical losses/updates."""
    def run(fused):
        cfg = GPTConfig(n_layer=2, n_head=2, n_embd=32, block_size=32,
                        vocab_size=64, fused_lm_head=fused)
        torch.manual_seed(0)
        model = Single(GPT2Model(cfg))
        opt = AdamW(model.named_parameters(), lr=1e-3)
        g = torch.Generator().manual_seed(1)
        x = torch.randint(0, 64, (2, 32), generator=g)
        y = torch.randint(0, 64, (2, 32), generator=g)
        out = []
        for _ in range(3):
            _, loss = model(x, y)
            loss.backward()
            opt.step()
            out.append(loss.item())
        return out

    monkeypatch.setenv("TDSA_CE_CHUNK", "16")
    assert run(True) == pytest.approx(run(False), rel=1e-5)
