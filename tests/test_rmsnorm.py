"""RMSNorm on the CPU path: the module against nn.RMSNorm under autograd, a
norm="rmsnorm" GPT-2 under Single and under ZeRO-3 (gloo, 2 ranks)."""

import pytest
import torch
import torch.nn as nn

import tiny_deepspeed_amd as tdsa
from tiny_deepspeed_amd import modules
from tiny_deepspeed_amd.models import GPTConfig, GPT2Model
from tests import _dist_workers as W
from tests.dist_utils import run_distributed

TOL = 1e-5


def _rms_cfg():
    return GPTConfig(norm="rmsnorm", **W.CFG)


@pytest.mark.parametrize("eps", [1e-5, None])
def test_module_matches_nn_rmsnorm(eps):
    torch.manual_seed(0)
    ref = nn.RMSNorm(48, eps=eps)
    mod = modules.RMSNorm(48, eps=eps)
    with torch.no_grad():
        ref.weight.normal_()
        mod.weight.copy_(ref.weight)
    x, res, gy, gh = (torch.randn(3, 5, 48) for _ in range(4))

    def run(m, fn, *ins):
        """outputs of fn and the gradients of its inputs and m.weight"""
        ins = [t.clone().requires_grad_(True) for t in ins]
        outs = fn(*ins)
        return (*outs, *torch.autograd.grad(outs, [*ins, m.weight],
                                            [gh, gy][-len(outs):]))

    # y, dx, dw; then the fused residual form with gradients through both
    # outputs: h, y, dx, dres, dw
    for got, want in (
            (run(mod, lambda a: (mod(a),), x),
             run(ref, lambda a: (ref(a),), x)),
            (run(mod, mod.forward_fused, x, res),
             run(ref, lambda a, r: (a + r, ref(a + r)), x, res))):
        for a, b in zip(got, want):
            assert torch.allclose(a, b, atol=TOL, rtol=TOL)


def test_rmsnorm_model_under_single():
    torch.manual_seed(0)
    raw = GPT2Model(_rms_cfg())
    torch.manual_seed(0)
    wrapped = tdsa.Single(GPT2Model(_rms_cfg()))
    assert isinstance(wrapped.module.transformer.ln_f, modules.RMSNorm)
    assert all(getattr(p, "_tdsa_wrapped", False) for p in wrapped.parameters())
    x, y = W.batch()
    _, loss_raw = raw(x, y)
    _, loss = wrapped(x, y)
    loss_raw.backward()
    loss.backward()
    assert loss.item() == pytest.approx(loss_raw.item(), abs=TOL)
    for (n, p), q in zip(wrapped.named_parameters(), raw.parameters()):
        assert torch.allclose(p.grad, q.grad, atol=TOL, rtol=1e-4), n
    state = wrapped.state_dict()
    assert "transformer.ln_f.weight" in state
    assert "transformer.ln_f.bias" not in state
    raw.load_state_dict(state)  # same keys, strict


def _zero3_rms_losses(rank, world):
    W.make_cfg = _rms_cfg
    return W.train_strategy(rank, world, "zero3")


def test_rmsnorm_model_under_zero3(monkeypatch):
    monkeypatch.setattr(W, "make_cfg", _rms_cfg)
    expected = W.single_device_losses()
    results = run_distributed(_zero3_rms_losses, world=2)
    for rank, losses in results.items():
        assert losses == pytest.approx(expected, abs=2e-4), (rank, losses)


def test_unknown_norm_raises():
    with pytest.raises(ValueError, match="bogus"):
        GPT2Model(GPTConfig(norm="bogus", **W.CFG))
