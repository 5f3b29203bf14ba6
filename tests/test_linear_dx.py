"""linear_input_grad off the GPU: plain ``dy @ w``, no tuner, no native op."""

import importlib

import torch

from tiny_deepspeed_amd import ops

linear = importlib.import_module("tiny_deepspeed_amd.ops.linear")


class _NoTuner:
    def choose(self, *args, **kwargs):
        raise AssertionError("the tuner was consulted for CPU tensors")


def test_cpu_input_grad_is_plain_matmul_and_asks_no_tuner():
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float32, torch.bfloat16):
        dy = torch.randn(2, 3, 64, generator=g).to(dtype)
        w = torch.randn(64, 128, generator=g).to(dtype)
        dx = ops.linear_input_grad(dy, w, tuner=_NoTuner())
        assert dx.shape == (2, 3, 128)
        assert torch.equal(dx, torch.matmul(dy, w))
        assert torch.equal(ops.linear_input_grad(dy, w), torch.matmul(dy, w))
    # 2-D dy and a strided weight take the same way
    dy2 = torch.randn(5, 8, generator=g)
    wt = torch.randn(4, 8, generator=g).t()
    assert torch.equal(ops.linear_input_grad(dy2, wt, tuner=_NoTuner()),
                       dy2 @ wt)


def test_dx_nt_unsupported_without_the_extension(monkeypatch):
    dy2 = torch.randn(128, 64).to(torch.bfloat16)
    w = torch.randn(64, 64).to(torch.bfloat16)
    monkeypatch.delenv("TDSA_LINEAR_DX", raising=False)
    monkeypatch.setattr(linear._ext, "ext_available", lambda: False)
    assert not linear._dx_nt_supported(dy2, w)


def test_dx_nt_predicate_checks_the_kernel_contract(monkeypatch):
    """With an extension that has the op, the predicate is the kernel's
    contract: bf16, contiguous 2-D weight, both dims multiples of 64, and
    the TDSA_LINEAR_DX knob."""
    class _Ext:
        linear_dx_nt = staticmethod(lambda dy2, w: dy2 @ w)

    monkeypatch.setattr(linear._ext, "ext_available", lambda: True)
    monkeypatch.setattr(linear._ext, "get_ext", lambda: _Ext())
    monkeypatch.delenv("TDSA_LINEAR_DX", raising=False)
    bf = torch.bfloat16
    dy2 = torch.zeros(128, 64, dtype=bf)
    assert linear._dx_nt_supported(dy2, torch.zeros(64, 192, dtype=bf))
    assert not linear._dx_nt_supported(dy2, torch.zeros(64, 96, dtype=bf))
    assert not linear._dx_nt_supported(torch.zeros(128, 96, dtype=bf),
                                       torch.zeros(96, 64, dtype=bf))
    assert not linear._dx_nt_supported(dy2, torch.zeros(128, 64, dtype=bf).t())
    assert not linear._dx_nt_supported(dy2.float(), torch.zeros(64, 64))
    assert not linear._dx_nt_supported(dy2, torch.zeros(64, 64))
    monkeypatch.setenv("TDSA_LINEAR_DX", "0")
    assert not linear._dx_nt_supported(dy2, torch.zeros(64, 192, dtype=bf))
    monkeypatch.setattr(linear._ext, "get_ext", lambda: object())
    monkeypatch.delenv("TDSA_LINEAR_DX")
    assert not linear._dx_nt_supported(dy2, torch.zeros(64, 192, dtype=bf))
