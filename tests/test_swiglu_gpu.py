"""SwiGLU HIP kernels (csrc/kernels/swiglu.hip), called through their
``*_hip`` functions, against fp64 silu(gate) * up and its analytic gradient on
the same rounded inputs; the op's torch candidate is the plain baseline of
kernel_check.assert_tracks and the slice is the whole output of one call.
Shapes are (M, F, TDSA_SWIGLU_GRID), chosen for the index walk (see CASES).

K_SWIGLU_FWD / K_SWIGLU_BWD: twice the largest ratio of the kernel's error to
the plain candidate's over these cases on an MI355X, rounded up to a power of
two (docs/kernels.md, "Test bounds").
"""

import copy
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tiny_deepspeed_amd.ops import _ext

S = importlib.import_module("tiny_deepspeed_amd.ops.swiglu")

BF16 = torch.bfloat16
F32 = torch.float32

K_SWIGLU_FWD = 2  # largest ratio 1.00 (every case: the rounding of the output)
K_SWIGLU_BWD = 4  # largest ratio 1.93 (fp32 (7, 5), unit pool: 9.8e-8 / 5.1e-8)

CASES = [
    # one vector per row, most threads idle
    (BF16, 3, 8, None),
    # 512 threads, vpr = 3, dc = 2, dr = 170: the carry fires on some steps
    (BF16, 1000, 24, 2),
    # dc = 0: the carry never fires
    (BF16, 700, 64, 2),
    # vpr = 600 > 512 threads: dr = 0, a row spans two steps
    (BF16, 5, 4800, 2),
    # the W = 1 path: F < W, F odd, F % 8 = 4
    (BF16, 3, 1, None), (BF16, 130, 7, 1), (BF16, 9, 2820, 1),
    # fp32: W = 4 and its W = 1 fallback
    (F32, 130, 4, 1), (F32, 9, 12, 1), (F32, 7, 5, 1),
]


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("TDSA_SWIGLU_GRID", raising=False)
    else:
        monkeypatch.setenv("TDSA_SWIGLU_GRID", str(grid))


def _inputs(M, F, dtype, pool, seed=0):
    gate, _ = KC.gelu_inputs(M * F, dtype, "cuda", pool, seed=seed)
    gate = gate.view(M, F).clone()
    if pool == "large":
        gate[0] = -100.0
    g = torch.Generator().manual_seed(seed + 1)
    up = torch.randn(M, F, generator=g).to(dtype).cuda()
    dy = torch.randn(M, F, generator=g).to(dtype).cuda()
    return torch.cat([gate, up], dim=1).contiguous(), dy


def _ref64(gu, dy):
    g, u = gu.double().chunk(2, dim=1)
    s = torch.sigmoid(g)
    ds = dy.double() * s
    return g * s * u, torch.cat([ds * u * (1 + g * (1 - s)), ds * g], dim=1)


def _poison_allocator(like):
    """Leave NaN behind in freed blocks of the output's size, so an element
    nobody wrote fails the finiteness check."""
    junk = [torch.full_like(like, float("nan")) for _ in range(2)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("dtype,M,F,grid", CASES)
def test_swiglu_kernels_gpu(dtype, M, F, grid, monkeypatch):
    _set_grid(monkeypatch, grid)
    cap = KC.CAP_POINT_BF16 if dtype == BF16 else KC.CAP_F32
    for pool in KC.gelu_pools():
        gu, dy = _inputs(M, F, dtype, pool)
        y64, dgu64 = _ref64(gu, dy)
        name = f"swiglu {pool} {M}x{F}"
        _poison_allocator(dy)
        y = S.swiglu_fwd_hip(gu)
        assert y.shape == (M, F) and y.dtype == dtype
        KC.assert_tracks(y, S.swiglu_fwd_torch(gu), y64, (0, 1), K_SWIGLU_FWD,
                         cap, name + " fwd")
        _poison_allocator(gu)
        dgu = S.swiglu_bwd_hip(dy, gu)
        assert dgu.shape == (M, 2 * F) and dgu.dtype == dtype
        KC.assert_tracks(dgu, S.swiglu_bwd_torch(dy, gu), dgu64, (0, 1),
                         K_SWIGLU_BWD, cap, name + " bwd")
        if pool == "large":
            assert (y[0] == 0).all() and (dgu[0] == 0).all()


def test_swiglu_repeatable_gpu(monkeypatch):
    _set_grid(monkeypatch, 2)
    gu, dy = _inputs(1000, 24, BF16, "unit")
    runs = [(S.swiglu_fwd_hip(gu), S.swiglu_bwd_hip(dy, gu)) for _ in range(3)]
    for y, dgu in runs[1:]:
        assert torch.equal(y, runs[0][0]) and torch.equal(dgu, runs[0][1])


def test_swiglu_binding_errors_gpu():
    ext = _ext.get_ext()
    gu = torch.randn(6, 16, device="cuda", dtype=BF16)
    dy = torch.randn(6, 8, device="cuda", dtype=BF16)
    with pytest.raises(RuntimeError, match="swiglu_fwd"):
        ext.swiglu_fwd(gu[:, :8])               # not contiguous
    with pytest.raises(RuntimeError, match="swiglu_fwd"):
        ext.swiglu_fwd(gu[:, :7].contiguous())  # odd last dim
    with pytest.raises(RuntimeError, match="swiglu_bwd"):
        ext.swiglu_bwd(dy[:5], gu)              # wrong element count
    with pytest.raises(RuntimeError, match="swiglu_bwd"):
        ext.swiglu_bwd(dy.t(), gu)              # not contiguous


def test_swiglu_model_step_gpu(monkeypatch):
    """One bf16 step under Single: the tuner saw swiglu and no gelu, and the
    loss is that of an fp32 CPU copy of the model on the same batch
    (TDSA_AUTOTUNE=0 would run the HIP candidates, not the torch ones)."""
    monkeypatch.delenv("TDSA_AUTOTUNE", raising=False)
    monkeypatch.delenv("TDSA_SWIGLU_GRID", raising=False)
    import tiny_deepspeed_amd.ops.autotuner as at
    monkeypatch.setattr(at, "_DEFAULT_TUNER", None)
    from tiny_deepspeed_amd import Single, AdamW
    from tiny_deepspeed_amd.models import GPTConfig, GPT2Model
    torch.manual_seed(0)
    cfg = GPTConfig(mlp="swiglu", norm="rmsnorm", n_layer=2, n_head=4,
                    n_embd=256, block_size=128, vocab_size=1024)
    model = GPT2Model(cfg).to(BF16)
    ref = copy.deepcopy(model).float()
    x = torch.randint(0, 1024, (2, 128))
    _, loss_ref = ref(x, x)
    wrapped = Single(model.cuda())
    opt = AdamW(wrapped.named_parameters(), lr=1e-4)
    _, loss = wrapped(x.cuda(), x.cuda())
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    tuned = {k[0] for k in at._DEFAULT_TUNER.choices()}
    assert {"swiglu_fwd", "swiglu_bwd"} <= tuned, sorted(tuned)
    assert "gelu_fwd" not in tuned
    print(f"loss {loss.item():.5f} fp32 cpu {loss_ref.item():.5f}")
    assert abs(loss.item() - loss_ref.item()) <= KC.CAP_FWD * abs(loss_ref.item())
