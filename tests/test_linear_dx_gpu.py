"""Linear input gradient through the forward's GEMM layout: the bf16
transpose kernel bit for bit, both dX candidates against fp64, and what
``linear_input_grad`` offers the tuner.
"""

import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tiny_deepspeed_amd.ops import _ext
from tiny_deepspeed_amd.ops.autotuner import RuntimeAutoTuner

linear = importlib.import_module("tiny_deepspeed_amd.ops.linear")

BF16 = torch.bfloat16

# kernel_check's rule: 2 x the largest ratio measured on an MI355X, rounded
# up to a power of two. Largest ratio 1.00 (both candidates, all three
# shapes: the library GEMMs accumulate in fp32 and round once, as plain
# does); the table is in docs/kernels.md ("Test bounds").
K_LINEAR_DX = 2


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


# ---- transpose ---------------------------------------------------------------
@pytest.mark.parametrize("N,K", [
    (64, 64),
    (64, 192),
    (192, 64),
    (320, 448),     # 5 x 7 tiles: odd on both axes, a last workgroup part full
    (50304, 128),   # a long tile axis (the padded vocabulary)
])
def test_transpose_is_exact(N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    # every 16-bit pattern is possible: NaN payloads, infinities, both zeros
    bits = torch.randint(-32768, 32768, (N, K), generator=g, dtype=torch.int16)
    bits[0, 0], bits[-1, -1] = 0, -32768          # +0.0 and -0.0
    bits[0, -1], bits[-1, 0] = 0x7FC1, -63        # NaNs with payloads
    w = bits.view(BF16).cuda()
    before = w.view(torch.int16).clone()
    out = _ext.get_ext().transpose_bf16(w)
    assert out.shape == (K, N) and out.dtype == BF16 and out.is_contiguous()
    want = w.t().contiguous()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.equal(w.view(torch.int16), before), "input was written"


# ---- both candidates against fp64 ---------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 64, 64), (192, 192, 320),
                                   (256, 448, 64)])
def test_dx_candidates_track_fp64(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    dy = torch.randn(M, N, generator=g).to(BF16).cuda()
    w = torch.randn(N, K, generator=g).to(BF16).cuda()
    ref64 = dy.double() @ w.double()
    plain = (dy.float() @ w.float()).to(BF16)
    assert linear._dx_nt_supported(dy, w)
    for fn in (linear.dx_nt, linear.dx_library):
        out = fn(dy, w)
        assert out.shape == (M, K) and out.dtype == BF16
        KC.assert_tracks(out, plain, ref64, -1, K_LINEAR_DX,
                         KC.CAP_POINT_BF16, f"{fn.__name__} {M}x{N}x{K}")


# ---- dispatch ------------------------------------------------------------------
class _RecordingTuner:
    def __init__(self):
        self.calls = []

    def choose(self, op, candidates, *args):
        self.calls.append((op, [c.__name__ for c in candidates], args))
        return candidates[0](*args)


def _forbid_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native dX op was reached")
    monkeypatch.setattr(_ext.get_ext(), "linear_dx_nt", boom)
    monkeypatch.setattr(_ext.get_ext(), "transpose_bf16", boom)


def _dy_w(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(2, M // 2, N, generator=g).to(BF16).cuda()
    w = torch.randn(N, K, generator=g).to(BF16).cuda()
    return dy, w


def test_supported_weight_offers_nt_first():
    dy, w = _dy_w(128, 64, 128)
    tuner = _RecordingTuner()
    dx = linear.linear_input_grad(dy, w, tuner=tuner)
    assert dx.shape == (2, 64, 128)
    (op, names, args), = tuner.calls
    assert op == "linear_dx" and names == ["dx_nt", "dx_library"]
    assert args[0].shape == (128, 64) and args[1] is w
    ref64 = dy.double() @ w.double()
    assert KC.rel_err(dx, ref64, -1)[0] <= KC.CAP_POINT_BF16


@pytest.mark.parametrize("kind", ["k_off_width", "n_off_width", "strided"])
def test_unsupported_weight_stays_on_the_library(monkeypatch, kind):
    if kind == "k_off_width":
        dy, w = _dy_w(128, 64, 96)
    elif kind == "n_off_width":
        dy, w = _dy_w(128, 96, 64)
    else:
        dy, base = _dy_w(128, 64, 128)
        w = base[:, ::2]              # (64, 64), row stride 128
        assert not w.is_contiguous()
    assert not linear._dx_nt_supported(dy.reshape(-1, dy.shape[-1]), w)
    _forbid_native(monkeypatch)
    tuner = _RecordingTuner()
    dx = linear.linear_input_grad(dy, w, tuner=tuner)
    assert [names for _, names, _ in tuner.calls] == [["dx_library"]]
    assert torch.equal(dx, torch.matmul(dy, w))
    # and the same without a tuner in the way
    monkeypatch.setenv("TDSA_AUTOTUNE", "0")
    assert torch.equal(linear.linear_input_grad(dy, w), torch.matmul(dy, w))


def test_env_knob_leaves_the_library_only(monkeypatch):
    monkeypatch.setenv("TDSA_LINEAR_DX", "0")
    _forbid_native(monkeypatch)
    dy, w = _dy_w(128, 64, 128)
    tuner = _RecordingTuner()
    dx = linear.linear_input_grad(dy, w, tuner=tuner)
    assert [names for _, names, _ in tuner.calls] == [["dx_library"]]
    assert torch.equal(dx, torch.matmul(dy, w))


def test_fresh_tuner_records_a_linear_dx_choice(monkeypatch):
    monkeypatch.delenv("TDSA_LINEAR_DX", raising=False)
    tuner = RuntimeAutoTuner(warmup=2, iters=5)
    dy, w = _dy_w(256, 192, 320)
    dx = linear.linear_input_grad(dy, w, tuner=tuner)
    keys = [k for k in tuner.choices() if k[0] == "linear_dx"]
    assert len(keys) == 1, tuner.choices()
    assert tuner.choices()[keys[0]] in ("dx_nt", "dx_library")
    ref64 = dy.double() @ w.double()
    assert KC.rel_err(dx, ref64, -1)[0] <= KC.CAP_POINT_BF16
