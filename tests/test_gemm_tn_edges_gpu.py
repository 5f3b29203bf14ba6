"""TN weight-grad GEMM on edge shapes (M % 64, N % 128 or K % 128 nonzero):
against fp64, bit for bit against the aligned kernel on the zero-padded
problem, no read past row M - 1, and what ``linear_weight_grad`` offers the
tuner.
"""

import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tiny_deepspeed_amd.ops import _ext

linear = importlib.import_module("tiny_deepspeed_amd.ops.linear")

BF16 = torch.bfloat16

# kernel_check's rule: 2 x the largest ratio measured on an MI355X, rounded
# up to a power of two. Largest ratio 1.00 (all nine shapes: kernel and
# library both accumulate in fp32 and sit at the bf16 rounding of the output,
# 3.3e-3 .. 3.8e-3 per row); the table is in docs/kernels.md ("Test bounds").
K_LINEAR_DW = 2


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _dy_x(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    dy = torch.randn(M, N, generator=g).to(BF16).cuda()
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    return dy, x


@pytest.mark.parametrize("M,N,K", [
    (64, 64, 64),        # half tile both ways; waves 2 and 3 idle
    (64, 192, 128),      # N edge on the second tile row
    (64, 128, 192),      # K edge
    (128, 192, 320),     # both edges, two chunks
    (1, 128, 128),       # one row
    (63, 128, 128),      # one chunk, ragged
    (65, 128, 128),      # a full chunk plus one row
    (200, 192, 192),     # everything at once, splits > 1
    (256, 1600, 1600),   # the xl width itself
])
def test_edge_shapes_track_fp64(M, N, K):
    dy, x = _dy_x(M, N, K)
    out = _ext.get_ext().gemm_tn(dy, x)
    assert out.shape == (N, K) and out.dtype == BF16
    ref64 = dy.double().t() @ x.double()
    KC.assert_tracks(out, linear.dw_library(dy, x), ref64, -1, K_LINEAR_DW,
                     1e-2, f"gemm_tn {M}x{N}x{K}")


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("M,N,K", [(100, 192, 192), (63, 64, 320),
                                   (130, 128, 128)])
def test_bits_of_the_padded_aligned_call(monkeypatch, M, N, K, splits):
    # the same chunk ranges in both calls: every element sums the same
    # products in the same order, plus exact zeros
    monkeypatch.setenv("TDSA_GEMM_TN_SPLITS", str(splits))
    dy, x = _dy_x(M, N, K)
    pm, pn, pk = -M % 64, -N % 128, -K % 128
    dy_p, x_p = F.pad(dy, (0, pn, 0, pm)), F.pad(x, (0, pk, 0, pm))
    gemm_tn = _ext.get_ext().gemm_tn
    assert torch.equal(gemm_tn(dy, x), gemm_tn(dy_p, x_p)[:N, :K])


@pytest.mark.parametrize("M,N,K", [(63, 128, 128), (200, 192, 192)])
def test_no_read_past_the_last_row(M, N, K):
    dy, x = _dy_x(M, N, K)
    nan = lambda t: torch.cat([t, torch.full_like(t[:64], float("nan"))])
    dy_big, x_big = nan(dy), nan(x)
    gemm_tn = _ext.get_ext().gemm_tn
    out = gemm_tn(dy_big[:M], x_big[:M])
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, gemm_tn(dy, x))


class _RecordingTuner:
    def __init__(self):
        self.calls = []

    def choose(self, op, candidates, *args):
        self.calls.append((op, [c.__name__ for c in candidates]))
        return candidates[0](*args)


def test_dispatch_offers_the_kernel_on_edge_shapes():
    dy, x = _dy_x(65, 192, 64)
    assert linear._dw_hip_supported(dy, x)
    assert not linear._dw_hip_supported(*_dy_x(65, 96, 64))
    assert not linear._dw_hip_supported(*_dy_x(65, 192, 96))
    dy, x = _dy_x(200, 1600, 1600)
    tuner = _RecordingTuner()
    dw = linear.linear_weight_grad(dy, x, tuner=tuner)
    assert tuner.calls == [("linear_dw", ["dw_hip", "dw_library"])]
    ref64 = dy.double().t() @ x.double()
    assert KC.rel_err(dw, ref64, -1)[0] <= 1e-2
