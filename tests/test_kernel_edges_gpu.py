"""Pointwise and reduction HIP kernels, called through their ``*_hip``
functions (never the tuner), at the widths, row counts and values where
they take another path: cross-entropy, GELU, column sum, embedding. fp64
references, the project's torch candidates as the plain baseline, slices and
bounds from tests/kernel_check.py. Both dtypes wherever the kernel has both.
"""

import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tiny_deepspeed_amd.ops import _ext

ce = importlib.import_module("tiny_deepspeed_amd.ops.cross_entropy")
emb = importlib.import_module("tiny_deepspeed_amd.ops.embedding")
gelu = importlib.import_module("tiny_deepspeed_amd.ops.gelu")
linear = importlib.import_module("tiny_deepspeed_amd.ops.linear")

BF16 = torch.bfloat16
F32 = torch.float32
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


# ---- cross-entropy -----------------------------------------------------------
def _ce_case(R, V, dtype, name, **kind):
    """Forward and backward of one input through ce_fwd_hip/ce_bwd_hip."""
    cap = KC.CAP_FWD if dtype == BF16 else KC.CAP_F32
    logits, tgt = KC.ce_inputs(R, V, dtype, "cuda", **kind)
    lse64, loss64, n64, d64 = KC.ce_ref64(logits, tgt)
    assert torch.isfinite(lse64).all()

    loss, lse, n = ce.ce_fwd_hip(logits, tgt, KC.IGNORE)
    loss_p, lse_p, _ = ce.ce_fwd_torch(logits, tgt, KC.IGNORE)
    assert n.dtype == torch.int64 and int(n) == n64, (int(n), n64)
    KC.assert_tracks(lse, lse_p, lse64, None, KC.K_CE, KC.CAP_F32, name + " lse")
    KC.assert_tracks(loss, loss_p, loss64, None, KC.K_CE, KC.CAP_F32,
                     name + " loss", plain_floor=KC.U_F32)

    # dlogits into a row-slice of a larger NaN-filled buffer
    buf = torch.full((R + 5, V), NAN, device="cuda", dtype=dtype)
    d = ce.ce_bwd_hip(1.0, logits, tgt, lse, n, KC.IGNORE, out=buf[2:R + 2])
    assert d.data_ptr() == buf[2:R + 2].data_ptr()
    assert torch.isnan(buf[:2]).all() and torch.isnan(buf[R + 2:]).all(), \
        "rows outside the slice were written"
    d_p = ce.ce_bwd_torch(1.0, logits, tgt, lse_p, n, KC.IGNORE)
    KC.assert_tracks(d, d_p, d64, -1, KC.K_CE, cap, name + " dlogits")
    ignored = tgt == KC.IGNORE
    assert (d[ignored] == 0).all(), "ignored rows must be exactly zero"
    assert torch.equal(ce.ce_bwd_hip(1.0, logits, tgt, lse, n, KC.IGNORE), d)
    return loss, n, d


CE_KINDS = {
    "x3": dict(scale=3.0),
    # the running max changes often
    "x30": dict(scale=30.0),
    # masked vocabulary padding, and one row with a single finite column
    "neginf_tail": dict(scale=3.0, neg_inf_tail=True),
}


# widths: one thread has data and 255 merge (-inf, 0) states; exactly one
# chunk per thread; one thread has two chunks
@pytest.mark.parametrize("R", [1, 5, 300])
@pytest.mark.parametrize("dtype,V", [(BF16, 8), (BF16, 2048), (BF16, 2056),
                                     (F32, 4), (F32, 1024), (F32, 1028)])
@pytest.mark.parametrize("kind", list(CE_KINDS))
def test_cross_entropy_edges_gpu(dtype, V, R, kind, monkeypatch):
    if R == 300:
        # 64 blocks loop over 300 rows: four full rounds and a ragged fifth
        monkeypatch.setenv("TDSA_CE_GRID", "64")
    _ce_case(R, V, dtype, f"ce {kind} R{R} V{V}", **CE_KINDS[kind])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("kind", ["x3", "neginf_tail"])
def test_cross_entropy_vocab_width_gpu(dtype, kind):
    _ce_case(8, 50304, dtype, f"ce {kind} R8 V50304", **CE_KINDS[kind])


@pytest.mark.parametrize("dtype,V", [(BF16, 2056), (F32, 1028)])
@pytest.mark.parametrize("R", [1, 5, 300])
def test_cross_entropy_all_rows_ignored_gpu(dtype, V, R, monkeypatch):
    if R == 300:
        monkeypatch.setenv("TDSA_CE_GRID", "64")
    loss, n, d = _ce_case(R, V, dtype, f"ce all-ignored R{R} V{V}",
                          all_ignored=True)
    assert int(n) == 0 and loss.item() == 0.0
    assert (d == 0).all()


# ---- GELU --------------------------------------------------------------------
# n: tail-only launches (1, 7), body only (8), body + tail (9, 2048*8+5)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2048 * 8 + 5])
@pytest.mark.parametrize("dtype,cap", [(BF16, KC.CAP_POINT_BF16),
                                       (F32, KC.CAP_GELU_F32)])
def test_gelu_edges_gpu(dtype, cap, n):
    for pool in KC.gelu_pools():
        x, dy = KC.gelu_inputs(n, dtype, "cuda", pool)
        y64, dx64 = KC.gelu_ref64(x, dy)
        name = f"gelu {pool} n{n}"
        KC.assert_tracks(gelu.gelu_fwd_hip(x), gelu.gelu_fwd_torch(x), y64, 0,
                         KC.K_GELU_FWD, cap, name + " fwd")
        KC.assert_tracks(gelu.gelu_bwd_hip(dy, x), gelu.gelu_bwd_torch(dy, x),
                         dx64, 0, KC.K_GELU_BWD, cap, name + " bwd")


# ---- column sum --------------------------------------------------------------
# one chunk; several chunks with a ragged last one; N no multiple of the block
@pytest.mark.parametrize("M,N", [(1, 8), (129, 257), (4097, 2304), (1000, 33)])
@pytest.mark.parametrize("dtype,cap", [(BF16, KC.CAP_POINT_BF16),
                                       (F32, KC.CAP_F32)])
def test_column_sum_edges_gpu(dtype, cap, M, N):
    dy = KC.colsum_inputs(M, N, dtype, "cuda")
    out = linear.db_hip(dy)
    assert out.shape == (N,) and out.dtype == dtype
    KC.assert_tracks(out, linear.db_torch(dy), dy.double().sum(dim=0), 0,
                     KC.K_COLSUM, cap, f"colsum {M}x{N}")


# ---- embedding ---------------------------------------------------------------
# D = 12 takes the scalar path in bf16 (12 % 8 != 0), the vector path in fp32;
# D = 6 the scalar path in both (6 % 4 != 0)
@pytest.mark.parametrize("D", [6, 8, 12, 768])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_embedding_fwd_edges_gpu(dtype, D):
    V = 97
    g = torch.Generator().manual_seed(D)
    w = torch.randn(V, D, generator=g).to(dtype).cuda()
    idx = torch.randint(0, V, (3, 50), generator=g)
    idx[0, 0], idx[0, 1], idx[2, 49], idx[1, 7] = 0, V - 1, V - 1, 0
    idx = idx.cuda()
    out = emb.emb_fwd_hip(w, idx)
    assert out.shape == (3, 50, D) and out.dtype == dtype
    assert torch.equal(out, w[idx])       # a gather is exact
    assert torch.equal(out, emb.emb_fwd_torch(w, idx))


@pytest.mark.parametrize("D", [12, 264])
@pytest.mark.parametrize("dtype,cap", [(BF16, KC.CAP_POINT_BF16),
                                       (F32, KC.CAP_F32)])
def test_embedding_bwd_edges_gpu(dtype, cap, D):
    for name, (idx, pad) in KC.emb_bwd_cases("cuda").items():
        dy = KC.emb_dy(idx.numel(), D, dtype, "cuda")
        ref = KC.emb_bwd_ref64(idx, dy, KC.EMB_V, pad)
        out = emb.emb_bwd_hip(idx, dy, KC.EMB_V, pad)
        assert out.shape == (KC.EMB_V, D) and out.dtype == dtype
        KC.assert_tracks(out, emb.emb_bwd_torch(idx, dy, KC.EMB_V, pad), ref,
                         -1, KC.K_EMB, cap, f"emb bwd {name} D{D}")
        hit = torch.zeros(KC.EMB_V, dtype=torch.bool, device="cuda")
        hit[idx] = True
        if pad is not None:
            hit[pad] = False
        assert (out[~hit] == 0).all(), "rows never indexed must be exactly zero"
        assert (ref[hit].abs().amax(dim=-1) > 0).all()
