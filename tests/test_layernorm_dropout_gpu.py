"""Residual dropout fused into the row-per-wave LayerNorm kernels: the mask is
exactly ops.dropout_keep_mask, and every output matches fp64 autograd of
LN(x + mask * res / (1 - p)) on the same inputs. Shapes: one vector per row,
exactly one lane with a second vector, 768, the ragged fourth vector, the last
routed width; fewer rows than a workgroup's waves, and 64 waves that loop with
a ragged last batch. Tolerances are tests/test_layernorm_rowwave_gpu.py's."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.modules.normalization import LayerNorm
from tiny_deepspeed_amd.ops import _ext
from tiny_deepspeed_amd.ops.attention import _draw_seed

BF16 = torch.bfloat16
FWD_TOL = 2e-2
BWD_TOL = 8e-2
P = 0.3
SEEDS = [12345, (1 << 40) + 977]
N_VALUES = [8, 520, 768, 1600, 2048]
SMALL_WAVES = 64
# 64 waves at batch depth 4 (forward, N <= 1024) or 2: three full rounds of
# either plus a ragged one
M_VALUES = [3, 3 * SMALL_WAVES * 4 + 5]


@pytest.fixture(autouse=True)
def _small_grid(monkeypatch):
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"
    monkeypatch.setenv("TDSA_LN_STRIPES", str(SMALL_WAVES))
    monkeypatch.setenv("TDSA_LN_RW_WAVES", str(SMALL_WAVES))


def _close(out, ref, tol, name):
    out = out.double()
    err = (out - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1.0)
    print(f"{name}: max err {err:.3e} scale {scale:.3e} tol {tol}")
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    assert err <= tol * scale, f"{name}: max err {err} vs scale {scale} tol {tol}"


def _poison(M, N):
    """NaN in freed blocks of the outputs' and the stripes' sizes, so an
    unwritten dres element or stripe row shows."""
    junk = [torch.full((M, N), float("nan"), device="cuda", dtype=BF16)
            for _ in range(2)]
    junk += [torch.full((SMALL_WAVES, N), float("nan"), device="cuda")
             for _ in range(2)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("N", N_VALUES)
@pytest.mark.parametrize("M", M_VALUES)
def test_mask_exact(M, N, seed):
    keep = ops.dropout_keep_mask(M, N, P, seed, "cuda")
    zero = torch.zeros(M, N, device="cuda", dtype=BF16)
    one = torch.ones_like(zero)
    # 1 / (1 - p) from the fp32 p, as fp32, rounded to bf16 once
    inv_keep = torch.tensor(1.0 / (1.0 - torch.tensor(P).item())).to(BF16)
    want = torch.where(keep, inv_keep.cuda(), zero)
    w, b = one[0].clone(), zero[0].clone()
    h, _, mean, rstd = ops.layernorm_fwd_res_dropout(zero, one, w, b, P, seed)
    assert torch.equal(h, want)
    # dy = 0, dh = 1: dx = 1 everywhere, dres is the pattern again
    _poison(M, N)
    dx, dres, _ = ops.layernorm_dx_dropout(zero, h, w, mean, rstd, one, P, seed)
    assert torch.equal(dx, one)
    assert torch.equal(dres, want)


@pytest.mark.parametrize("with_dh", [False, True])
@pytest.mark.parametrize("N", N_VALUES)
@pytest.mark.parametrize("M", M_VALUES)
def test_values(M, N, with_dh):
    seed = SEEDS[(M + N // 8) % 2]
    g = torch.Generator(device="cuda").manual_seed(M + N)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g).to(BF16)
    x, res, w, b, dy = r(M, N), r(M, N), r(N), r(N), r(M, N)
    dh = r(M, N) if with_dh else None
    keep = ops.dropout_keep_mask(M, N, P, seed, "cuda")

    def reference(x_in, res_in):
        """fp64 autograd of LN(x + keep * res / (1 - p)), h's own grad dh."""
        xd, rd, wd, bd = (t.double().requires_grad_(True)
                          for t in (x_in, res_in, w, b))
        hd = xd + keep * rd / (1.0 - P)
        yd = torch.nn.functional.layer_norm(hd, (N,), wd, bd)
        out = (yd * dy.double()).sum()
        if with_dh:
            out = out + (hd * dh.double()).sum()
        out.backward()
        return hd.detach(), yd.detach(), xd.grad, rd.grad, wd.grad, bd.grad

    h, y, mean, rstd = ops.layernorm_fwd_res_dropout(x, res, w, b, P, seed)
    hd, yd, *_ = reference(x, res)
    tag = f"M={M} N={N} dh={with_dh}"
    _close(h, hd, FWD_TOL, f"h {tag}")
    _close(y, yd, FWD_TOL, f"y {tag}")
    _close(mean, hd.mean(-1), FWD_TOL, f"mean {tag}")
    _close(rstd, (hd.var(-1, unbiased=False) + 1e-5).rsqrt(), FWD_TOL, f"rstd {tag}")
    # the backward reads the bf16 h the forward wrote, as the model does:
    # its reference is the same function at (h, 0)
    _, _, dxd, dresd, dwd, dbd = reference(h, torch.zeros_like(h))
    _poison(M, N)
    dx, dres, ws = ops.layernorm_dx_dropout(dy, h, w, mean, rstd, dh, P, seed)
    dw, db = ops.layernorm_dwdb(ws, dtype=BF16)
    _close(dx, dxd, BWD_TOL, f"dx {tag}")
    _close(dres, dresd, BWD_TOL, f"dres {tag}")
    _close(dw, dwd, BWD_TOL, f"dw {tag}")
    _close(db, dbd, BWD_TOL, f"db {tag}")
    assert (dres[~keep] == 0).all()


def _module(N, dtype):
    torch.manual_seed(0)
    ln = LayerNorm(N, device="cuda", dtype=dtype)
    with torch.no_grad():
        ln.weight.normal_()
        ln.bias.normal_()
    return ln


def test_module_draws_the_seed_and_matches_the_op():
    M, N, s = 37, 768, 4321
    ln = _module(N, BF16)
    x, res = (torch.randn(M, N, device="cuda").to(BF16) for _ in range(2))
    torch.manual_seed(s)
    seed = _draw_seed()
    torch.manual_seed(s)
    h, y = ln.train().forward_fused(x, res, dropout_p=P)
    h_op, y_op, _, _ = ops.layernorm_fwd_res_dropout(x, res, ln.weight, ln.bias,
                                                     P, seed, eps=ln.eps)
    assert torch.equal(h, h_op) and torch.equal(y, y_op)
    h0, y0 = ln.forward_fused(x, res)
    for got in (ln.forward_fused(x, res, dropout_p=0.0),
                ln.eval().forward_fused(x, res, dropout_p=P)):
        assert torch.equal(got[0], h0) and torch.equal(got[1], y0)


@pytest.mark.parametrize("N,dtype", [(2056, BF16), (768, torch.float32)])
def test_module_unrouted_shape_takes_the_replica_mask(N, dtype):
    M, s = 5, 99
    ln = _module(N, dtype).train()
    x = torch.zeros(M, N, device="cuda", dtype=dtype)
    res = torch.ones_like(x).requires_grad_(True)
    torch.manual_seed(s)
    seed = _draw_seed()
    torch.manual_seed(s)
    h, y = ln.forward_fused(x, res, dropout_p=P)
    keep = ops.dropout_keep_mask(M, N, P, seed, "cuda")
    assert torch.equal(h != 0, keep)
    h.sum().backward()  # y unused: the gradient reaches res through h alone
    assert torch.equal(res.grad != 0, keep)
