"""RMSNorm HIP kernels (bf16, N % 8 == 0, N <= 8192) against fp64 torch on
the same bf16 inputs, at the shapes where the design can go wrong: one vector
per row, exactly one lane with a second vector, ragged last vectors at model
widths, the last wave-per-row width and the first workgroup-per-row width
(2056: a single thread with a second vector), the Llama widths and the bound;
fewer rows than units, and units that loop with a ragged final round (the
case that catches a wrong LDS slot alternation). Tolerances are the project's
own (tests/test_gpu_kernels.py): 2e-2 of scale forward, 8e-2 backward."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.ops import _ext
from tiny_deepspeed_amd.ops import rmsnorm as R

BF16 = torch.bfloat16
FWD_TOL = 2e-2
BWD_TOL = 8e-2
EPS = 1e-5
N_VALUES = [8, 520, 768, 1600, 2048, 2056, 4096, 5120, 8192]
SMALL_UNITS = 64  # waves: 64 wave-per-row units, 16 workgroup-per-row units


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _geometry(M, N, bf16=True):
    """(stripes G, fwd units, fwd depth, bwd depth, span, bound)."""
    return tuple(_ext.get_ext().rmsnorm_geometry(M, N, bf16))


def _close(out, ref, tol, name):
    out = out.double()
    err = (out - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1.0)
    print(f"{name}: max err {err:.3e} scale {scale:.3e} tol {tol}")
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    assert err <= tol * scale, f"{name}: max err {err} vs scale {scale} tol {tol}"


def _inputs(M, N, seed, dtype=BF16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g).to(dtype)
    return dict(x=r(M, N), res=r(M, N), w=r(N), dy=r(M, N), dh=r(M, N))


def _reference(h, w, dy):
    """fp64 forward and backward of RMSNorm(h) for upstream grad dy."""
    h = h.double().clone().requires_grad_(True)
    w = w.double().requires_grad_(True)
    rstd = (h.square().mean(dim=-1) + EPS).rsqrt()
    y = h * rstd.unsqueeze(-1) * w
    y.backward(dy.double())
    return dict(y=y.detach(), rstd=rstd.detach(), dx=h.grad, dw=w.grad)


def _poison_allocator(G, N):
    """Leave NaN behind in freed blocks of the stripe buffer's size, so a
    stripe row the kernel does not write shows up in dw."""
    junk = [torch.full((G, N), float("nan"), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    del junk


def _check_shape(M, N, seed, poison=False):
    t = _inputs(M, N, seed)
    tag = f"M={M} N={N}"
    for with_res in (False, True):
        if with_res:
            h, y, rstd = R.rms_fwd_res_hip(t["x"], t["res"], t["w"], EPS)
            href = t["x"].double() + t["res"].double()
            _close(h, href, FWD_TOL, f"h {tag}")
            fref = _reference(href, t["w"], t["dy"])
        else:
            y, rstd = R.rms_fwd_hip(t["x"], t["w"], EPS)
            h = t["x"]
        # the backward reads the bf16 h the forward wrote, as the model does
        ref = _reference(h, t["w"], t["dy"])
        if not with_res:
            fref = ref
        _close(y, fref["y"], FWD_TOL, f"y res={with_res} {tag}")
        _close(rstd, fref["rstd"], FWD_TOL, f"rstd res={with_res} {tag}")
        for with_dh in (False, True):
            if poison:
                _poison_allocator(_geometry(M, N)[0], N)
            dx, ws = R.rms_dx_hip(t["dy"], h, t["w"], rstd,
                                  t["dh"] if with_dh else None)
            dw = ops.rmsnorm_dw(ws, dtype=BF16)
            assert ws[0].shape == (_geometry(M, N)[0], N)
            name = f"res={with_res} dh={with_dh} {tag}"
            if with_dh:
                _close(dx, ref["dx"] + t["dh"].double(), BWD_TOL, f"dx+dh {name}")
            else:
                _close(dx, ref["dx"], BWD_TOL, f"dx {name}")
            _close(dw, ref["dw"], BWD_TOL, f"dw {name}")


@pytest.mark.parametrize("N", N_VALUES)
def test_small_M(N):
    """M = 1, 3, 5: most units own nothing. dw must match although the
    stripe buffer was NaN before the call (every row written, zeros too)."""
    for M in (1, 3, 5):
        _check_shape(M, N, seed=100 + M, poison=True)


@pytest.mark.parametrize("N", N_VALUES)
def test_looping_M(N, monkeypatch):
    """units*depth + 1 and 2*units*depth + 3 rows: every unit loops and the
    final round is ragged, for the forward's and the backward's geometry."""
    monkeypatch.setenv("TDSA_LN_STRIPES", str(SMALL_UNITS))
    monkeypatch.setenv("TDSA_LN_RW_WAVES", str(SMALL_UNITS))
    G, fu, fd, bd, span, _ = _geometry(1 << 20, N)
    assert G == fu == SMALL_UNITS // span
    Ms = sorted({fu * fd + 1, 2 * fu * fd + 3, G * bd + 1, 2 * G * bd + 3})
    for M in Ms:
        _check_shape(M, N, seed=200 + M % 97)


@pytest.mark.parametrize("N", [1024, 4096])
def test_default_grid_repeatable(N):
    """(2*G*R + 3, N) at the default geometry, one shape per span: three
    calls of fwd_res, dx+dh and the reduce give the same bits."""
    G, fu, fd, bd, _, _ = _geometry(1 << 20, N)
    M = 2 * max(G * bd, fu * fd) + 3
    t = _inputs(M, N, seed=8)
    runs = []
    for _ in range(3):
        h, y, rstd = R.rms_fwd_res_hip(t["x"], t["res"], t["w"], EPS)
        dx, ws = R.rms_dx_hip(t["dy"], h, t["w"], rstd, t["dh"])
        runs.append((h, y, rstd, dx, ws[0], ops.rmsnorm_dw(ws, dtype=BF16)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    ref = _reference(runs[0][0], t["w"], t["dy"])
    _close(runs[0][1], ref["y"], FWD_TOL, f"y N={N}")
    _close(runs[0][3], ref["dx"] + t["dh"].double(), BWD_TOL, f"dx+dh N={N}")
    _close(runs[0][5], ref["dw"], BWD_TOL, f"dw N={N}")


@pytest.mark.parametrize("M,N", [(3, 520), (515, 1024), (131, 8192)])
def test_reduce_cast(M, N):
    """The reduce kernel's own bf16 rounding equals fp32 output + .to()."""
    t = _inputs(M, N, seed=11)
    y, rstd = R.rms_fwd_hip(t["x"], t["w"], EPS)
    _, ws = R.rms_dx_hip(t["dy"], t["x"], t["w"], rstd, None)
    dw32 = ops.rmsnorm_dw(ws)
    dw16 = ops.rmsnorm_dw(ws, dtype=BF16)
    assert dw32.dtype == torch.float32 and dw16.dtype == BF16
    assert torch.equal(dw16, dw32.to(BF16))
    _close(dw32, _reference(t["x"], t["w"], t["dy"])["dw"], BWD_TOL,
           f"dw fp32 M={M} N={N}")


def test_routing():
    """Span 1 / 4 / 0 at N = 2048 / 2056 / 8200 and 0 for fp32; the op layer
    still answers unrouted shapes, through the composite."""
    assert _geometry(64, 2048)[4] == 1
    assert _geometry(64, 2056)[4] == 4
    assert _geometry(64, 8192)[4:] == (4, 8192)
    assert _geometry(64, 8200) == (0,) * 6
    assert _geometry(64, 1024, bf16=False) == (0,) * 6
    for N, dtype in ((8200, BF16), (1024, torch.float32)):
        t = _inputs(5, N, seed=31, dtype=dtype)
        y, rstd = ops.rmsnorm_fwd(t["x"], t["w"], EPS)
        ref = _reference(t["x"], t["w"], t["dy"])
        _close(y, ref["y"], FWD_TOL, f"y composite N={N}")
        _close(rstd, ref["rstd"], FWD_TOL, f"rstd composite N={N}")
        with pytest.raises(RuntimeError, match="rmsnorm_fwd"):
            R.rms_fwd_hip(t["x"], t["w"], EPS)
