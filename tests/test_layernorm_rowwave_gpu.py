"""Row-per-wave LayerNorm kernels (bf16, N % 8 == 0, N <= 2048) against fp64
torch on the same inputs, at the shapes where that design can go wrong:
one vector per row, exactly one lane with a second vector, the ragged last
vector of the model widths, the last routed N and the first N handed back to
the workgroup-per-row kernels; fewer rows than waves, and waves that loop
with a ragged final round. Tolerances are the project's own
(tests/test_gpu_kernels.py): 2e-2 of scale forward, 4x that for dx/dw/db,
8e-2 for the fused dx+dh."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.ops import _ext
from tiny_deepspeed_amd.ops import layernorm as L

BF16 = torch.bfloat16
FWD_TOL = 2e-2
BWD_TOL = 8e-2
BOUND = 2048  # asserted against what the extension reports
N_VALUES = [8, 520, 768, 1024, 1280, 1600, BOUND, BOUND + 8]
# small grids for the looping shapes: the loop and its ragged tail are the
# same code at 64 waves as at 2048, at a fraction of the rows
SMALL_WAVES = 64


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _geometry(M, N):
    """(stripes G, fwd waves, fwd depth, bwd depth, bound)."""
    return tuple(_ext.get_ext().layernorm_rowwave_geometry(M, N, True))


def _close(out, ref, tol, name):
    out = out.double()
    err = (out - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1.0)
    print(f"{name}: max err {err:.3e} scale {scale:.3e} tol {tol}")
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    assert err <= tol * scale, f"{name}: max err {err} vs scale {scale} tol {tol}"


def _inputs(M, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g).to(BF16)
    return dict(x=r(M, N), res=r(M, N), w=r(N), b=r(N), dy=r(M, N), dh=r(M, N))


def _reference(t, with_res):
    """fp64 forward and backward of LN(x [+ res]) for upstream grad dy."""
    h = t["x"].double()
    if with_res:
        h = h + t["res"].double()
    h = h.requires_grad_(True)
    w = t["w"].double().requires_grad_(True)
    b = t["b"].double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(h, (h.shape[-1],), w, b)
    y.backward(t["dy"].double())
    mean = h.detach().mean(dim=-1)
    rstd = (h.detach().var(dim=-1, unbiased=False) + 1e-5).rsqrt()
    return dict(h=h.detach(), y=y.detach(), dx=h.grad, dw=w.grad, db=b.grad,
                mean=mean, rstd=rstd)


def _poison_allocator(G, N):
    """Leave NaN behind in freed blocks of the stripe buffers' size, so a
    stripe row the kernel does not write shows up in dw/db."""
    junk = [torch.full((G, N), float("nan"), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    del junk


def _check_shape(M, N, seed, poison=False):
    t = _inputs(M, N, seed)
    tag = f"M={M} N={N}"
    for with_res in (False, True):
        ref = _reference(t, with_res)
        if with_res:
            h, y, mean, rstd = L.ln_fwd_res_hip(t["x"], t["res"], t["w"],
                                                t["b"], 1e-5)
            _close(h, ref["h"], FWD_TOL, f"h {tag}")
        else:
            y, mean, rstd = L.ln_fwd_hip(t["x"], t["w"], t["b"], 1e-5)
            h = t["x"]
        _close(y, ref["y"], FWD_TOL, f"y res={with_res} {tag}")
        _close(mean, ref["mean"], FWD_TOL, f"mean res={with_res} {tag}")
        _close(rstd, ref["rstd"], FWD_TOL, f"rstd res={with_res} {tag}")
        # the backward reads the bf16 h the forward wrote, as the model does
        href = dict(t, x=h)
        bref = _reference(href, False) if with_res else ref
        for with_dh in (False, True):
            if poison:
                _poison_allocator(_geometry(M, N)[0], N)
            dx, ws = L.ln_dx_hip(t["dy"], h, t["w"], mean, rstd,
                                 t["dh"] if with_dh else None)
            dw, db = ops.layernorm_dwdb(ws, dtype=BF16)
            assert ws[0].shape == (_geometry(M, N)[0], N)
            name = f"res={with_res} dh={with_dh} {tag}"
            if with_dh:
                _close(dx, bref["dx"] + t["dh"].double(), BWD_TOL, f"dx+dh {name}")
            else:
                _close(dx, bref["dx"], BWD_TOL, f"dx {name}")
            _close(dw, bref["dw"], BWD_TOL, f"dw {name}")
            _close(db, bref["db"], BWD_TOL, f"db {name}")


def test_bound_and_routing():
    """The routed range is what this file assumes, and the hand-over is
    where it says: depths are reported 0 past the bound and with the knob
    off."""
    G, fw, fd, bd, bound = _geometry(4096, 1024)
    assert bound == BOUND and BOUND >= 2048
    assert fd >= 2 and bd >= 2 and G % 4 == 0 and fw % 4 == 0
    assert _geometry(4096, BOUND)[2] >= 2
    assert _geometry(4096, BOUND + 8)[1:4] == (0, 0, 0)


@pytest.mark.parametrize("N", N_VALUES)
def test_rowwave_small_M(N):
    """M = 1, 3, 5: all waves but one own nothing / fewer rows than one
    workgroup's waves. dw/db must match although the stripe buffers were
    NaN before the call (every stripe row written, zeros included)."""
    for M in (1, 3, 5):
        _check_shape(M, N, seed=100 + M, poison=True)


@pytest.mark.parametrize("N", N_VALUES)
def test_rowwave_looping_M(N, monkeypatch):
    """G*R + 1 and 2*G*R + 3 rows: every wave loops and the final round is
    ragged, for the forward's and the backward's own G and R."""
    monkeypatch.setenv("TDSA_LN_STRIPES", str(SMALL_WAVES))
    monkeypatch.setenv("TDSA_LN_RW_WAVES", str(SMALL_WAVES))
    G, fw, fd, bd, _ = _geometry(1 << 20, N)
    if N <= BOUND:
        assert G == SMALL_WAVES and fw == SMALL_WAVES
    else:  # old path: the same row counts, one row per workgroup
        fw, fd, bd = G, 4, 2
    Ms = sorted({fw * fd + 1, 2 * fw * fd + 3, G * bd + 1, 2 * G * bd + 3})
    for M in Ms:
        _check_shape(M, N, seed=200 + M % 97)


def test_rowwave_default_grid_repeatable():
    """(2*G*R + 3, 1024) at the default launch geometry: correct, and three
    calls of fwd_res, dx+dh and dwdb on the same inputs give the same bits."""
    N = 1024
    G, fw, fd, bd, _ = _geometry(1 << 20, N)
    M = 2 * max(G * bd, fw * fd) + 3
    _check_shape(M, N, seed=7)
    t = _inputs(M, N, seed=8)
    runs = []
    for _ in range(3):
        h, y, mean, rstd = L.ln_fwd_res_hip(t["x"], t["res"], t["w"], t["b"],
                                            1e-5)
        dx, ws = L.ln_dx_hip(t["dy"], h, t["w"], mean, rstd, t["dh"])
        dw, db = ops.layernorm_dwdb(ws, dtype=BF16)
        runs.append((h, y, mean, rstd, dx, ws[0], ws[1], dw, db))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("M,N", [(3, 520), (515, 1024), (131, 8200)])
def test_dwdb_fused_cast(M, N):
    """The reduce kernel's own bf16 rounding equals fp32 output + .to()."""
    t = _inputs(M, N, seed=11)
    y, mean, rstd = L.ln_fwd_hip(t["x"], t["w"], t["b"], 1e-5)
    _, ws = L.ln_dx_hip(t["dy"], t["x"], t["w"], mean, rstd, None)
    dw32, db32 = ops.layernorm_dwdb(ws)
    assert dw32.dtype == torch.float32 and db32.dtype == torch.float32
    dw16, db16 = ops.layernorm_dwdb(ws, dtype=BF16)
    assert dw16.dtype == BF16 and db16.dtype == BF16
    assert torch.equal(dw16, dw32.to(BF16))
    assert torch.equal(db16, db32.to(BF16))
    ref = _reference(t, False)
    _close(dw32, ref["dw"], BWD_TOL, f"dw fp32 M={M} N={N}")
    _close(db32, ref["db"], BWD_TOL, f"db fp32 M={M} N={N}")


def _ulp(v, mant_bits):
    """Spacing of a format with `mant_bits` explicit mantissa bits at |v|."""
    v = v.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - mant_bits)


@pytest.mark.parametrize("M,N", [(5, 520), (515, 1024), (259, 1600)])
def test_old_and_new_paths_side_by_side(M, N, monkeypatch):
    """TDSA_LN_ROWWAVE is read per launch. Only the fp32 summation order
    differs between the paths, so (a) mean/rstd of the new path are at most
    2x as far from fp64 as the old path's on the same input, plus one fp32
    ulp of the value (the old path's own error is what a summation order is
    worth), and (b) y, h and dx differ in the last bf16 bit at most. By
    construction the new path keeps the old one's summation order, so dw/db
    (fp32) are required to be bit-equal on top of that."""
    t = _inputs(M, N, seed=21)
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("TDSA_LN_ROWWAVE", knob)
        assert (_geometry(M, N)[2] > 0) == (knob == "1")
        h, y, mean, rstd = L.ln_fwd_res_hip(t["x"], t["res"], t["w"], t["b"],
                                            1e-5)
        # same mean/rstd into both backwards: isolates the dx kernels
        out[knob] = dict(h=h, y=y, mean=mean, rstd=rstd)
    for knob in ("0", "1"):
        monkeypatch.setenv("TDSA_LN_ROWWAVE", knob)
        o = out["0"]
        out[knob]["dx"], ws = L.ln_dx_hip(t["dy"], o["h"], t["w"], o["mean"],
                                          o["rstd"], t["dh"])
        out[knob]["dw"], out[knob]["db"] = ops.layernorm_dwdb(ws)
    for k in ("mean", "rstd"):
        # reference statistics of the bf16 h the kernels normalise
        hq = out["0"]["h"].double()
        r = hq.mean(-1) if k == "mean" else (hq.var(-1, unbiased=False) + 1e-5).rsqrt()
        e_old = (out["0"][k].double() - r).abs().max().item()
        e_new = (out["1"][k].double() - r).abs().max().item()
        ulp = _ulp(r, 23).max().item()
        print(f"{k} M={M} N={N}: old err {e_old:.3e} new err {e_new:.3e} ulp {ulp:.3e}")
        assert e_new <= 2 * e_old + ulp, (k, e_old, e_new, ulp)
    assert torch.equal(out["0"]["h"], out["1"]["h"])
    # wave g accumulates the rows, in the order and with the expression, that
    # stripe g of the old path did, and the stripe reduce is shared
    assert torch.equal(out["0"]["dw"], out["1"]["dw"])
    assert torch.equal(out["0"]["db"], out["1"]["db"])
    for k in ("y", "h", "dx"):
        a, b = out["0"][k].double(), out["1"][k].double()
        d = (a - b).abs()
        lim = _ulp(torch.maximum(a.abs(), b.abs()), 7)
        worst = (d / lim).max().item()
        print(f"{k} M={M} N={N}: max |d| {d.max().item():.3e} = {worst:.2f} bf16 ulp")
        assert (d <= lim).all(), (k, worst)
