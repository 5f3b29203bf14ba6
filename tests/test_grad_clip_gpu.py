"""Gradient clipping on the MI355X: the multi-tensor sum-of-squares kernel
(csrc/kernels/gradnorm.hip), the gradient scale of the fused update kernel,
the clipped optimizers end to end and the norm all-reduce through RCCL.

The kernel cases reuse the carved layout of tests/test_gpu_kernels.py: every
view is followed by guard elements of -7.0, whose square is 49, so any read
past a view shows in an otherwise exact sum."""

import os

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

from tests import kernel_check as kc
from tests.dist_utils import free_port
from tests.test_gpu_kernels import (_Carved, _OPT_CHUNK, _OPT_GUARD,
                                    _adamw_ref64, _sgd_ref64)
from tiny_deepspeed_amd import AdamW, SGD, ops
from tiny_deepspeed_amd.ops import _ext

BF16, F32 = torch.bfloat16, torch.float32
C = _OPT_CHUNK
NUMELS = [1, 3, 4, 7, 8, 9, C, C + 5, 2 * C + 4]
TOTAL = sum(NUMELS)  # 262185 < 2^24: exact in fp32
LAYOUTS = ["bf16", "fp32", "mixed"]

# sqrt(sum of squares) against fp64, relative to the ops-layer torch formula
# on the GPU floored at one fp32 rounding: twice the largest ratio measured
# on the MI355X, rounded up to a power of two (docs/kernels.md "Test bounds").
K_SUMSQ = 4  # largest ratio 1.36 (bf16: 8.1e-8 against the credited 2^-24)


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"


def _dtypes(layout, n):
    if layout == "mixed":
        return [BF16 if i % 2 == 0 else F32 for i in range(n)]
    return [BF16 if layout == "bf16" else F32] * n


class _Grads:
    """One carved flat buffer per dtype; view i comes from the buffer of its
    dtype. fill: "ones", "zeros" or a generator (randn)."""

    def __init__(self, numels, layout, fill):
        self.lay = _Carved(numels)
        self.flats = {}
        for dt in sorted(set(_dtypes(layout, len(numels))), key=str):
            if isinstance(fill, str):
                data = torch.full((self.lay.total,),
                                  1.0 if fill == "ones" else 0.0,
                                  device="cuda")
                flat = torch.where(self.lay.mask, data,
                                   torch.full_like(data, _OPT_GUARD)).to(dt)
            else:
                flat, _ = self.lay.stream(dt, fill)
            self.flats[dt] = flat
        self.views = [
            self.flats[dt][o:o + n] for dt, o, n in
            zip(_dtypes(layout, len(numels)), self.lay.offsets, numels)]
        self.before = {dt: f.clone() for dt, f in self.flats.items()}

    def check_untouched(self, name):
        for dt, f in self.flats.items():
            self.lay.check_guards(f, f"{name} {dt}")
            assert torch.equal(f, self.before[dt]), f"{name}: input written"


def _sumsq(views):
    out = _ext.get_ext().grad_sumsq_multi(views)
    assert out.dim() == 0 and out.dtype == F32 and out.is_cuda
    return out


# ---- 5. exact cases --------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sumsq_all_ones_exact_gpu(layout):
    g = _Grads(NUMELS, layout, "ones")
    assert _sumsq(g.views).item() == float(TOTAL)
    g.check_untouched(f"ones {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sumsq_one_hot_positions_gpu(layout):
    """A single 1.0 at the first, last, last-vector-start and chunk-boundary
    positions of every tensor in turn: a dropped tail or chunk gives 0, a
    boundary element counted twice gives 2."""
    g = _Grads(NUMELS, layout, "zeros")
    results = []
    for i, n in enumerate(NUMELS):
        for pos in sorted({0, n - 1, (n - 1) // 4 * 4, C - 1, C}):
            if pos >= n:
                continue
            g.views[i][pos] = 1.0
            results.append(((n, pos), _sumsq(g.views)))
            g.views[i][pos] = 0.0
    for where, r in results:
        assert r.item() == 1.0, (layout, where, r.item())
    g.check_untouched(f"one-hot {layout}")


# ---- 6. shapes of the launch -----------------------------------------------
def test_sumsq_more_chunks_than_workgroups_gpu():
    numels = [i % 9 + 1 for i in range(2100)]  # 2100 chunks, grid of 2048
    g = _Grads(numels, "mixed", "ones")
    assert _sumsq(g.views).item() == float(sum(numels))
    g.check_untouched("grid stride")


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_sumsq_zero_numel_entry_gpu(dtype):
    g = _Grads(NUMELS, "mixed", "ones")
    empty = torch.empty(0, dtype=dtype, device="cuda")
    views = g.views[:3] + [empty] + g.views[3:] + [empty]
    assert _sumsq(views).item() == float(TOTAL)
    assert _sumsq([empty]).item() == 0.0
    assert ops.grad_sumsq([empty], device="cuda").item() == 0.0
    with pytest.raises(RuntimeError, match="empty gradient list"):
        _ext.get_ext().grad_sumsq_multi([])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("n", [1, 5, 9, C + 5, 2 * C + 4])
def test_sumsq_unaligned_view_gpu(dtype, n):
    """A view at element offset 1 of an aligned buffer: 2 or 4 bytes off the
    16-byte grid. Guards on both sides."""
    flat = torch.full((n + 16,), _OPT_GUARD, dtype=dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + n]
    view.fill_(1.0)
    assert view.data_ptr() % 16 == flat.element_size()
    assert _sumsq([view]).item() == float(n)
    # next to an aligned tensor in the same launch
    other = torch.ones(C + 3, dtype=F32, device="cuda")
    assert _sumsq([other, view]).item() == float(n + C + 3)


# ---- 7/8. determinism and accuracy -----------------------------------------
@pytest.fixture(scope="module")
def randn_grads():
    gen = torch.Generator(device="cuda").manual_seed(7)
    return {layout: _Grads(NUMELS, layout, gen) for layout in LAYOUTS}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sumsq_repeats_bitwise_gpu(layout, randn_grads):
    views = randn_grads[layout].views
    a, b = _sumsq(views), _sumsq(views)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sumsq_norm_tracks_fp64_gpu(layout, randn_grads):
    views = randn_grads[layout].views
    ref64 = sum(v.double().pow(2).sum() for v in views).sqrt()
    plain = torch.zeros((), dtype=F32, device="cuda")
    for v in views:  # ops.grad_sumsq's torch branch, evaluated on the GPU
        plain = plain + v.float().pow(2).sum()
    kc.assert_tracks(ops.grad_sumsq(views).sqrt(), plain.sqrt(), ref64, None,
                     K_SUMSQ, kc.CAP_F32, f"grad norm {layout}",
                     plain_floor=kc.U_F32)


# ---- 9. non-finite values --------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_sumsq_propagates_non_finite_gpu(layout, bad):
    g = _Grads(NUMELS, layout, "ones")
    for i, pos in ((0, 0), (7, C + 4), (8, C)):  # tail, tail, vector body
        keep = g.views[i][pos].clone()
        g.views[i][pos] = bad
        r = _sumsq(g.views).item()
        g.views[i][pos] = keep
        if bad != bad:
            assert r != r, (layout, i, pos, r)
        else:
            assert r == float("inf"), (layout, i, pos, r)


# ---- 10. gradient scale in the update kernel --------------------------------
_OPT_DTYPES = [(BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32)]


def _scale(x):
    return torch.tensor(x, dtype=F32, device="cuda")


def _adamw_streams(pdt, gdt):
    lay = _Carved(NUMELS)
    gen = torch.Generator(device="cuda").manual_seed(11)
    s = {"p": lay.stream(pdt, gen), "g": lay.stream(gdt, gen),
         "m": lay.stream(F32, gen), "v": lay.stream(F32, gen, absolute=True),
         "vmax": lay.stream(F32, gen, absolute=True)}
    return lay, s


def _clone_streams(lay, s):
    out = {}
    for k, (flat, _) in s.items():
        f = flat.clone()
        out[k] = (f, [f[o:o + n] for o, n in zip(lay.offsets, lay.numels)])
    return out


def _with_master(lay, s, pdt):
    if pdt != BF16:
        return None, [None] * len(lay.numels)
    wf = s["p"][0].float().clone()
    return wf, [wf[o:o + n] for o, n in zip(lay.offsets, lay.numels)]


def _call_adamw(lay, s, pdt, amsgrad, hyper, grad_scale):
    wf, ws = _with_master(lay, s, pdt)
    n = len(lay.numels)
    args = (s["p"][1], s["g"][1], s["m"][1], s["v"][1], ws,
            s["vmax"][1] if amsgrad else [None] * n, *hyper)
    if grad_scale is None:
        _ext.get_ext().adamw_step_multi(*args)
    else:
        _ext.get_ext().adamw_step_multi(*args, grad_scale)
    return wf


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("pdt,gdt", _OPT_DTYPES)
def test_adamw_grad_scale_gpu(pdt, gdt, amsgrad):
    lay, s = _adamw_streams(pdt, gdt)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.01, 3)
    gs = _scale(0.37)
    rp, rm, rv, rx = _adamw_ref64(
        s["p"][0].double(), gs.double() * s["g"][0].double(),
        s["m"][0].double(), s["v"][0].double(),
        s["vmax"][0].double() if amsgrad else None, *hyper)
    g0, x0 = s["g"][0].clone(), s["vmax"][0].clone()
    wf = _call_adamw(lay, s, pdt, amsgrad, hyper, gs)
    name = f"adamw scaled {pdt}/{gdt} ams={amsgrad}"
    for k, (flat, _) in s.items():
        lay.check_guards(flat, f"{name} {k}")
    assert torch.equal(s["g"][0], g0), f"{name}: gradient written"
    assert gs.item() == _scale(0.37).item()
    lay.close(s["m"][0], rm, f"{name} m")
    lay.close(s["v"][0], rv, f"{name} v")
    if amsgrad:
        lay.close(s["vmax"][0], rx, f"{name} vmax")
    else:
        assert torch.equal(s["vmax"][0], x0)
    if wf is not None:
        lay.check_guards(wf, f"{name} master")
        lay.close(wf, rp, f"{name} master")
        assert torch.equal(s["p"][0][lay.mask], wf.to(BF16)[lay.mask])
    else:
        lay.close(s["p"][0], rp, f"{name} p")


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("pdt,gdt", _OPT_DTYPES)
def test_adamw_unit_grad_scale_is_bitwise_noop_gpu(pdt, gdt, amsgrad):
    lay, s1 = _adamw_streams(pdt, gdt)
    s2 = _clone_streams(lay, s1)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.01, 3)
    w1 = _call_adamw(lay, s1, pdt, amsgrad, hyper, None)
    w2 = _call_adamw(lay, s2, pdt, amsgrad, hyper, _scale(1.0))
    for k in s1:
        assert torch.equal(s1[k][0], s2[k][0]), (pdt, gdt, amsgrad, k)
    if w1 is not None:
        assert torch.equal(w1, w2)


def _sgd_streams(pdt, gdt):
    lay = _Carved(NUMELS)
    gen = torch.Generator(device="cuda").manual_seed(12)
    s = {"p": lay.stream(pdt, gen), "g": lay.stream(gdt, gen),
         "buf": lay.stream(F32, gen)}
    return lay, s


_SGD_HYPER = (0.1, 0.9, 0.1, 0.01, False, False)  # lr mom damp wd nest max


def _call_sgd(lay, s, pdt, first, grad_scale):
    wf, ws = _with_master(lay, s, pdt)
    args = (s["p"][1], s["g"][1], s["buf"][1], ws, first, *_SGD_HYPER)
    if grad_scale is None:
        _ext.get_ext().sgd_step_multi(*args)
    else:
        _ext.get_ext().sgd_step_multi(*args, grad_scale)
    return wf


@pytest.mark.parametrize("pdt,gdt", _OPT_DTYPES)
def test_sgd_momentum_grad_scale_gpu(pdt, gdt):
    lay, s = _sgd_streams(pdt, gdt)
    first = [i % 3 == 1 for i in range(len(NUMELS))]
    gs = _scale(0.37)
    rp, rb = _sgd_ref64(s["p"][0].double(),
                        gs.double() * s["g"][0].double(),
                        s["buf"][0].double(), lay.per_tensor(first),
                        *_SGD_HYPER)
    g0 = s["g"][0].clone()
    wf = _call_sgd(lay, s, pdt, first, gs)
    name = f"sgd scaled {pdt}/{gdt}"
    for k, (flat, _) in s.items():
        lay.check_guards(flat, f"{name} {k}")
    assert torch.equal(s["g"][0], g0), f"{name}: gradient written"
    lay.close(s["buf"][0], rb, f"{name} buf")
    if wf is not None:
        lay.check_guards(wf, f"{name} master")
        lay.close(wf, rp, f"{name} master")
        assert torch.equal(s["p"][0][lay.mask], wf.to(BF16)[lay.mask])
    else:
        lay.close(s["p"][0], rp, f"{name} p")


@pytest.mark.parametrize("pdt,gdt", _OPT_DTYPES)
def test_sgd_unit_grad_scale_is_bitwise_noop_gpu(pdt, gdt):
    lay, s1 = _sgd_streams(pdt, gdt)
    s2 = _clone_streams(lay, s1)
    first = [i % 3 == 1 for i in range(len(NUMELS))]
    w1 = _call_sgd(lay, s1, pdt, first, None)
    w2 = _call_sgd(lay, s2, pdt, first, _scale(1.0))
    for k in s1:
        assert torch.equal(s1[k][0], s2[k][0]), (pdt, gdt, k)
    if w1 is not None:
        assert torch.equal(w1, w2)


def test_grad_scale_argument_checks_gpu():
    p = torch.zeros(8, device="cuda")
    g = torch.ones(8, device="cuda")
    m, v = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    ext = _ext.get_ext()

    def call(scale):
        ext.adamw_step_multi([p], [g], [m], [v], [None], [None], 1e-3, 0.9,
                             0.999, 1e-8, 0.0, 1, scale)

    for bad, msg in ((torch.ones(2, device="cuda"), "elements"),
                     (torch.ones((), device="cuda", dtype=BF16), "float32"),
                     (torch.ones(()), "is on")):
        with pytest.raises(RuntimeError, match=msg):
            call(bad)
    assert torch.equal(p, torch.zeros_like(p))  # nothing launched
    call(torch.ones(1, device="cuda"))          # any 1-element shape


# ---- 11. end to end ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_clipped_optimizer_matches_cpu_gpu(kind):
    """bf16 parameters with fixed gradients: the GPU optimizer (norm kernel
    + scaled fused update) against the same optimizer on CPU copies (the
    torch branch of every op). ~70k elements of randn * f have norm
    ~265 * f: step 1 (f = 0.02) clips, step 3 (f = 0.001) does not."""
    gen = torch.Generator().manual_seed(3)
    shapes = [(C + 5,), (7,), (300, 17)]
    init = [(torch.randn(s, generator=gen) * 0.1).to(BF16) for s in shapes]
    grads = [[(torch.randn(s, generator=gen) * f).to(BF16) for s in shapes]
             for f in (0.02, 0.004, 0.001)]

    def make(device):
        ps = [(f"p{i}", torch.nn.Parameter(t.clone().to(device)))
              for i, t in enumerate(init)]
        if kind == "adamw":
            return ps, AdamW(ps, lr=1e-2, weight_decay=0.1, max_grad_norm=1.0)
        return ps, SGD(ps, lr=1e-2, momentum=0.9, max_grad_norm=1.0)

    (gp, gopt), (cp, copt) = make("cuda"), make("cpu")
    norms = []
    for step_grads in grads:
        for (_, a), (_, b), g in zip(gp, cp, step_grads):
            a.grad = g.clone().cuda()
            b.grad = g.clone()
        gopt.step()
        copt.step()
        got = gopt.last_grad_norm
        assert got.is_cuda and got.dim() == 0 and got.dtype == F32
        torch.testing.assert_close(got.cpu(), copt.last_grad_norm, rtol=1e-5,
                                   atol=0.0)
        norms.append(got.item())
        for n in gopt.master:
            d = (gopt.master[n].cpu() - copt.master[n]).abs().max().item()
            assert d <= 1e-6, (kind, n, d)
    assert norms[0] > 1.0 and norms[2] < 1.0, norms


# ---- 12. the norm all-reduce through RCCL -----------------------------------
@pytest.fixture(scope="module")
def nccl_world1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(free_port())  # an earlier module's is spent
    os.environ["TDSA_COMM_FORCE"] = "1"
    dist.init_process_group("nccl", rank=0, world_size=1)
    yield
    dist.destroy_process_group()
    os.environ.pop("TDSA_COMM_FORCE", None)


def _train_clipped(strategy, force, steps=3):
    """Bias-free Linears only: their GEMMs repeat bit for bit, so the forced
    and the unforced run can be compared exactly."""
    from collections import OrderedDict

    from tiny_deepspeed_amd import (Zero2, Zero2SGD, Zero2Flat, Zero2FlatSGD,
                                    partition_tensors)
    from tiny_deepspeed_amd.parallel.comm import CommContext

    os.environ["TDSA_COMM_FORCE"] = "1" if force else "0"
    os.environ["TDSA_AUTOTUNE"] = "0"
    try:
        torch.manual_seed(21)
        model = torch.nn.Sequential(
            torch.nn.Linear(256, 512, bias=False),
            torch.nn.Linear(512, 256, bias=False),
        ).to(device="cuda", dtype=BF16)
        comm = CommContext()
        assert comm._inactive() != force
        kw = dict(lr=0.1, momentum=0.9, max_grad_norm=1.0)
        if strategy == "zero2flat":
            wrapped = Zero2Flat(model, comm=comm, bucket_bytes=1 << 18)
            opt = Zero2FlatSGD(wrapped, **kw)
        else:
            parts, _ = partition_tensors(
                OrderedDict(model.named_parameters()), ranks_map=["cuda:0"],
                evenness_priority=0, verbose=False)
            wrapped = Zero2(model, parts, comm=comm)
            opt = Zero2SGD(wrapped.named_parameters(), param_part_table=parts,
                           ranks_map=["cuda:0"], comm=comm, **kw)
        g = torch.Generator().manual_seed(5)
        x = (torch.randn(64, 256, generator=g) * 4.0).to(BF16).cuda()
        norms, counts = [], []
        for _ in range(steps):
            wrapped.require_backward_grad_sync = True
            wrapped(x).float().square().mean().backward()
            opt.step()
            norms.append(opt.last_grad_norm.clone())
            counts.append(comm.stats.get("all_reduce", [0, 0])[0])
        torch.cuda.synchronize()
        params = [p.detach().clone() for p in wrapped.parameters()]
        return norms, counts, params
    finally:
        os.environ["TDSA_COMM_FORCE"] = "1"
        os.environ.pop("TDSA_AUTOTUNE", None)


@pytest.mark.parametrize("strategy", ["zero2", "zero2flat"])
def test_forced_rccl_clipped_step_matches_unforced_gpu(strategy, nccl_world1):
    f_norms, f_counts, f_params = _train_clipped(strategy, force=True)
    u_norms, u_counts, u_params = _train_clipped(strategy, force=False)
    assert f_counts == [1, 2, 3], f_counts   # one norm all-reduce per step
    assert u_counts == [0, 0, 0], u_counts
    assert f_norms[0].item() > 1.0, f_norms  # the clip is live
    for a, b in zip(f_norms, u_norms):
        assert torch.equal(a, b), (f_norms, u_norms)
    for a, b in zip(f_params, u_params):
        assert torch.equal(a, b)
