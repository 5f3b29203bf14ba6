"""Shared comparator, input generators and fp64 references for the tests that
pin one HIP kernel against a plain reference of the same op
(test_attention_geometry_gpu.py, test_kernel_edges_gpu.py) and for the CPU
self-test that proves the comparator can fail (test_kernel_check.py).

Error metric. A tensor is cut into slices, the natural unit of the op (one
token's 64 attention values, one logits row, one table row, ...). The error of
a slice is max|out - ref64| over the slice divided by the slice's own
max|ref64|; the floor of the divisor is the smallest normal of the output
dtype, so a slice whose reference is all zero must be reproduced as zero.
One wrong row therefore shows whatever the largest element elsewhere is.

Bounds. ``cap`` is the project's tolerance for that output, per slice.
``K`` ties the kernel to the project's own fp32 torch candidate for the op
(``plain``): the kernel's worst slice may be at most K times as far from the
fp64 reference as plain's worst slice. The K constants below are twice the
largest ratio measured on an MI355X, rounded up to a power of two; the table
is in docs/kernels.md ("Test bounds").
"""

import math

import torch

BF16 = torch.bfloat16
INF = float("inf")

# ---- caps: the tolerances tests/test_gpu_kernels.py used, now per slice ----
CAP_FWD = 2e-2        # bf16 forward outputs (attention o and lse, CE)
CAP_ATTN_GRAD = 4e-2  # attention dq/dk/dv
CAP_F32 = 1e-5        # fp32 outputs
CAP_POINT_BF16 = 1e-2  # GELU, column sum, embedding in bf16
CAP_GELU_F32 = 1e-6   # GELU in fp32

# ---- K per op family: 2 x largest measured ratio, rounded up to 2^n --------
# (measured on MI355X; per-output figures in docs/kernels.md "Test bounds")
K_ATTN = 16        # o/dq/dk/dv; largest ratio 5.13 (dv, spike input)
K_ATTN_DROP = 8    # Pd/o/dq/dk/dv under dropout; largest ratio 2.74 (dq)
K_CE = 4           # lse, dlogits, loss; largest ratio 1.90 (dlogits, fp32,
#                    V = 50304); lse 1.35; loss 1.66 with plain floored
U_F32 = 2.0 ** -24  # rounding of one fp32 number; plain_floor of the CE loss:
#                     9.9e-8 against max(7.4e-9, U_F32) is the 1.66 above;
#                     unfloored, the luck of one number gives up to 19.2
K_GELU_FWD = 8     # largest ratio 3.50 (fp32, |x| <= 1e-3)
K_GELU_BWD = 32    # largest ratio 8.30 (fp32, n = 1: 5.9e-8 against 7.1e-9)
K_COLSUM = 8       # largest ratio 2.46 (fp32 129 x 257)
K_EMB = 4          # backward; largest ratio 1.41 (fp32, padded run of 40)
# attention lse has no K: the kernel rounds the prescaled Q to bf16 where
# plain keeps fp32 scores, a ratio of 4e3..1.6e4; see lse_format_bound.


def rel_err(out, ref64, dim):
    """Worst slice error of ``out`` against ``ref64`` and that slice's index.

    ``dim``: the dimension(s) one slice spans (int or tuple); None makes every
    element its own slice. Returns (worst, index) where index is a tuple over
    the remaining dimensions. A non-finite value in ``out`` counts as an
    infinite error."""
    assert out.shape == ref64.shape, (out.shape, ref64.shape)
    assert ref64.dtype == torch.float64
    floor = torch.finfo(out.dtype).smallest_normal
    err = (out.double() - ref64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, INF))
    mag = ref64.abs()
    if dim is not None:
        err = err.amax(dim=dim)
        mag = mag.amax(dim=dim)
    r = err / mag.clamp_min(floor)
    if r.dim() == 0:
        return r.item(), ()
    flat = int(r.reshape(-1).argmax().item())
    idx = []
    for n in reversed(r.shape):
        idx.append(flat % n)
        flat //= n
    return r.reshape(-1).max().item(), tuple(reversed(idx))


def assert_tracks(out, plain, ref64, dim, K, cap, name, plain_floor=0.0):
    """out: the kernel's result; plain: the project's fp32 torch candidate on
    the same inputs, rounded to the same dtype; ref64: the fp64 reference.

    plain_floor: least error credited to a plain that is not exact. For an
    output that is ONE number (the loss sum) the worst slice is the only
    slice, and whether plain lands 0.03 or 0.5 ulp from the reference is
    luck; such an output passes U_F32, the rounding of its format, which no
    implementation can be asked to beat."""
    e_out, i_out = rel_err(out, ref64, dim)
    e_plain, _ = rel_err(plain, ref64, dim)
    ratio = e_out / e_plain if e_plain > 0 else (0.0 if e_out == 0 else INF)
    print(f"TRACK {name}: out {e_out:.3e} at {i_out}  plain {e_plain:.3e}  "
          f"ratio {ratio:.2f}  K {K}  cap {cap}")
    assert torch.isfinite(out.float()).all(), f"{name}: non-finite output"
    assert e_out <= cap, f"{name}: slice {i_out} err {e_out:.3e} > cap {cap}"
    # an exact plain (a gather, an all-zero gradient) demands an exact kernel
    credit = max(e_plain, plain_floor) if e_plain > 0 else 0.0
    assert e_out <= K * credit, (
        f"{name}: slice {i_out} err {e_out:.3e} > {K} x plain {credit:.3e}")
    return e_out, e_plain


def rejected(out, ref64, dim, cap):
    """True when ``out`` misses ``cap`` (or is not finite)."""
    return not rel_err(out, ref64, dim)[0] <= cap


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- attention ---------------------------------------------------------------
def attn_inputs(B, H, T, device, seed=0, spike=False):
    """bf16 q, k, v, do of shape (B, H, T, 64), drawn on the CPU so the same
    values reach the CPU self-test and the GPU tests. ``do`` is scaled so the
    gradients are O(1). spike: key row T*5//8 dot-products hugely with every
    query (the input of test_attention_rescale_spike_gpu)."""
    g = _gen(seed)
    q, k, v, do = (torch.randn(B, H, T, 64, generator=g).to(BF16)
                   for _ in range(4))
    if spike:
        k[:, :, T * 5 // 8, :] = (4.0 * torch.sign(q.float().mean(dim=2))).to(BF16)
    do = (do.float() * 4.0).to(BF16)
    return tuple(t.to(device) for t in (q, k, v, do))


def causal_mask(T, device, diagonal=0):
    return torch.ones(T, T, dtype=torch.bool, device=device).tril(diagonal)


def attn_autograd(q, k, v, do, scale, dtype, keep=None, p=0.0, rescale=True,
                  diagonal=0, drop_tile=None):
    """Causal attention forward and backward by autograd in ``dtype`` on the
    given bf16 values: returns o, lse, dq, dk, dv in ``dtype``.

    keep/p: dropout keep-mask (B,H,T,T) and rate, Pd = P * keep / (1-p).
    The remaining arguments build the mutants of the self-test: rescale=False
    omits 1/(1-p); diagonal shifts the causal mask; drop_tile=(b, h, j)
    removes the contribution of key tile j (64 keys) from head (b, h)."""
    T = q.shape[-2]
    qf, kf, vf = (t.to(dtype).detach().requires_grad_(True) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-2, -1)) * scale
    s = s.masked_fill(~causal_mask(T, q.device, diagonal), -INF)
    lse = torch.logsumexp(s, dim=-1)
    P = torch.softmax(s, dim=-1)
    if keep is not None:
        P = P * keep.to(dtype)
        if rescale:
            P = P / (1.0 - p)
    if drop_tile is not None:
        b, h, j = drop_tile
        m = torch.ones_like(P)
        m[b, h, :, 64 * j:64 * j + 64] = 0
        P = P * m
    o = torch.matmul(P, vf)
    o.backward(do.to(dtype))
    return o.detach(), lse.detach(), qf.grad, kf.grad, vf.grad


def attn_fwd_formula(q, k, v, scale, dtype, keep=None, p=0.0):
    """o, lse and the (undropped) softmax P in ``dtype``, forward only."""
    T = q.shape[-2]
    qf, kf, vf = (t.to(dtype) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-2, -1)) * scale
    s = s.masked_fill(~causal_mask(T, q.device), -INF)
    lse = torch.logsumexp(s, dim=-1)
    P = (s - lse.unsqueeze(-1)).exp()
    Pd = P if keep is None else P * (keep.to(dtype) / (1.0 - p))
    return torch.matmul(Pd, vf), lse, P


def attn_bwd_formula(q, k, v, o, lse, do, scale, dtype, keep=None, p=0.0):
    """dq, dk, dv of the backward OPERATION in ``dtype``: like the kernel it
    takes o and lse as inputs, P = exp(S - lse), delta = rowsum(dO * o),
    dS = P * (dP - delta). fp64 gives the reference, fp32 the plain baseline
    under dropout (ops.attention._composite_bwd has no mask).

    Why o and lse are inputs here and not recomputed: o arrives rounded to
    bf16, so delta is off by up to 2^-9 * sum|dO_i o_i| whoever computes it,
    and the row sum of dS is off by as much. Where the softmax is peaked (the
    first tokens, rows that a spike key dominates) the true dq of a token is
    far smaller than that, and the error of ANY implementation against an
    exact-o reference reaches 5-20% of the token's own magnitude (measured on
    _composite_bwd). Against the reference of the operation on its actual
    inputs the same implementations are within 1%."""
    T = q.shape[-2]
    qf, kf, vf, of, dof = (t.to(dtype) for t in (q, k, v, o, do))
    s = torch.matmul(qf, kf.transpose(-2, -1)) * scale
    s = s.masked_fill(~causal_mask(T, q.device), -INF)
    P = (s - lse.to(dtype).unsqueeze(-1)).exp()
    dP = torch.matmul(dof, vf.transpose(-2, -1))
    Pd = P
    if keep is not None:
        m = keep.to(dtype) / (1.0 - p)
        Pd = P * m
        dP = dP * m
    dv = torch.matmul(Pd.transpose(-2, -1), dof)
    delta = (dof * of).sum(dim=-1, keepdim=True)
    dS = P * (dP - delta)
    dq = torch.matmul(dS, kf) * scale
    dk = torch.matmul(dS.transpose(-2, -1), qf) * scale
    return dq, dk, dv


def lse_format_bound(q, k, lse64, scale):
    """(B, H, T) bound on |lse - lse64| from the kernel's number formats. The
    forward folds scale * log2(e) into Q and rounds the product to bf16
    (relative error <= 2^-8) before the QK^T MFMA, so score (i, j) is off by
    at most 2^-8 * scale * sum_d |q_id k_jd|; lse is 1-Lipschitz in the
    largest score error of its row. 2^-20 * (1 + |lse|) covers the fp32
    exp2/log2 and the row sum. plain keeps fp32 scores, which is why lse
    cannot be tied to plain by a small K."""
    T = q.shape[-2]
    a = torch.matmul(q.double().abs(), k.double().abs().transpose(-2, -1))
    a = a.masked_fill(~causal_mask(T, q.device), 0.0).amax(dim=-1)
    return 2.0 ** -8 * scale * a + 2.0 ** -20 * (1.0 + lse64.abs())


def assert_lse_tracks(lse, plain, lse64, q, k, scale, name):
    """lse (fp32) per (batch, head) slice at the forward cap, and per element
    inside lse_format_bound."""
    e_out, i_out = rel_err(lse, lse64, -1)
    e_plain, _ = rel_err(plain, lse64, -1)
    frac = (lse.double() - lse64).abs() / lse_format_bound(q, k, lse64, scale)
    worst = frac.max().item()
    ratio = e_out / e_plain if e_plain > 0 else (0.0 if e_out == 0 else INF)
    print(f"TRACK {name}: out {e_out:.3e} at {i_out}  plain {e_plain:.3e}  "
          f"ratio {ratio:.1f}  err/format-bound {worst:.3f}")
    assert torch.isfinite(lse).all(), f"{name}: non-finite"
    assert e_out <= CAP_FWD, f"{name}: slice {i_out} err {e_out:.3e}"
    assert worst <= 1.0, f"{name}: {worst:.3f} x the format bound"


def dq_token0_bound(k, v, do, scale, p=0.0):
    """(B, H) bound on the absolute error of dq[b, h, 0, :], whose reference
    is zero, or the bf16 rounding of o0 times dO: token 0 sees one key, P = 1,
    and dS = dO.v0 - dO.o0 with o0 = v0. Any fp32 evaluation leaves the
    cancellation residue of two 64-term dot products summed in different
    orders, at most 64 * 2^-24 * sum|dO_i v_i| each; dq = dS * scale * k0,
    and 2x covers the bf16 rounding of dS and dq. The slice metric (floor:
    smallest normal) cannot judge a row that cancels to nothing, so dq is
    compared from token 1 on and token 0 against this bound. Dropout scales
    both products by 1/(1-p), and dS by it once more."""
    terms = (do[:, :, 0].double() * v[:, :, 0].double()).abs().sum(-1)
    k0 = k[:, :, 0].double().abs().amax(-1)
    return 2 * 2 * 64 * 2.0 ** -24 * terms * scale * k0 / (1.0 - p) ** 2


def assert_dq_tracks(dq, plain, ref64, bound0, K, cap, name):
    """assert_tracks on tokens 1.., dq_token0_bound on token 0."""
    err0 = (dq[:, :, 0].double() - ref64[:, :, 0]).abs().amax(-1)
    worst0 = (err0 / bound0).max().item()
    print(f"TRACK {name} token 0: |dq - ref| / bound = {worst0:.3e}")
    assert worst0 <= 1.0, f"{name}: token 0 is {worst0:.3e} x its bound"
    return assert_tracks(dq[:, :, 1:], plain[:, :, 1:], ref64[:, :, 1:], -1, K,
                         cap, name)


# ---- cross-entropy -----------------------------------------------------------
IGNORE = -100


def ce_inputs(R, V, dtype, device, seed=0, scale=3.0, neg_inf_tail=False,
              all_ignored=False):
    """Logits (R, V) and targets. In rows 0..2 the targets sit at column 0,
    at the last finite column and on a chunk boundary (W = 8 bf16 / 4 fp32
    columns per chunk): the start of thread 0's second chunk, column 256*W,
    where V reaches it, else the start of the last chunk. Beyond those, rows
    2 mod 3 have random targets and the others are ignored (two of five rows,
    198 of 300). The target's own logit is kept at least 2 below the row's
    largest other logit: with p_target -> 1 the gradient row is a difference
    of nearly equal numbers that no fp32 lse resolves, for plain and kernel
    alike, and its relative error says nothing about the kernel. Rows whose
    target is the row maximum are therefore not covered.

    neg_inf_tail: the last min(48, V-1) columns of each row are -inf, as when
    padded vocabulary columns are masked, and row 1, a valid row, keeps one
    finite column only: its target, the last finite column."""
    g = _gen(seed)
    W = 8 if dtype == BF16 else 4
    logits = torch.randn(R, V, generator=g) * scale
    tail = min(48, V - 1) if neg_inf_tail else 0
    Vf = V - tail  # finite columns
    tgt = torch.randint(0, Vf, (R,), generator=g)
    edge = [0, Vf - 1, min(256 * W, (Vf - 1) // W * W)]
    for r in range(R):
        if r < 3:
            tgt[r] = edge[r]
    # keep the target off the row maximum
    own = logits.gather(1, tgt[:, None])
    others = logits.scatter(1, tgt[:, None], -INF)[:, :Vf].amax(dim=1, keepdim=True)
    if Vf > 1:
        logits.scatter_(1, tgt[:, None], torch.minimum(own, others - 2.0))
    for r in range(R):
        if r >= 3 and r % 3 != 2:
            tgt[r] = IGNORE
    if all_ignored:
        tgt[:] = IGNORE
    if neg_inf_tail:
        logits[:, Vf:] = -INF
        if R > 1:
            val = logits[1, Vf - 1].clone()
            logits[1, :] = -INF
            logits[1, Vf - 1] = val
    return logits.to(dtype).to(device), tgt.to(device)


def ce_ref64(logits, targets, ignore_index=IGNORE, dloss=1.0,
             count_ignored=False, onehot_shift=0, grad_ignored=False):
    """fp64 lse (R,), loss sum, n_valid and dlogits (R, V). The keyword
    arguments build the mutants of the self-test."""
    lf = logits.double()
    V = lf.shape[1]
    lse = torch.logsumexp(lf, dim=-1)
    valid = targets != ignore_index
    tgt = targets.clamp_min(0)
    picked = lf.gather(1, tgt[:, None]).squeeze(1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse)).sum()
    n_valid = int(valid.sum().item())
    n = targets.numel() if count_ignored else n_valid
    soft = (lf - lse[:, None]).exp()
    soft.scatter_add_(1, ((tgt + onehot_shift) % V)[:, None],
                      -torch.ones_like(soft[:, :1]))
    d = soft * (dloss / max(n, 1))
    if not grad_ignored:
        d = torch.where(valid[:, None], d, torch.zeros_like(d))
    return lse, loss, n_valid, d


# ---- GELU --------------------------------------------------------------------
_C0 = math.sqrt(2.0 / math.pi)
_C1 = 0.044715


def _bf16_neighbours(x):
    """x rounded to bf16, with the bf16 values one and two ulps either side."""
    b = torch.tensor([x], dtype=torch.float32).to(BF16)
    bits = b.view(torch.int16).to(torch.int32)
    out = [(bits + d).to(torch.int16).view(BF16).float().item()
           for d in (-2, -1, 0, 1, 2)]
    return out


def gelu_pools():
    """Input values by magnitude class; a test runs each class as its own
    vector so that one row holds values of one size. |x| <= 100, where the
    fp64 reference is finite."""
    around3 = _bf16_neighbours(3.0) + _bf16_neighbours(-3.0)
    return {
        "tiny": [0.0, -0.0, 1e-3, -1e-3, 5e-4, -7e-4],
        "unit": around3 + [0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 0.0],
        "large": [10.0, -10.0, 100.0, -100.0, 30.0, -30.0],
    }


def gelu_inputs(n, dtype, device, pool, seed=0):
    """x: the pool's values cycled over n elements, in a seeded random order
    with a little seeded jitter on the 'unit' class once the pool is used up;
    dy: O(1) random."""
    g = _gen(seed)
    vals = torch.tensor(gelu_pools()[pool], dtype=torch.float32)
    x = vals[torch.arange(n) % len(vals)].clone()
    if n > len(vals) and pool == "unit":
        x[len(vals):] = torch.randn(n - len(vals), generator=g) * 2.0
    dy = torch.randn(n, generator=g) + 2.0
    return x.to(dtype).to(device), dy.to(dtype).to(device)


def gelu_ref64(x, dy):
    xf = x.double()
    t = torch.tanh(_C0 * (xf + _C1 * xf ** 3))
    y = 0.5 * xf * (1.0 + t)
    dt = (1.0 - t * t) * _C0 * (1.0 + 3.0 * _C1 * xf * xf)
    return y, dy.double() * (0.5 * (1.0 + t) + 0.5 * xf * dt)


# ---- column sum --------------------------------------------------------------
def colsum_inputs(M, N, dtype, device, seed=0):
    # a mean of 1 keeps every column's sum away from zero
    return (torch.randn(M, N, generator=_gen(seed)) + 1.0).to(dtype).to(device)


# ---- embedding ---------------------------------------------------------------
EMB_V = 64  # table rows of the backward cases


def emb_bwd_cases(device, seed=0):
    """name -> (flat idx, padding_idx) over a table of EMB_V rows. The kernel
    sums a run of equal (sorted) indices in pieces of 32 that a second kernel
    joins: 'all_equal' is one run of 1025 = 32 pieces + 1 row, 'pad40' a
    padded run that crosses a piece boundary."""
    g = _gen(seed)
    V = EMB_V
    rnd = lambda n: torch.randint(1, V, (n,), generator=g)
    pad1 = rnd(200)
    pad1[17] = 0
    pad40 = rnd(200)
    pad40[torch.randperm(200, generator=g)[:40]] = 0
    cases = {
        "all_equal": (torch.full((1025,), 7, dtype=torch.long), None),
        "distinct": (torch.randperm(V, generator=g)[:50], None),
        "pad0": (rnd(200), 0),
        "pad1": (pad1, 0),
        "pad40": (pad40, 0),
        "single": (torch.tensor([V - 1]), None),
    }
    return {n: (i.to(device), p) for n, (i, p) in cases.items()}


def emb_dy(R, D, dtype, device, seed=1):
    return torch.randn(R, D, generator=_gen(seed)).to(dtype).to(device)


def emb_bwd_ref64(idx, dy, V, padding_idx=None, once=None):
    """fp64 index_add_. once: a table row whose duplicate occurrences are
    counted one time only (mutant)."""
    flat = idx.reshape(-1)
    dy2 = dy.reshape(-1, dy.shape[-1]).double()
    keep = torch.ones_like(flat, dtype=torch.bool)
    if padding_idx is not None:
        keep &= flat != padding_idx
    if once is not None:
        hits = (flat == once).nonzero().reshape(-1)
        keep[hits[1:]] = False
    dw = torch.zeros(V, dy2.shape[-1], dtype=torch.float64, device=dy.device)
    dw.index_add_(0, flat[keep], dy2[keep])
    return dw
