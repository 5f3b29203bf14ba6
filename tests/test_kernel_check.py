"""CPU self-test of tests/kernel_check.py: the comparator and the inputs of
the kernel tests can fail. On the generators and the smallest shapes of
test_attention_geometry_gpu.py and test_kernel_edges_gpu.py, the project's
plain fp32 candidate (rounded to the output dtype) passes against the fp64
reference, and every corrupted copy of the fp64 reference is rejected at the
cap alone: the copy carries no rounding error, only the corruption.

The 'plain passes' tests hand plain in as both ``out`` and ``plain`` with
K = 1, so there the K condition holds by construction and only the cap and
the finiteness check are exercised; the K condition itself is tested in
test_assert_tracks_needs_cap_K_and_finite."""

import importlib
import math

import pytest
import torch

from tests import kernel_check as KC

attention = importlib.import_module("tiny_deepspeed_amd.ops.attention")
ce = importlib.import_module("tiny_deepspeed_amd.ops.cross_entropy")
emb = importlib.import_module("tiny_deepspeed_amd.ops.embedding")
gelu = importlib.import_module("tiny_deepspeed_amd.ops.gelu")
linear = importlib.import_module("tiny_deepspeed_amd.ops.linear")

BF16 = torch.bfloat16
SCALE = 1.0 / math.sqrt(64)
P_DROP = 0.3
GRADS = ("dq", "dk", "dv")


# ---- the comparator itself ---------------------------------------------------
def test_rel_err_names_the_worst_slice():
    ref = torch.ones(3, 4, 8, dtype=torch.float64)
    ref[0] *= 1000.0                      # a large slice elsewhere
    out = ref.clone().float()
    out[2, 1, 5] += 0.5                   # the culprit: slice (2, 1)
    worst, idx = KC.rel_err(out, ref, -1)
    assert idx == (2, 1) and worst == pytest.approx(0.5)
    # one global scale would have hidden it
    assert (out.double() - ref).abs().max() / ref.abs().max() < 1e-3
    assert KC.rel_err(out, ref, (0, 1, 2))[1] == ()


def test_rel_err_floor_is_smallest_normal():
    ref = torch.zeros(4, 8, dtype=torch.float64)
    out = torch.zeros(4, 8, dtype=BF16)
    assert KC.rel_err(out, ref, -1)[0] == 0.0
    out[3, 0] = 1e-6                      # an all-zero slice must stay zero
    worst, idx = KC.rel_err(out, ref, -1)
    assert idx == (3,) and worst > 1e30


def test_rel_err_counts_nan_as_infinite():
    ref = torch.ones(2, 8, dtype=torch.float64)
    out = torch.ones(2, 8)
    out[1, 2] = float("nan")
    assert KC.rel_err(out, ref, -1) == (float("inf"), (1,))
    assert KC.rejected(out, ref, -1, 1e30)


def test_assert_tracks_needs_cap_K_and_finite():
    ref = torch.ones(2, 8, dtype=torch.float64)
    plain = ref.float() * (1 + 1e-3)
    KC.assert_tracks(ref.float() * (1 + 2e-3), plain, ref, -1, 4, 1e-2, "ok")
    with pytest.raises(AssertionError, match="x plain"):
        KC.assert_tracks(ref.float() * (1 + 8e-3), plain, ref, -1, 4, 1e-2, "K")
    with pytest.raises(AssertionError, match="cap"):
        KC.assert_tracks(ref.float() * 1.1, plain, ref, -1, 1e9, 1e-2, "cap")
    # plain_floor credits a lucky (not an exact) plain with the format's rounding
    ref1 = torch.tensor(1.0, dtype=torch.float64)
    lucky = torch.tensor(1 + 1e-9, dtype=torch.float64)
    out = torch.tensor(1 + 1e-7, dtype=torch.float64)
    with pytest.raises(AssertionError, match="x plain"):
        KC.assert_tracks(out, lucky, ref1, None, 4, 1e-5, "no floor")
    KC.assert_tracks(out, lucky, ref1, None, 4, 1e-5, "floor", plain_floor=KC.U_F32)
    with pytest.raises(AssertionError, match="x plain"):
        KC.assert_tracks(out, ref1, ref1, None, 4, 1e-5, "exact plain",
                         plain_floor=KC.U_F32)
    bad = ref.float().clone()
    bad[0, 0] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        KC.assert_tracks(bad, plain, ref, -1, KC.INF, KC.INF, "finite")


# ---- attention ---------------------------------------------------------------
@pytest.fixture(scope="module")
def attn64():
    """(2, 8, 64): the single-tile shape of the geometry tests."""
    q, k, v, do = KC.attn_inputs(2, 8, 64, "cpu")
    names = ("o", "lse") + GRADS
    return (q, k, v, do), dict(zip(names, KC.attn_autograd(
        q, k, v, do, SCALE, torch.float64)))


@pytest.fixture(scope="module")
def attn320():
    """(1, 6, 320): five key tiles, the smallest dropout shape."""
    q, k, v, do = KC.attn_inputs(1, 6, 320, "cpu", seed=1)
    names = ("o", "lse") + GRADS
    ref = dict(zip(names, KC.attn_autograd(q, k, v, do, SCALE, torch.float64)))
    g = torch.Generator().manual_seed(5)
    keep = (torch.rand(1, 6, 320, 320, generator=g) >= P_DROP)
    keep &= KC.causal_mask(320, "cpu")
    refd = dict(zip(names, KC.attn_autograd(
        q, k, v, do, SCALE, torch.float64, keep=keep, p=P_DROP)))
    return (q, k, v, do), ref, keep, refd


@pytest.fixture(scope="module")
def spike256():
    """(1, 2, 256) with the spike key at row 160."""
    q, k, v, do = KC.attn_inputs(1, 2, 256, "cpu", seed=5, spike=True)
    names = ("o", "lse") + GRADS
    return (q, k, v, do), dict(zip(names, KC.attn_autograd(
        q, k, v, do, SCALE, torch.float64)))


def _cap(name):
    return KC.CAP_FWD if name in ("o", "lse") else KC.CAP_ATTN_GRAD


@pytest.mark.parametrize("fix", ["attn64", "attn320", "spike256"])
def test_attention_plain_passes(fix, request):
    got = request.getfixturevalue(fix)
    (q, k, v, do), ref = got[0], got[1]
    o, lse = attention._composite_fwd(q, k, v, SCALE)
    dq, dk, dv = attention._composite_bwd(q, k, v, o, lse, do, SCALE)
    KC.assert_tracks(o, o, ref["o"], -1, 1, KC.CAP_FWD, "plain o")
    KC.assert_tracks(lse, lse, ref["lse"], -1, 1, KC.CAP_FWD, "plain lse")
    # the backward is an operation on (q, k, v, o, lse, do): its reference
    # takes the same bf16 o and fp32 lse (see KC.attn_bwd_formula)
    r = dict(zip(GRADS, KC.attn_bwd_formula(q, k, v, o, lse, do, SCALE,
                                            torch.float64)))
    KC.assert_dq_tracks(dq, dq, r["dq"], KC.dq_token0_bound(k, v, do, SCALE),
                        1, KC.CAP_ATTN_GRAD, "plain dq")
    for n, g in zip(GRADS[1:], (dk, dv)):
        KC.assert_tracks(g, g, r[n], -1, 1, KC.CAP_ATTN_GRAD, "plain " + n)


@pytest.mark.parametrize("fix", ["attn64", "attn320"])
def test_bwd_formula_is_the_autograd_gradient(fix, request):
    """With the exact o and lse the backward formula is the gradient."""
    got = request.getfixturevalue(fix)
    (q, k, v, do), ref = got[0], got[1]
    got = KC.attn_bwd_formula(q, k, v, ref["o"], ref["lse"], do, SCALE,
                              torch.float64)
    for n, g in zip(GRADS, got):
        assert not KC.rejected(g, ref[n], -1, 1e-12), n
    if fix == "attn320":
        keep, refd = request.getfixturevalue(fix)[2:]
        got = KC.attn_bwd_formula(q, k, v, refd["o"], refd["lse"], do, SCALE,
                                  torch.float64, keep=keep, p=P_DROP)
        for n, g in zip(GRADS, got):
            # token 0 of dq cancels to rounding noise: from token 1 on
            assert not KC.rejected(g[:, :, 1:], refd[n][:, :, 1:], -1, 1e-12), n


def test_attention_dropout_plain_passes(attn320):
    (q, k, v, do), _, keep, refd = attn320
    o, lse = KC.attn_autograd(q, k, v, do, SCALE, torch.float32, keep=keep,
                              p=P_DROP)[:2]
    o = o.to(BF16)
    KC.assert_tracks(o, o, refd["o"], -1, 1, KC.CAP_FWD, "plain drop o")
    KC.assert_tracks(lse, lse, refd["lse"], -1, 1, KC.CAP_FWD, "plain drop lse")
    args = (q, k, v, o, lse, do, SCALE)
    r = dict(zip(GRADS, KC.attn_bwd_formula(*args, torch.float64, keep=keep,
                                            p=P_DROP)))
    dq, dk, dv = (t.to(BF16) for t in KC.attn_bwd_formula(
        *args, torch.float32, keep=keep, p=P_DROP))
    KC.assert_dq_tracks(dq, dq, r["dq"],
                        KC.dq_token0_bound(k, v, do, SCALE, P_DROP), 1,
                        KC.CAP_ATTN_GRAD, "plain drop dq")
    for n, g in zip(GRADS[1:], (dk, dv)):
        KC.assert_tracks(g, g, r[n], -1, 1, KC.CAP_ATTN_GRAD, "plain drop " + n)


@pytest.mark.parametrize("fix", ["attn64", "attn320"])
@pytest.mark.parametrize("name", ("o",) + GRADS)
def test_mutant_token_row_zeroed(fix, name, request):
    ref = request.getfixturevalue(fix)[1]
    bad = ref[name].clone()
    bad[-1, 3, 37, :] = 0
    assert KC.rel_err(bad, ref[name], -1)[1] == (bad.shape[0] - 1, 3, 37)
    assert KC.rejected(bad, ref[name], -1, _cap(name))


@pytest.mark.parametrize("tile", [0, 2, 4])
def test_mutant_key_tile_removed_from_one_head(attn320, tile):
    (q, k, v, do), ref = attn320[0], attn320[1]
    bad = dict(zip(("o", "lse") + GRADS, KC.attn_autograd(
        q, k, v, do, SCALE, torch.float64, drop_tile=(0, 4, tile))))
    for n in ("o",) + GRADS:
        assert KC.rejected(bad[n], ref[n], -1, _cap(n)), n
        assert KC.rel_err(bad[n], ref[n], -1)[1][:2] == (0, 4), n
        # every other head is untouched
        others = [h for h in range(6) if h != 4]
        assert not KC.rejected(bad[n][:, others], ref[n][:, others], -1, 0.0)


@pytest.mark.parametrize("fix", ["attn64", "attn320"])
@pytest.mark.parametrize("diagonal", [-1, 1])
def test_mutant_causal_mask_off_by_one(fix, diagonal, request):
    (q, k, v, do), ref = request.getfixturevalue(fix)[:2]
    bad = dict(zip(("o", "lse") + GRADS, KC.attn_autograd(
        q, k, v, do, SCALE, torch.float64, diagonal=diagonal)))
    for n in ("o",) + GRADS:
        # tril(-1) leaves token 0 without a key (NaN): rejected as a whole,
        # and from token 1 on by the numbers alone
        assert KC.rejected(bad[n], ref[n], -1, _cap(n)), n
        assert KC.rejected(bad[n][:, :, 1:], ref[n][:, :, 1:], -1, _cap(n)), n


@pytest.mark.parametrize("name", ("o", "lse") + GRADS)
def test_mutant_two_heads_swapped(attn64, name):
    ref = attn64[1][name]
    bad = ref.clone()
    bad[1, 2], bad[1, 5] = ref[1, 5], ref[1, 2]
    assert KC.rejected(bad, ref, -1, _cap(name))


def test_mutant_dk_dv_swapped(attn64):
    ref = attn64[1]
    assert KC.rejected(ref["dv"], ref["dk"], -1, KC.CAP_ATTN_GRAD)
    assert KC.rejected(ref["dk"], ref["dv"], -1, KC.CAP_ATTN_GRAD)


def test_mutant_dropout_rescale_omitted(attn320):
    (q, k, v, do), _, keep, refd = attn320
    bad = dict(zip(("o", "lse") + GRADS, KC.attn_autograd(
        q, k, v, do, SCALE, torch.float64, keep=keep, p=P_DROP,
        rescale=False)))
    for n in ("o",) + GRADS:
        assert KC.rejected(bad[n], refd[n], -1, _cap(n)), n


@pytest.mark.parametrize("bit", [(0, 0, 5, 2), (0, 3, 9, 9), (0, 5, 12, 10)])
def test_mutant_one_dropout_mask_bit_flipped(attn320, bit):
    """One bit moves o[row] by P[row, key] / (1-p) * v[key]: it is visible
    where P[row, key] is not small, that is in the early rows, which are the
    ones chosen here. dk and dv of a key sum over every later row, so there
    one bit shows at keys close to the row, where few rows weigh in. (On the
    GPU the realised mask is extracted and the reference uses it bit for
    bit.)"""
    (q, k, v, do), _, keep, refd = attn320
    keep2 = keep.clone()
    keep2[bit] = ~keep2[bit]
    bad = dict(zip(("o", "lse") + GRADS, KC.attn_autograd(
        q, k, v, do, SCALE, torch.float64, keep=keep2, p=P_DROP)))
    assert KC.rejected(bad["o"], refd["o"], -1, KC.CAP_FWD)
    assert KC.rel_err(bad["o"], refd["o"], -1)[1] == bit[:3]
    for n in GRADS:
        assert KC.rejected(bad[n], refd[n], -1, KC.CAP_ATTN_GRAD), n
    # dq moves in the flipped row, dk and dv at the flipped key
    assert KC.rel_err(bad["dq"], refd["dq"], -1)[1] == bit[:3]
    assert KC.rel_err(bad["dv"], refd["dv"], -1)[1] == bit[:2] + bit[3:]


# ---- cross-entropy -----------------------------------------------------------
CE_SHAPES = [(BF16, 8), (BF16, 2056), (torch.float32, 4), (torch.float32, 1028)]


def _ce_cap(dtype):
    return KC.CAP_FWD if dtype == BF16 else KC.CAP_F32


@pytest.mark.parametrize("dtype,V", CE_SHAPES)
@pytest.mark.parametrize("scale,tail", [(3.0, False), (30.0, False), (3.0, True)])
def test_cross_entropy_plain_passes(dtype, V, scale, tail):
    logits, tgt = KC.ce_inputs(5, V, dtype, "cpu", scale=scale,
                               neg_inf_tail=tail)
    lse64, loss64, n64, d64 = KC.ce_ref64(logits, tgt)
    assert torch.isfinite(lse64).all() and torch.isfinite(d64).all()
    loss, lse, n = ce.ce_fwd_torch(logits, tgt, KC.IGNORE)
    d = ce.ce_bwd_torch(1.0, logits, tgt, lse, n, KC.IGNORE)
    assert int(n) == n64 == 3             # two of the five rows are ignored
    KC.assert_tracks(lse, lse, lse64, None, 1, KC.CAP_F32, "plain ce lse")
    KC.assert_tracks(loss, loss, loss64, None, 1, KC.CAP_F32, "plain ce loss")
    KC.assert_tracks(d, d, d64, -1, 1, _ce_cap(dtype), "plain ce dlogits")


@pytest.mark.parametrize("dtype,V", CE_SHAPES)
@pytest.mark.parametrize("mutant", [
    "zero", "onehot_at_t_plus_1", "ignored_row_has_gradient",
    "n_valid_counts_ignored"])
def test_cross_entropy_mutants(dtype, V, mutant):
    logits, tgt = KC.ce_inputs(5, V, dtype, "cpu")
    assert (tgt == KC.IGNORE).sum() == 2
    _, _, _, d64 = KC.ce_ref64(logits, tgt)
    if mutant == "zero":
        bad = torch.zeros_like(d64)
    elif mutant == "onehot_at_t_plus_1":
        bad = KC.ce_ref64(logits, tgt, onehot_shift=1)[3]
    elif mutant == "ignored_row_has_gradient":
        bad = KC.ce_ref64(logits, tgt, grad_ignored=True)[3]
    else:
        bad = KC.ce_ref64(logits, tgt, count_ignored=True)[3]
    assert KC.rejected(bad, d64, -1, _ce_cap(dtype))


# ---- GELU --------------------------------------------------------------------
@pytest.mark.parametrize("dtype,cap", [(BF16, KC.CAP_POINT_BF16),
                                       (torch.float32, KC.CAP_GELU_F32)])
@pytest.mark.parametrize("pool", ["tiny", "unit", "large"])
@pytest.mark.parametrize("n", [1, 7, 9])
def test_gelu_plain_passes(dtype, cap, pool, n):
    x, dy = KC.gelu_inputs(n, dtype, "cpu", pool)
    y64, dx64 = KC.gelu_ref64(x, dy)
    assert torch.isfinite(y64).all() and torch.isfinite(dx64).all()
    y = gelu.gelu_fwd_torch(x)
    dx = gelu.gelu_bwd_torch(dy, x)
    KC.assert_tracks(y, y, y64, 0, 1, cap, "plain gelu fwd")
    KC.assert_tracks(dx, dx, dx64, 0, 1, cap, "plain gelu bwd")


# ---- column sum --------------------------------------------------------------
@pytest.mark.parametrize("dtype,cap", [(BF16, KC.CAP_POINT_BF16),
                                       (torch.float32, KC.CAP_F32)])
@pytest.mark.parametrize("M,N", [(1, 8), (129, 257)])
def test_column_sum_plain_and_mutant(dtype, cap, M, N):
    dy = KC.colsum_inputs(M, N, dtype, "cpu")
    ref = dy.double().sum(dim=0)
    plain = linear.db_torch(dy)
    KC.assert_tracks(plain, plain, ref, 0, 1, cap, "plain colsum")
    bad = dy[:-1].double().sum(dim=0)     # the last row left out
    assert KC.rejected(bad, ref, 0, cap)


# ---- embedding ---------------------------------------------------------------
@pytest.mark.parametrize("dtype,cap", [(BF16, KC.CAP_POINT_BF16),
                                       (torch.float32, KC.CAP_F32)])
def test_embedding_bwd_plain_and_mutant(dtype, cap):
    for name, (idx, pad) in KC.emb_bwd_cases("cpu").items():
        dy = KC.emb_dy(idx.numel(), 8, dtype, "cpu")
        ref = KC.emb_bwd_ref64(idx, dy, KC.EMB_V, pad)
        plain = emb.emb_bwd_torch(idx, dy, KC.EMB_V, pad)
        KC.assert_tracks(plain, plain, ref, -1, 1, cap, "plain emb " + name)
        # a table row hit more than once, counted once
        counts = torch.bincount(idx, minlength=KC.EMB_V)
        if pad is not None:
            counts[pad] = 0
        dup = (counts > 1).nonzero().reshape(-1)
        if name in ("distinct", "single"):
            assert dup.numel() == 0
            continue
        bad = KC.emb_bwd_ref64(idx, dy, KC.EMB_V, pad, once=int(dup[0]))
        assert KC.rejected(bad, ref, -1, cap), name
        assert KC.rel_err(bad, ref, -1)[1] == (int(dup[0]),)
