"""The attention kernels reproduce recorded output bits.

tests/golden/attention_bits.json holds SHA-256 digests of the raw bytes of
o, lse, dq, dk, dv (and of the inputs q, k, v, do) for the cases below,
recorded from the commit before the forward/backward loops were re-scheduled
(one-instruction bf16 packing, lse/delta fetched one Q tile ahead in the
dK/dV kernel). Neither change touches an arithmetic operation or its order
and the kernels have no atomics, so every later build must give the same
bits. A change that is MEANT to alter the arithmetic regenerates the file:

    python -m tests.test_attention_bits_gpu --record

The same cases are also held against the fp64 formulas with the bounds of
tests/kernel_check.py, so this file still says something after that.

Cases (B, H, T), each without dropout and with p = 0.3:
  (1, 2, 64)   2-wave template, one Q tile: the dK/dV prologue fetch only
  (1, 2, 192)  2-wave, three Q tiles, key blocks starting at tiles 0, 1, 2
  (1, 2, 128)  4-wave
  (2, 8, 256)  8-wave, XCD remap on
  (1, 3, 512)  8-wave, remap off, the second key block starts at Q tile 4
  (2, 8, 512)  with TDSA_ATTN_{FWD,BWD}_NW = 4 and = 2
T = 192 and T = 512 of the first group take the spike input: lse then
differs strongly from one Q tile to the next, and lse/delta of the wrong
tile cannot pass.
"""

import functools
import hashlib
import importlib
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kernel_check as KC
from tiny_deepspeed_amd.ops import _ext

BF16 = torch.bfloat16
SCALE = 1.0 / math.sqrt(64)
P_DROP = 0.3
SEED = 987654321
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "attention_bits.json")
INPUTS = ("q", "k", "v", "do")
OUTPUTS = ("o", "lse", "dq", "dk", "dv")

# (B, H, T, spike, waves knob or None)
SHAPES = [
    (1, 2, 64, False, None),
    (1, 2, 192, True, None),
    (1, 2, 128, False, None),
    (2, 8, 256, False, None),
    (1, 3, 512, True, None),
    (2, 8, 512, False, 4),
    (2, 8, 512, False, 2),
]
CASES = [s + (p,) for s in SHAPES for p in (0.0, P_DROP)]


def _name(B, H, T, spike, nw, p):
    return (f"B{B}H{H}T{T}" + ("spike" if spike else "") +
            (f"NW{nw}" if nw else "") + f"p{p}")


def _digest(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == BF16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=BF16)


class _waves:
    """TDSA_ATTN_FWD_NW / TDSA_ATTN_BWD_NW for the calls inside; the
    launchers read them at every launch."""
    KEYS = ("TDSA_ATTN_FWD_NW", "TDSA_ATTN_BWD_NW")

    def __init__(self, nw):
        self.nw = nw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.KEYS}
        for k in self.KEYS:
            if self.nw is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(self.nw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _inputs(B, H, T, spike):
    return KC.attn_inputs(B, H, T, "cuda", seed=T + H, spike=spike)


@functools.lru_cache(maxsize=None)
def _run(B, H, T, spike, nw, p):
    """Forward and backward through the extension into NaN-filled buffers,
    once per case; shared by the tests below and never modified."""
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"
    ext = _ext.get_ext()
    q, k, v, do = _inputs(B, H, T, spike)
    seed = SEED if p > 0 else 0
    with _waves(nw):
        o, lse = ext.attention_fwd(q, k, v, SCALE, _nan(*q.shape), p, seed)
        dq, dk, dv = ext.attention_bwd(q, k, v, o, lse, do, SCALE,
                                       _nan(*q.shape), _nan(*q.shape),
                                       _nan(*q.shape), p, seed)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def _digests(case):
    B, H, T, spike, nw, p = case
    return {
        "inputs": dict(zip(INPUTS, map(_digest, _inputs(B, H, T, spike)))),
        "outputs": dict(zip(OUTPUTS, map(_digest, _run(*case)))),
    }


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: _name(*c))
def test_attention_reproduces_recorded_bits_gpu(case):
    want = _golden()[_name(*case)]
    got = _digests(case)
    # a change of inputs (generator, seeds) is not a change of kernel
    assert got["inputs"] == want["inputs"], "inputs differ from the recorded ones"
    for name, t in zip(OUTPUTS, _run(*case)):
        assert torch.isfinite(t.float()).all(), name
    differ = [n for n in OUTPUTS if got["outputs"][n] != want["outputs"][n]]
    assert not differ, f"{_name(*case)}: bits of {differ} differ from the record"


def _keep_mask(q, k, p, nw):
    """The realised dropout keep-mask (B,H,T,T), by T/64 forward calls with
    V the 64x64 identity in key rows 64j..64j+63 (O = Pd[:, 64j:64j+64]);
    the RNG key is (seed, bh, row, key), so V does not enter it."""
    ext = _ext.get_ext()
    B, H, T, _ = q.shape
    pd = torch.empty(B, H, T, T, device="cuda", dtype=BF16)
    eye = torch.eye(64, device="cuda", dtype=BF16)
    with _waves(nw):
        for j in range(T // 64):
            vj = torch.zeros(B, H, T, 64, device="cuda", dtype=BF16)
            vj[:, :, 64 * j:64 * j + 64] = eye
            pd[..., 64 * j:64 * j + 64] = ext.attention_fwd(
                q, k, vj, SCALE, _nan(B, H, T, 64), p, SEED)[0]
    assert not torch.isnan(pd).any()
    return (pd != 0) & KC.causal_mask(T, "cuda")


@pytest.mark.parametrize("case", CASES, ids=lambda c: _name(*c))
def test_attention_recorded_cases_track_fp64_gpu(case):
    B, H, T, spike, nw, p = case
    attention = importlib.import_module("tiny_deepspeed_amd.ops.attention")
    name = _name(*case)
    q, k, v, do = _inputs(B, H, T, spike)
    o, lse, dq, dk, dv = _run(*case)
    keep = _keep_mask(q, k, p, nw) if p > 0 else None
    K = KC.K_ATTN_DROP if p > 0 else KC.K_ATTN

    o64, _, _ = KC.attn_fwd_formula(q, k, v, SCALE, torch.float64, keep, p)
    _, lse64, _ = KC.attn_fwd_formula(q, k, v, SCALE, torch.float64)
    # plain: the project's fp32 composite; under dropout, which it does not
    # have, the fp32 formula with the same mask
    o_p, lse_p = attention._composite_fwd(q, k, v, SCALE)
    if p > 0:
        o_p = KC.attn_fwd_formula(q, k, v, SCALE, torch.float32, keep,
                                  p)[0].to(BF16)
    KC.assert_tracks(o, o_p, o64, -1, K, KC.CAP_FWD, name + " o")
    # the row sum is unmasked: lse is the no-dropout lse
    KC.assert_lse_tracks(lse, lse_p, lse64, q, k, SCALE, name + " lse")

    args = (q, k, v, o, lse, do, SCALE)
    g64 = KC.attn_bwd_formula(*args, torch.float64, keep, p)
    if p > 0:
        g_p = [t.to(BF16) for t in
               KC.attn_bwd_formula(*args, torch.float32, keep, p)]
    else:
        g_p = attention._composite_bwd(*args)
    KC.assert_dq_tracks(dq, g_p[0], g64[0],
                        KC.dq_token0_bound(k, v, do, SCALE, p), K,
                        KC.CAP_ATTN_GRAD, name + " dq")
    KC.assert_tracks(dk, g_p[1], g64[1], -1, K, KC.CAP_ATTN_GRAD, name + " dk")
    KC.assert_tracks(dv, g_p[2], g64[2], -1, K, KC.CAP_ATTN_GRAD, name + " dv")


def record(path=GOLDEN):
    """Write the digests of the build that is importable now."""
    cases = {_name(*c): _digests(c) for c in CASES}
    with open(path, "w") as f:
        json.dump({"scale": SCALE, "p_drop": P_DROP, "seed": SEED,
                   "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    return cases


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        for n, d in record().items():
            print(n, d["outputs"]["dk"][:16])
