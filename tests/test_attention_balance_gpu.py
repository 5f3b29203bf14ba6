"""Every workgroup -> tile mapping of the attention kernels gives the bits of
the one-tile-per-workgroup kernels it replaced.

tests/golden/attention_balance_bits.json holds SHA-256 digests of the raw
bytes of o, lse, dq, dk, dv (and of the inputs q, k, v, do), recorded from the
build of commit 1c7d739 ("Attention: one-instruction bf16 packs, lse/delta
prefetched in dK/dV"), the last one with one tile per workgroup, a grid of
(T / rows per workgroup, B * H) and two-byte epilogue stores. Pairing tiles
and storing whole rows changes which workgroup computes a tile and how its
result reaches memory, no arithmetic operation and no order of operations,
and the kernels have no atomics: the bits must not move. To record again from
the build that is importable now:

    python -m tests.test_attention_balance_gpu --record

The cases are the grid geometries that tests/test_attention_bits_gpu.py does
not reach; gx is the number of tiles (workgroups of the old grid) along T:

  (B, H, T)      waves  gx  XCD remap  dropout p
  (1, 8, 768)    8      3   on         0 and 0.3   odd: the middle tile runs alone
  (1, 8, 1024)   8      4   on         0 and 0.3   two pairs per head
  (1, 3, 1024)   8      4   off        0           B*H % 8 != 0
  (1, 8, 640)    4      5   on         0
  (1, 8, 320)    2      5   on         0
  (4, 16, 1024)  8      4   on         0           256 workgroups of one tile

TDSA_ATTN_BALANCE: 0 is one tile per workgroup in the old order, 2 one tile
per workgroup with the heaviest tiles of the grid first, 1 (the default) tile
pairs where the halved grid still fills the device and 2 otherwise. All the
cases above are on the "otherwise" side, (4, 16, 1024) with its 128 pairs
included, so -1 asks for pairs whatever the grid. Every case runs under all
four values. Inputs come from kernel_check.attn_inputs, outputs
are written into NaN-filled buffers. T = 768, 640 and 320 take the spike
input: lse then differs strongly between tiles, and a pass that kept
anything of the tile before it cannot pass.
"""

import functools
import hashlib
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
KNOB = "TDSA_ATTN_BALANCE"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "attention_balance_bits.json")
INPUTS = ("q", "k", "v", "do")
OUTPUTS = ("o", "lse", "dq", "dk", "dv")

# (B, H, T, spike, p)
CASES = [
    (1, 8, 768, True, 0.0),
    (1, 8, 768, True, P_DROP),
    (1, 8, 1024, False, 0.0),
    (1, 8, 1024, False, P_DROP),
    (1, 3, 1024, False, 0.0),
    (1, 8, 640, True, 0.0),
    (1, 8, 320, True, 0.0),
    (4, 16, 1024, False, 0.0),
]
MODES = (0, 1, 2, -1)


def _name(B, H, T, spike, p):
    return f"B{B}H{H}T{T}" + ("spike" if spike else "") + f"p{p}"


def _digest(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == BF16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=BF16)


class _balance:
    """TDSA_ATTN_BALANCE for the calls inside (None: unset); the launchers
    read it at every launch."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = os.environ.get(KNOB)
        if self.mode is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = str(self.mode)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.old


@functools.lru_cache(maxsize=None)
def _inputs(B, H, T, spike):
    return KC.attn_inputs(B, H, T, "cuda", seed=T + H, spike=spike)


def _run(case, mode):
    """Forward and backward through the extension into NaN-filled buffers."""
    assert torch.cuda.is_available()
    assert _ext.ext_available(), "HIP extension must be built (no eager fallback)"
    ext = _ext.get_ext()
    B, H, T, spike, p = case
    q, k, v, do = _inputs(B, H, T, spike)
    seed = SEED if p > 0 else 0
    with _balance(mode):
        o, lse = ext.attention_fwd(q, k, v, SCALE, _nan(*q.shape), p, seed)
        dq, dk, dv = ext.attention_bwd(q, k, v, o, lse, do, SCALE,
                                       _nan(*q.shape), _nan(*q.shape),
                                       _nan(*q.shape), p, seed)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"balance{m}")
@pytest.mark.parametrize("case", CASES, ids=lambda c: _name(*c))
def test_attention_mapping_keeps_recorded_bits_gpu(case, mode):
    want = _golden()[_name(*case)]
    got_in = dict(zip(INPUTS, map(_digest, _inputs(*case[:4]))))
    # a change of inputs (generator, seeds) is not a change of kernel
    assert got_in == want["inputs"], "inputs differ from the recorded ones"
    outs = _run(case, mode)
    for name, t in zip(OUTPUTS, outs):
        assert torch.isfinite(t.float()).all(), name
    got = dict(zip(OUTPUTS, map(_digest, outs)))
    differ = [n for n in OUTPUTS if got[n] != want["outputs"][n]]
    assert not differ, (f"{_name(*case)} {KNOB}={mode}: bits of {differ} "
                        "differ from the record")


def record(path=GOLDEN):
    """Write the digests of the build that is importable now."""
    cases = {}
    for c in CASES:
        cases[_name(*c)] = {
            "inputs": dict(zip(INPUTS, map(_digest, _inputs(*c[:4])))),
            "outputs": dict(zip(OUTPUTS, map(_digest, _run(c, None)))),
        }
    with open(path, "w") as f:
        json.dump({"scale": SCALE, "p_drop": P_DROP, "seed": SEED,
                   "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    return cases


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--record"]
        for n, d in record(*rest[:1]).items():
            print(n, d["outputs"]["dk"][:16])
