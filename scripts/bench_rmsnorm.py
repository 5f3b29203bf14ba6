"""Isolated RMSNorm fwd/bwd timing, three variants alternated per round in
one process (every round is printed: the spread is the noise a difference
has to beat). The HIP candidates are called directly, no autotuner.

  a  the RMSNorm kernels: forward with res; dx+dh plus the dw reduce
  b  the torch composite a raw nn.RMSNorm model runs: F.rms_norm after an
     explicit add, and its autograd backward with both output gradients
  c  N <= 2048 only: the LayerNorm row-per-wave kernels at the same shape

  python scripts/bench_rmsnorm.py [--rounds 5] [--M 32768] [--N 1024 4096]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch
import torch.nn.functional as F

from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.ops import layernorm as L
from tiny_deepspeed_amd.ops import rmsnorm as R
from bench_ln import timeit


def bench(M, N, rounds):
    bf = torch.bfloat16
    x = torch.randn(M, N, device="cuda", dtype=bf)
    res, dy, dh = (torch.randn_like(x) for _ in range(3))
    w = torch.randn(N, device="cuda", dtype=bf)
    b = torch.randn(N, device="cuda", dtype=bf)
    h, _, rstd = R.rms_fwd_res_hip(x, res, w, 1e-5)

    def a_bwd():
        _, ws = R.rms_dx_hip(dy, h, w, rstd, dh)
        ops.rmsnorm_dw(ws, dtype=bf)

    xg, rg, wg = (t.clone().requires_grad_(True) for t in (x, res, w))

    def b_fwd():
        hh = xg + rg
        return hh, F.rms_norm(hh, (N,), wg, 1e-5)

    outs = b_fwd()

    def b_bwd():
        torch.autograd.grad(outs, (xg, rg, wg), (dh, dy), retain_graph=True)

    parts = [("a fwd+res", lambda: R.rms_fwd_res_hip(x, res, w, 1e-5)),
             ("a bwd full", a_bwd),
             ("b fwd+res", b_fwd),
             ("b bwd full", b_bwd)]
    if N <= 2048:
        _, _, mean, lrstd = L.ln_fwd_res_hip(x, res, w, b, 1e-5)

        def c_bwd():
            _, ws = L.ln_dx_hip(dy, h, w, mean, lrstd, dh)
            ops.layernorm_dwdb(ws, dtype=bf)

        parts += [("c fwd+res", lambda: L.ln_fwd_res_hip(x, res, w, b, 1e-5)),
                  ("c bwd full", c_bwd)]
    times = {name: [] for name, _ in parts}
    for _ in range(rounds):
        for name, fn in parts:
            times[name].append(timeit(fn))
    geo = ops.get_ext().rmsnorm_geometry(M, N, True)
    print(f"shape ({M}, {N}) bf16, geometry (G, fwd units, fwd R, bwd R, "
          f"span, bound) = {tuple(geo)}")
    stream = M * N * 2  # fwd+res and dx+dh each move four (M, N) bf16 streams
    for name, _ in parts:
        ts = times[name]
        med = sorted(ts)[len(ts) // 2]
        print(f"{name:12s} median {med:7.1f} us  {4 * stream / med / 1e6:5.2f} "
              f"TB/s of 4 streams  range {min(ts):7.1f}-{max(ts):7.1f}  "
              f"rounds: {' '.join(f'{t:7.1f}' for t in ts)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--M", type=int, default=32768)
    ap.add_argument("--N", type=int, nargs="+", default=[1024, 1600, 4096, 8192])
    args = ap.parse_args()
    for N in args.N:
        bench(args.M, N, args.rounds)


if __name__ == "__main__":
    main()
