"""Isolated SwiGLU fwd/bwd timing at (M, F) bf16, F = 2816 and 4096 by
default (the "swiglu" MLP widths of n_embd 1024 and 1536).

Three ways, alternated inside each round of one process, every round printed
(the spread of the rounds is the noise a difference has to beat):
  a = the HIP kernels (swiglu_fwd_hip / swiglu_bwd_hip, no autotuner between),
  b = the op's torch candidate (fp32 math, one rounding),
  c = what a user writes without the op: F.silu(gate) * up under autograd.
The yardstick is gelu_fwd of the same session at (M, 4096): one stream in, one
out. Bytes the algorithm needs per row: 6F forward (gate, up in; y out), 10F
backward (dy, gate, up in; dgate, dup out).

  python scripts/bench_swiglu.py [--rounds 5] [--M 32768] [--F 2816 4096]
                                 [--grids 1024 ...]

--grids alternates TDSA_SWIGLU_GRID caps for the HIP kernels as well.
"""

import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch
import torch.nn.functional as F_

from tiny_deepspeed_amd.ops.gelu import gelu_fwd_hip

# ops.swiglu is the function; the module is wanted
S = importlib.import_module("tiny_deepspeed_amd.ops.swiglu")


def timeit(fn, iters=50, warmup=10):
    """Mean µs per call from device events around `iters` back-to-back calls."""
    for _ in range(warmup):
        fn()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def with_grid(grid, fn):
    def run():
        os.environ["TDSA_SWIGLU_GRID"] = str(grid)
        fn()
    return run


def bench_shape(M, F, rounds, grids, gelu_rate):
    bf = torch.bfloat16
    gu = torch.randn(M, 2 * F, device="cuda", dtype=bf)
    dy = torch.randn(M, F, device="cuda", dtype=bf)
    gu_req = gu.clone().requires_grad_(True)

    def plain_fwd():
        g, u = gu_req.chunk(2, dim=-1)
        return F_.silu(g) * u

    y_graph = plain_fwd()
    parts = []
    for grid in grids:
        tag = f"a hip grid {grid}"
        parts.append((f"{tag} fwd", with_grid(grid, lambda: S.swiglu_fwd_hip(gu)), 6))
        parts.append((f"{tag} bwd", with_grid(grid, lambda: S.swiglu_bwd_hip(dy, gu)), 10))
    parts += [
        ("b torch candidate fwd", lambda: S.swiglu_fwd_torch(gu), 6),
        ("b torch candidate bwd", lambda: S.swiglu_bwd_torch(dy, gu), 10),
        ("c F.silu(g)*u fwd", plain_fwd, 6),
        ("c F.silu(g)*u autograd bwd", lambda: torch.autograd.grad(
            y_graph, gu_req, dy, retain_graph=True), 10),
    ]
    times = {name: [] for name, _, _ in parts}
    for _ in range(rounds):
        for name, fn, _ in parts:
            times[name].append(timeit(fn))
    os.environ.pop("TDSA_SWIGLU_GRID", None)
    print(f"shape ({M}, {F}) bf16, gu ({M}, {2 * F})")
    for name, _, per_row in parts:
        ts = times[name]
        med = sorted(ts)[len(ts) // 2]
        rate = per_row * F * M / med / 1e6
        print(f"{name:28s} median {med:7.1f} us  {rate:5.2f} TB/s "
              f"({100 * rate / gelu_rate:3.0f}% of gelu)  rounds: "
              + " ".join(f"{t:7.1f}" for t in ts))
    for d in ("fwd", "bwd"):
        hip = [times[n] for n, _, _ in parts if n.startswith("a") and n.endswith(d)]
        rest = [times[n] for n, _, _ in parts if n[0] in "bc" and n.endswith(d)]
        wins = all(min(h[r] for h in hip) < min(o[r] for o in rest)
                   for r in range(rounds))
        print(f"  {d}: HIP fastest in every round: {wins}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--M", type=int, default=32768)
    ap.add_argument("--F", type=int, nargs="+", default=[2816, 4096])
    ap.add_argument("--grids", type=int, nargs="+", default=[1024])
    args = ap.parse_args()
    xg = torch.randn(args.M, 4096, device="cuda", dtype=torch.bfloat16)
    t_gelu = timeit(lambda: gelu_fwd_hip(xg))
    gelu_rate = 2 * xg.numel() * 2 / t_gelu / 1e6
    print(f"gelu_fwd ({args.M}, 4096) {t_gelu:7.1f} us = {gelu_rate:5.2f} TB/s")
    del xg
    for F in args.F:
        bench_shape(args.M, F, args.rounds, args.grids, gelu_rate)


if __name__ == "__main__":
    main()
