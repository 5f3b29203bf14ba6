"""Isolated LayerNorm fwd/bwd timing at GPT-2 medium shapes (within-box
tuning of the launcher knobs TDSA_LN_ROWWAVE / TDSA_LN_RW_WAVES /
TDSA_LN_STRIPES / TDSA_LN_GRID).

The launchers read their knobs per launch, so the row-per-wave path
(TDSA_LN_ROWWAVE=1) and the workgroup-per-row path (=0) are alternated
inside one process, --rounds times each, and every round is printed: the
spread of the rounds is the noise a difference has to beat. The HIP
candidates are called directly (no autotuner in between).

  python scripts/bench_ln.py [--rounds 5] [--M 32768] [--N 1024]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch

from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.ops.gelu import gelu_fwd_hip
from tiny_deepspeed_amd.ops import layernorm as L


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--M", type=int, default=32768)
    ap.add_argument("--N", type=int, default=1024)
    args = ap.parse_args()
    M, N = args.M, args.N
    bf = torch.bfloat16
    x = torch.randn(M, N, device="cuda", dtype=bf)
    res = torch.randn_like(x)
    w = torch.randn(N, device="cuda", dtype=bf)
    b = torch.randn(N, device="cuda", dtype=bf)
    dy = torch.randn_like(x)
    dh = torch.randn_like(x)
    _, mean, rstd = L.ln_fwd_hip(x, w, b, 1e-5)

    def full_bwd():
        _, ws = L.ln_dx_hip(dy, x, w, mean, rstd, dh)
        ops.layernorm_dwdb(ws, dtype=bf)

    _, ws0 = L.ln_dx_hip(dy, x, w, mean, rstd, dh)
    stream = M * N * 2  # bytes of one (M, N) bf16 stream
    parts = [
        # name, callable, bytes the algorithm needs
        ("fwd", lambda: L.ln_fwd_hip(x, w, b, 1e-5), 2 * stream),
        ("fwd+res", lambda: L.ln_fwd_res_hip(x, res, w, b, 1e-5), 4 * stream),
        ("bwd dx", lambda: L.ln_dx_hip(dy, x, w, mean, rstd, None), 3 * stream),
        ("bwd dx+dh", lambda: L.ln_dx_hip(dy, x, w, mean, rstd, dh), 4 * stream),
        ("dwdb", lambda: ops.layernorm_dwdb(ws0, dtype=bf), 0),
        ("bwd full", full_bwd, 4 * stream),
    ]
    # reference stream on the same box: the GELU forward at its flagship
    # size (M x 4N, read + write), the 6.1 TB/s kernel of the bench trace
    xg = torch.randn(M, 4 * N, device="cuda", dtype=bf)
    t_gelu = timeit(lambda: gelu_fwd_hip(xg))
    gelu_rate = 2 * xg.numel() * 2 / t_gelu / 1e6
    del xg
    print(f"shape ({M}, {N}) bf16; gelu_fwd ({M}, {4 * N}) {t_gelu:7.1f} us "
          f"= {gelu_rate:5.2f} TB/s")
    times = {(name, knob): [] for name, _, _ in parts for knob in "01"}
    for _ in range(args.rounds):
        for knob in "01":
            os.environ["TDSA_LN_ROWWAVE"] = knob
            for name, fn, _ in parts:
                times[(name, knob)].append(timeit(fn))
    os.environ.pop("TDSA_LN_ROWWAVE", None)
    for name, _, nbytes in parts:
        for knob in "01":
            ts = times[(name, knob)]
            med = sorted(ts)[len(ts) // 2]
            rate = nbytes / med / 1e6
            rounds = " ".join(f"{t:6.1f}" for t in ts)
            print(f"{name:10s} ROWWAVE={knob}  median {med:6.1f} us  "
                  f"{rate:5.2f} TB/s ({100 * rate / gelu_rate:3.0f}% of gelu)  "
                  f"rounds: {rounds}")


if __name__ == "__main__":
    main()
