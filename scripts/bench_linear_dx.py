"""Linear dX: transpose + forward-layout GEMM (dx_nt) vs the library's NN GEMM
(dx_library) on gpt2-medium's weights at M = B*T = 32768, and the transpose
kernel alone against torch's strided copy.

The measurement behind the `linear_dx` candidate list of ops/linear.py. Each
figure is the median of --reps hipEvent-timed batches of --iters back-to-back
calls after a warm-up, so a single slow batch does not move it. TunableOp is
pointed at the committed tuned/ cache the way bench.py does it, so the GEMMs
are the ones a training step runs. Run on an MI355X:
    python scripts/bench_linear_dx.py [--iters 50] [--reps 5]
"""

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_TUNED = os.path.join(ROOT, "tuned", "tunableop.csv")
if (os.path.exists(_TUNED.replace(".csv", "0.csv"))
        and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ):
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = _TUNED

import torch

from tiny_deepspeed_amd.ops import get_ext
from tiny_deepspeed_amd.ops import linear as linear_ops
from tiny_deepspeed_amd.ops.autotuner import RuntimeAutoTuner

M = 32768
# (name, N = out_features, K = in_features) of W[N, K]
WEIGHTS = [
    ("attn.c_attn", 3072, 1024),
    ("attn.c_proj", 1024, 1024),
    ("mlp.c_fc", 4096, 1024),
    ("mlp.c_proj", 1024, 4096),
    ("lm_head", 50304, 1024),
]


def time_fn(fn, iters, reps, warmup=10):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) / iters)
    return statistics.median(out)  # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ext = get_ext()
    torch.manual_seed(0)

    print("dX candidates, M = %d (ms; TF/s of the 2*M*N*K product)" % M)
    print(f"{'weight':>12} {'N':>6} {'K':>5} {'nt_ms':>8} {'nt_TF':>6} "
          f"{'lib_ms':>8} {'lib_TF':>6} {'saved':>7} {'tuner':>11}")
    for name, N, K in WEIGHTS:
        dy = torch.randn(M, N, device="cuda", dtype=torch.bfloat16) * 0.05
        w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
        assert linear_ops._dx_nt_supported(dy, w)
        iters = max(5, args.iters // 5) if N > 8192 else args.iters
        nt = time_fn(lambda: linear_ops.dx_nt(dy, w), iters, args.reps)
        lib = time_fn(lambda: linear_ops.dx_library(dy, w), iters, args.reps)
        tuner = RuntimeAutoTuner()
        linear_ops.linear_input_grad(dy, w, tuner=tuner)
        (won,) = tuner.choices().values()
        flop = 2.0 * M * N * K
        print(f"{name:>12} {N:>6} {K:>5} {nt:8.4f} {flop/nt/1e9:6.0f} "
              f"{lib:8.4f} {flop/lib/1e9:6.0f} {lib-nt:7.4f} {won:>11}")
        del dy, w

    print()
    print("transpose alone (us; TB/s counts the read and the write)")
    print(f"{'weight':>12} {'N':>6} {'K':>5} {'hip_us':>8} {'hip_TBs':>8} "
          f"{'torch_us':>9} {'torch_TBs':>9}")
    for name, N, K in WEIGHTS:
        w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16)
        hip = time_fn(lambda: ext.transpose_bf16(w), args.iters, args.reps)
        ref = time_fn(lambda: w.t().contiguous(), args.iters, args.reps)
        assert torch.equal(ext.transpose_bf16(w), w.t().contiguous())
        byts = 2.0 * w.numel() * 2
        print(f"{name:>12} {N:>6} {K:>5} {hip*1e3:8.2f} {byts/hip/1e9:8.2f} "
              f"{ref*1e3:9.2f} {byts/ref/1e9:9.2f}")

    # the stream yardstick: gelu_fwd reads and writes one bf16 tensor
    x = torch.randn(M, 4096, device="cuda", dtype=torch.bfloat16)
    g = time_fn(lambda: ext.gelu_fwd(x), args.iters, args.reps)
    print(f"gelu_fwd {M}x4096: {g*1e3:.2f} us, "
          f"{2.0 * x.numel() * 2 / g / 1e9:.2f} TB/s")
    # launch floor: the same kernel on one 64x64 tile
    t = torch.randn(64, 64, device="cuda", dtype=torch.bfloat16)
    one = time_fn(lambda: ext.transpose_bf16(t), args.iters, args.reps)
    print(f"transpose 64x64 (one tile, allocation + launch): {one*1e3:.2f} us")


if __name__ == "__main__":
    main()
