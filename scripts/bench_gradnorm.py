"""Gradient-norm pass and clipped optimizer step at gpt2-medium size.

Part 1, the norm pass: ops.grad_sumsq (csrc/kernels/gradnorm.hip) over the
model's parameter list with bf16 gradients, against what
torch.nn.utils.clip_grad_norm_ runs on the same tensors (torch._foreach_norm,
stack, vector_norm). Part 2, the step: AdamW.step() on the same list with
synthetic gradients and no model, with and without max_grad_norm.

Compared versions are alternated inside one process, --rounds times each, and
every round is printed: the spread of the rounds is the noise a difference
has to beat. Times are device events around back-to-back calls, so the norm
pass includes its descriptor upload; the kernels' own time comes from a
kernel trace of this script (--trace-only runs few iterations for that).

  python scripts/bench_gradnorm.py [--rounds 5] [--model gpt2_medium]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch

from tiny_deepspeed_amd import AdamW, ops
from tiny_deepspeed_amd.models import GPTConfig, GPT2Model

HBM_PEAK_TBS = 8.0      # spec; 6.29 TB/s is what a float4 copy reaches
HBM_COPY_TBS = 6.29


def timeit(fn, iters, warmup):
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


def report(name, ts, nbytes):
    med = sorted(ts)[len(ts) // 2]
    rate = nbytes / med / 1e6
    rounds = " ".join(f"{t:8.1f}" for t in ts)
    print(f"{name:26s} median {med:8.1f} us  (min {min(ts):8.1f} max "
          f"{max(ts):8.1f})  {rate:5.2f} TB/s = {100 * rate / HBM_PEAK_TBS:3.0f}% "
          f"of {HBM_PEAK_TBS} TB/s peak, {100 * rate / HBM_COPY_TBS:3.0f}% of the "
          f"{HBM_COPY_TBS} TB/s copy rate  rounds: {rounds}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model", default="gpt2_medium")
    ap.add_argument("--trace-only", action="store_true",
                    help="3 calls of each version and no timing (for a "
                         "kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert ops.ext_available(), "needs the built HIP extension"

    with torch.device("meta"):
        shapes = [tuple(p.shape) for p in
                  GPT2Model(getattr(GPTConfig, args.model)()).parameters()]
    gen = torch.Generator(device="cuda").manual_seed(0)
    grads = [(torch.randn(s, device="cuda", generator=gen) * 1e-3)
             .to(torch.bfloat16) for s in shapes]
    numel = sum(g.numel() for g in grads)
    print(f"{args.model}: {len(grads)} tensors, {numel} elements, "
          f"{2 * numel / 1e9:.3f} GB of bf16 gradients")

    def ours():
        return ops.grad_sumsq(grads).sqrt()

    def torch_route():
        return torch.linalg.vector_norm(
            torch.stack(torch._foreach_norm(grads, 2.0)), 2.0)

    a, b = ours().item(), torch_route().item()
    ref = sum(g.double().pow(2).sum() for g in grads).sqrt().item()
    print(f"norm: ours {a:.8f}  torch {b:.8f}  fp64 {ref:.8f}  "
          f"rel err ours {abs(a - ref) / ref:.2e} torch {abs(b - ref) / ref:.2e}")

    if args.trace_only:
        for _ in range(3):
            ours()
            torch_route()
        torch.cuda.synchronize()
    else:
        print("## norm pass (read 2 B per element)")
        times = {"ours": [], "torch": []}
        for _ in range(args.rounds):
            times["ours"].append(timeit(ours, args.iters, 5))
            times["torch"].append(timeit(torch_route, args.iters, 5))
        report("ops.grad_sumsq + sqrt", times["ours"], 2 * numel)
        report("_foreach_norm+stack+norm", times["torch"], 2 * numel)

    # ---- the optimizer step, with and without clipping -----------------------
    def make(max_grad_norm):
        ps = [(f"p{i}", torch.nn.Parameter(
            torch.zeros(s, device="cuda", dtype=torch.bfloat16)))
            for i, s in enumerate(shapes)]
        # a threshold the gradients exceed, so the scaled update runs
        return ps, AdamW(ps, lr=1e-4, weight_decay=0.1,
                         max_grad_norm=max_grad_norm)

    runs = {"unclipped": make(None), "max_grad_norm=0.5": make(0.5)}

    def step_of(name):
        ps, opt = runs[name]

        def step():
            for (_, p), g in zip(ps, grads):
                p.grad = g
            opt.step()
        return step

    if args.trace_only:
        for name in runs:
            for _ in range(3):
                step_of(name)()
        torch.cuda.synchronize()
        return
    print("## AdamW.step(), bf16 params and grads: 30 B per element of the "
          "update, + 2 B for the norm pass")
    times = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name in runs:
            times[name].append(timeit(step_of(name), args.iters, 3))
    med = {}
    for name, nb in (("unclipped", 30), ("max_grad_norm=0.5", 32)):
        med[name] = report(f"step {name}", times[name], nb * numel)
    d = med["max_grad_norm=0.5"] - med["unclipped"]
    print(f"clipping adds {d:.1f} us per step "
          f"({100 * d / med['unclipped']:.1f}%); last_grad_norm "
          f"{runs['max_grad_norm=0.5'][1].last_grad_norm.item():.6f}")


if __name__ == "__main__":
    main()
