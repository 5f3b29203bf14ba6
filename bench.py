"""Flagship benchmark: GPT-2 ZeRO-2 training throughput (tokens/sec, whole job).

Driver contract:
    python bench.py --gpus N --steps K --warmup W
For N > 1 the driver launches this under torch.distributed.run with one rank
per GPU (RCCL over xGMI). Measures W untimed warmup steps, then exactly K
steps bracketed by barrier + torch.cuda.synchronize() on both sides, takes
the MAX elapsed over ranks, and rank 0 prints ONE JSON line.

A plain run does only that: set up, warm up, time the K steps, print. Two
options add to it:
    --dump-outputs DIR  rank 0 writes the loss, logits and updated parameters
                        of the last timed step as DIR/<name>.npy (float32,
                        seeded samples of the large tensors) so two builds
                        can be compared output for output; the inputs are
                        seeded and identical from run to run
    --full              everything the benchmark measures beyond the headline
                        figure belongs behind this flag (nothing today)

Metric/config per BASELINE.json: tokens/sec (whole node), GPT-2 ZeRO-2,
synthetic data, random-init weights, bf16 compute with fp32 accumulation and
fp32 optimizer state. Weak scaling: per-GPU batch is fixed as N grows.
"""

import argparse
import json
import os
import sys
import time
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# hipBLASLt/rocBLAS algorithm selection: use the committed TunableOp cache
# (read-only — tuning itself takes minutes and was done offline; +4% over
# the default heuristics on the GPT-2 medium shapes). torch inserts the
# device ordinal before the extension, so tuned/ ships one copy per GPU.
_TUNED = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "tuned", "tunableop.csv")
if (os.path.exists(_TUNED.replace(".csv", "0.csv"))
        and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ):
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = _TUNED

import torch
import torch.distributed as dist

from tiny_deepspeed_amd.models import GPTConfig, GPT2Model
from tiny_deepspeed_amd import (
    Single, AdamW,
    DDP, DDPAdamW,
    Zero1, Zero1AdamW,
    Zero2, Zero2AdamW,
    Zero3, Zero3AdamW,
    Zero2Flat, Zero2FlatAdamW,
    partition_tensors,
)

WRAPPERS = {
    "single": (Single, AdamW),
    "ddp": (DDP, DDPAdamW),
    "zero1": (Zero1, Zero1AdamW),
    "zero2": (Zero2, Zero2AdamW),
    "zero3": (Zero3, Zero3AdamW),
    "zero2flat": (Zero2Flat, Zero2FlatAdamW),
}


# --dump-outputs sample sizes: 4M logits + 16K per parameter tensor keeps the
# dump at 24 MB for gpt2-medium (under the 64 MB cap for every preset)
_DUMP_LOGITS = 1 << 22
_DUMP_PER_PARAM = 1 << 14
_DUMP_SEED = 20240


def _sample_flat(t, k, gen):
    """float32 copy of `t` flattened; a fixed seeded sample of k elements
    (sorted flat indices) when it holds more than k."""
    flat = t.detach().reshape(-1)
    if flat.numel() > k:
        idx = torch.randint(0, flat.numel(), (k,), generator=gen)
        flat = flat[idx.sort().values.to(flat.device)]
    return flat.float().cpu().numpy()


def dump_outputs(out_dir, loss, logits, named_params):
    """Write what the last timed step handed back: the loss, the logits (None
    on the fused lm_head path, then omitted) and the updated parameters.
    The sample indices depend only on the seed and the tensor shapes, so two
    runs with the same arguments write element-for-element comparable files."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    gen = torch.Generator().manual_seed(_DUMP_SEED)
    np.save(os.path.join(out_dir, "loss.npy"),
            loss.detach().float().cpu().numpy())
    if logits is not None:
        np.save(os.path.join(out_dir, "logits.npy"),
                _sample_flat(logits, _DUMP_LOGITS, gen))
    params = [_sample_flat(p, _DUMP_PER_PARAM, gen)
              for _, p in named_params if p.numel() > 0]
    np.save(os.path.join(out_dir, "params.npy"), np.concatenate(params))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--model", default="gpt2-medium")
    p.add_argument("--batch", type=int, default=32, help="per-GPU micro batch")
    p.add_argument("--seq", type=int, default=1024)
    p.add_argument("--parallel", default="zero2",
                   choices=list(WRAPPERS.keys()))
    p.add_argument("--fused-lmhead", type=int, default=0,
                   help="1: row-chunked fused lm_head+CE (-2.75 GB peak, "
                        "+4 ms/step at gpt2-medium b32); 0: materialized "
                        "logits (default, throughput headline)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed "
                        "step computed (loss, logits, updated parameters) "
                        "as DIR/<name>.npy in float32; large tensors are "
                        "written as a fixed seeded sample. Rank 0 writes "
                        "its own view: with more than one GPU under zero1/"
                        "zero2/zero3 that is rank 0's logits and whatever "
                        "rank 0 holds of the parameters (shards it does "
                        "not own may be stale or empty)")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements and checks that the "
                        "headline figure does not need (none today: a plain "
                        "run already does only setup, warmup, the timed "
                        "steps and the result line)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    have_gpu = torch.cuda.is_available()
    world_size = int(os.getenv("WORLD_SIZE", "1"))
    rank = int(os.getenv("RANK", "0"))
    local_rank = int(os.getenv("LOCAL_RANK", str(rank)))
    distributed = world_size > 1
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        dist.init_process_group(backend="nccl" if have_gpu else "gloo",
                                init_method="env://", world_size=world_size,
                                rank=rank)
    if have_gpu:
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        dtype = torch.bfloat16
    else:
        device = torch.device("cpu")
        dtype = torch.float32
        # CPU run is a plumbing check only (BASELINE.json config #1):
        # shrink so it completes in seconds.
        args.model = "gpt2-small"
        args.batch = 1
        args.seq = min(args.seq, 64)

    model_name = args.model
    config = GPTConfig.named(model_name, block_size=max(args.seq, 64),
                             fused_lm_head=bool(args.fused_lmhead))

    torch.manual_seed(1234)
    model = GPT2Model(config).to(device=device, dtype=dtype)

    wrapper_cls, optim_cls = WRAPPERS[args.parallel]
    if args.parallel == "zero2flat":
        wrapped = wrapper_cls(model)
        optimizer = optim_cls(wrapped, lr=1e-5, weight_decay=0.1)
    elif args.parallel in ("zero1", "zero2", "zero3"):
        ranks_map = [f"cuda:{i}" if have_gpu else "cpu"
                     for i in range(world_size)]
        with torch.device("meta"):
            parts, _ = partition_tensors(
                OrderedDict(GPT2Model(config).named_parameters()),
                ranks_map=ranks_map, evenness_priority=0, verbose=False,
            )
        wrapped = wrapper_cls(model, parts)
        optimizer = optim_cls(wrapped.named_parameters(), lr=1e-5,
                              weight_decay=0.1, param_part_table=parts,
                              ranks_map=ranks_map)
    elif args.parallel == "ddp":
        wrapped = wrapper_cls(model)
        optimizer = optim_cls(wrapped.named_parameters(), lr=1e-5,
                              weight_decay=0.1)
    else:
        wrapped = wrapper_cls(model)
        optimizer = optim_cls(wrapped.named_parameters(), lr=1e-5,
                              weight_decay=0.1)

    g = torch.Generator().manual_seed(4242 + rank)
    x = torch.randint(0, config.vocab_size, (args.batch, args.seq),
                      generator=g).to(device)
    y = torch.randint(0, config.vocab_size, (args.batch, args.seq),
                      generator=g).to(device)

    last = {}

    def step(keep=False):
        wrapped.require_backward_grad_sync = True
        logits, loss = wrapped(x, y)
        loss.backward()
        optimizer.step()
        if keep:
            # only the last timed step holds on to its logits, so the
            # steps before it free them exactly as a plain run does
            last["logits"], last["loss"] = logits, loss
        return loss

    for _ in range(args.warmup):
        step()

    if distributed:
        dist.barrier()
    if have_gpu:
        torch.cuda.synchronize()
        # report steady-state peak memory: warmup includes one-time autotuner
        # candidate timing whose composite transients never recur
        torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    dump = args.dump_outputs is not None and rank == 0
    for i in range(args.steps):
        step(keep=dump and i == args.steps - 1)
    if have_gpu:
        torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device
                         if have_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if dump:
        dump_outputs(args.dump_outputs, last["loss"], last["logits"],
                     wrapped.named_parameters())

    n_gpus = world_size if have_gpu else args.gpus
    tokens_per_step = args.batch * args.seq * world_size
    value = tokens_per_step * args.steps / elapsed
    if distributed and rank == 0:
        # diagnostic for multi-GPU runs (stderr; the stdout JSON contract
        # is untouched): per-step collective counts and payload GB
        comm = getattr(wrapped, "comm", None)
        if comm is not None and comm.stats:
            total = args.warmup + args.steps
            stats = {k: {"per_step": round(v[0] / total, 1),
                         "gb_per_step": round(v[1] / total / 2**30, 3)}
                     for k, v in sorted(comm.stats.items())}
            print(f"[comm-stats world={world_size}] {json.dumps(stats)}",
                  file=sys.stderr)
    if rank == 0:
        out = {
            "metric": "tokens/sec (whole node) GPT-2 ZeRO-2",
            "value": round(value, 1),
            "unit": "tokens/s",
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000.0, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "bf16" if dtype == torch.bfloat16 else "fp32",
            "data": "synthetic",
            "config": {
                "model": model_name,
                "global_batch": args.batch * world_size,
                "seq_len": args.seq,
                "parallelism": f"{args.parallel}-dp{world_size}",
                "peak_hbm_gb": round(
                    torch.cuda.max_memory_allocated() / 2**30, 2
                ) if have_gpu else None,
            },
        }
        print(json.dumps(out))

    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
