"""Isolated attention kernel benchmark (fwd / bwd), with TF/s accounting.

Usage (GPU box): python scripts/bench_attn.py [--T 1024] [--B 8] [--H 16]
                                               [--D 64|128]
Any T at either head dim: a length that is no multiple of 64 runs the ragged
entry points (the tail kernels); --D 128 runs attention_d128_* of the
extension. Each figure is the mean over --iters calls between two device
events, after warm-up. Causal flops: ~0.5 * 2 gemms * 2*B*H*T^2*D each for
fwd; bwd ~2.5x fwd.

    --tree DIR     import the package from another checkout (A/B runs of two
                   builds in one session, alternating)
    --composite    also time ops.attention._composite_fwd/_bwd, the path that
                   ragged T took before the tail kernels (fp32 (B,H,T,T)
                   scores: pick a --B that fits)
    --composite-only   time nothing else (a --tree whose extension has no
                   kernels for the shape, such as head dim 128 at ragged T
                   before its tail kernels)
    --dropout P    fused dropout at rate P with a fixed seed (either head dim;
                   default 0: the kernels without dropout). With --composite
                   the composite is then the op layer's torch-dropout path
                   (bf16 scores, fp32 softmax, torch dropout, autograd
                   backward), which head dim 128 took before its DROP kernels
    --sdpa         also time torch's scaled_dot_product_attention, forward
                   and backward (autograd)
    --kv-heads N   grouped-query attention at --D 128 with N K/V heads (N
                   divides --H, no dropout): besides the multi-head kernels at
                   H heads (the yardstick) each round times the grouped-query
                   entry points ("gqa") and what the same call costs without
                   them ("expanded": K/V repeated G-fold, the multi-head
                   kernels, dK/dV summed over each group in fp32), and prints
                   the memory the expanded call allocates on top. "expanded"
                   needs no grouped-query kernel, so it also runs on a --tree
                   that has none
    --rounds N     repeat the whole set N times, the alternatives taking turns
                   within a round; with N > 1 a closing line per measurement
                   gives its range over the rounds
"""

import argparse
import importlib
import math
import os
import sys


def timeit(fn, iters=20, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3 / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--B", type=int, default=8)
    p.add_argument("--H", type=int, default=16)
    p.add_argument("--T", type=int, default=1024)
    p.add_argument("--D", type=int, default=64, choices=(64, 128))
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--dropout", type=float, default=0.0)
    p.add_argument("--rounds", type=int, default=1)
    p.add_argument("--kv-heads", type=int, default=0)
    p.add_argument("--tree", default=os.path.join(os.path.dirname(__file__), ".."))
    p.add_argument("--composite", action="store_true")
    p.add_argument("--composite-only", action="store_true")
    p.add_argument("--sdpa", action="store_true")
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    _C = importlib.import_module("tiny_deepspeed_amd._C")

    B, H, T, D = args.B, args.H, args.T, args.D
    att = importlib.import_module("tiny_deepspeed_amd.ops.attention")
    names = {(64, False): "attention", (64, True): "attention_ragged",
             (128, False): "attention_d128",
             (128, True): "attention_d128_ragged"}
    name = names[D, T % 64 != 0]
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)
    q = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    drop = {"dropout_p": args.dropout, "seed": 20240607} if args.dropout else {}

    def composite_dropout(q, k, v):
        """The composite dropout branch of ops.attention.causal_attention."""
        s = torch.matmul(q, k.transpose(-2, -1)) * scale
        mask = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
        pm = torch.softmax(s.float(), dim=-1).to(q.dtype)
        pm = torch.nn.functional.dropout(pm, p=args.dropout, training=True)
        return torch.matmul(pm, v)

    Hkv = args.kv_heads
    if Hkv:
        assert D == 128 and not drop and H % Hkv == 0 and T >= 1
        G = H // Hkv
        kg, vg = (t[:, ::G].contiguous() for t in (k, v))
        gqa_fwd = getattr(_C, "attention_d128_gqa_fwd", None)
        gqa_bwd = getattr(_C, "attention_d128_gqa_bwd", None)
        rag_fwd = _C.attention_d128_ragged_fwd
        rag_bwd = _C.attention_d128_ragged_bwd

        def expanded_fwd():
            return rag_fwd(q, kg.repeat_interleave(G, dim=1),
                           vg.repeat_interleave(G, dim=1), scale)

        def expanded_bwd(o, lse, do):
            dq, dk, dv = rag_bwd(q, kg.repeat_interleave(G, dim=1),
                                 vg.repeat_interleave(G, dim=1), o, lse, do,
                                 scale)
            dk, dv = (t.view(B, Hkv, G, T, D).sum(2, dtype=torch.float32)
                      .to(t.dtype) for t in (dk, dv))
            return dq, dk, dv

    if args.composite_only:
        args.composite = True
        o, lse = att._composite_fwd(q, k, v, scale)
    else:
        fwd, bwd = getattr(_C, name + "_fwd"), getattr(_C, name + "_bwd")
        o, lse = fwd(q, k, v, scale, **drop)
    do = torch.randn_like(o)
    # causal effective flops
    f_fwd = 0.5 * 2 * (2 * B * H * T * T * D)
    f_bwd = 0.5 * 5 * (2 * B * H * T * T * D)  # dkv recompute S,dP + dV,dK; dq S,dP,dQ
    tag = f"B{B} H{H} T{T} D{D}" + (f" p{args.dropout}" if drop else "")
    seen = {}   # measurement -> times over the rounds

    def note(name, t):
        seen.setdefault(name, []).append(t)

    for _ in range(args.rounds):
        if not args.composite_only:
            t_fwd = timeit(lambda: fwd(q, k, v, scale, **drop), args.iters)
            t_bwd = timeit(lambda: bwd(q, k, v, o, lse, do, scale, **drop),
                           args.iters)
            note("fwd", t_fwd)
            note("bwd", t_bwd)
            print(f"{tag} fwd: {t_fwd*1e6:8.1f} us  {f_fwd/t_fwd/1e12:7.1f} TF/s (causal-effective)")
            print(f"{tag} bwd: {t_bwd*1e6:8.1f} us  {f_bwd/t_bwd/1e12:7.1f} TF/s (causal-effective)")

        if Hkv:
            gtag = f"{tag} Hkv{Hkv}"
            if gqa_fwd is not None:
                og, lseg = gqa_fwd(q, kg, vg, scale)
                t_gf = timeit(lambda: gqa_fwd(q, kg, vg, scale), args.iters)
                t_gb = timeit(lambda: gqa_bwd(q, kg, vg, og, lseg, do, scale),
                              args.iters)
                note("gqa fwd", t_gf)
                note("gqa bwd", t_gb)
                print(f"{gtag} gqa fwd: {t_gf*1e6:8.1f} us  bwd: {t_gb*1e6:8.1f} us")
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            oe, lsee = expanded_fwd()
            t_ef = timeit(expanded_fwd, args.iters)
            t_eb = timeit(lambda: expanded_bwd(oe, lsee, do), args.iters)
            # on top of what the grouped-query call allocates: o, lse, dq and
            # dk, dv of Hkv heads
            peak = (torch.cuda.max_memory_allocated() - base) / 2**20
            own = (2 * q.numel() + 2 * kg.numel()) * 2 / 2**20
            del oe, lsee
            note("expanded fwd", t_ef)
            note("expanded bwd", t_eb)
            print(f"{gtag} expanded fwd: {t_ef*1e6:8.1f} us  bwd: {t_eb*1e6:8.1f} us  "
                  f"peak memory {peak:.0f} MiB against {own:.0f} MiB of outputs")

        if args.composite:
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            iters = max(3, args.iters // 20)
            if drop:
                leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
                t_cf = timeit(lambda: composite_dropout(q, k, v), iters, 2)
                out = composite_dropout(*leaves)
                t_cb = timeit(lambda: torch.autograd.grad(
                    out, leaves, do, retain_graph=True), iters, 2)
                del out
            else:
                t_cf = timeit(lambda: att._composite_fwd(q, k, v, scale),
                              iters, 2)
                t_cb = timeit(lambda: att._composite_bwd(q, k, v, o, lse, do,
                                                         scale), iters, 2)
            note("composite fwd", t_cf)
            note("composite bwd", t_cb)
            peak = (torch.cuda.max_memory_allocated() - base) / 2**20
            print(f"{tag} composite fwd: {t_cf*1e6:8.1f} us  bwd: {t_cb*1e6:8.1f} us  "
                  f"peak extra memory {peak:.0f} MiB")

        if args.sdpa:
            # rocm flash attention via torch, if available
            def sdpa(*qkv):
                return torch.nn.functional.scaled_dot_product_attention(
                    *qkv, is_causal=True, scale=scale)
            try:
                t_sdpa = timeit(lambda: sdpa(q, k, v), args.iters)
                leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
                out = sdpa(*leaves)
                t_sb = timeit(lambda: torch.autograd.grad(
                    out, leaves, do, retain_graph=True), args.iters)
                note("torch sdpa fwd", t_sdpa)
                note("torch sdpa bwd", t_sb)
                print(f"{tag} torch sdpa fwd: {t_sdpa*1e6:8.1f} us  {f_fwd/t_sdpa/1e12:7.1f} TF/s"
                      f"  bwd: {t_sb*1e6:8.1f} us  {f_bwd/t_sb/1e12:7.1f} TF/s")
            except Exception as e:
                print("sdpa failed:", e)

    if args.rounds > 1:
        for name, ts in seen.items():
            print(f"{tag} {name}: range {min(ts)*1e6:.1f}-{max(ts)*1e6:.1f} us "
                  f"over {len(ts)} rounds")


if __name__ == "__main__":
    main()
