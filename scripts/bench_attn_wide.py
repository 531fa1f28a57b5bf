"""Time the attention kernels at head dims above 64 beside the two things a user would otherwise run.

    python scripts/bench_attn_wide.py [--json FILE]

Shapes (N, heads, L, hd): the wide UNet's 16x16 and 8x8 levels (128, 4, 256 / 64, 128) and DiT-XL/2 at 32x32
(128, 16, 256, 72). Per shape, in one process on one GPU, alternating over ROUNDS rounds:
  * dmc bf16 / dmc fp32: dmc_attn_fwd, and dmc_attn_bwd (its two kernels, dQ then dK/dV, back to back);
  * eager fp32: q @ k.T / sqrt(hd), softmax, @ v in torch, and its autograd backward;
  * sdpa bf16: torch.nn.functional.scaled_dot_product_attention and its autograd backward.
Times are HIP-event windows of at least WINDOW seconds after a warm-up of every variant; the printed figure is the
median of the rounds with their min..max beside it. The split of the backward into its dQ and dK/dV kernels comes from
a kernel trace of this script, one shape per run so that the kernel names tell the rest
(rocprofv3 --kernel-trace --stats -- python scripts/bench_attn_wide.py --rounds 1 --shape 0): the two are one ABI
call. No GPU, no number: the script fails without one.
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

SHAPES = [(128, 4, 256, 128), (128, 4, 64, 128), (128, 16, 256, 72)]
WINDOW = 0.1


def window(fn, iters):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def variants(N, heads, L, hd):
    """name -> (forward fn, backward fn)"""
    from diffusion_models_collection_amd import kernels as K
    dev, C = "cuda", heads * hd
    g = torch.Generator().manual_seed(L + hd)
    qkv32 = torch.randn(N, L, 3 * C, generator=g)
    do32 = torch.randn(N, L, C, generator=g)
    out = {}
    for name, dt in (("dmc bf16", torch.bfloat16), ("dmc fp32", torch.float32)):
        qkv, do = qkv32.to(dt).to(dev), do32.to(dt).to(dev)
        od = torch.empty(N, L, C, dtype=dt, device=dev)
        lse = torch.empty(N * heads * L, device=dev)
        dq = torch.empty_like(qkv)

        def fwd(dt=dt, qkv=qkv, od=od, lse=lse):
            K.attn_fwd(dt, qkv, 3 * C, N, L, heads, hd, od, C, lse)

        def bwd(dt=dt, qkv=qkv, od=od, do=do, lse=lse, dq=dq):
            K.attn_bwd(dt, qkv, 3 * C, od, do, C, lse, N, L, heads, hd, dq, 3 * C)

        out[name] = (fwd, bwd)
    split = qkv32.view(N, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    dos = do32.view(N, L, heads, hd).permute(0, 2, 1, 3)
    for name, dt in (("eager fp32", torch.float32), ("sdpa bf16", torch.bfloat16)):
        q, k, v = (split[i].to(dt).to(dev).contiguous().requires_grad_(True) for i in range(3))
        do = dos.to(dt).to(dev).contiguous()
        if name.startswith("eager"):
            def f(q=q, k=k, v=v):
                return torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1) @ v
        else:
            def f(q=q, k=k, v=v):
                return torch.nn.functional.scaled_dot_product_attention(q, k, v)
        o = f()

        def bwd(o=o, q=q, k=k, v=v, do=do):
            torch.autograd.grad(o, (q, k, v), do, retain_graph=True)

        def fwd(f=f):
            with torch.no_grad():
                f()

        out[name] = (fwd, bwd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: only this shape")
    ap.add_argument("--json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attn_wide: needs a GPU")
    rows = []
    for (N, heads, L, hd) in (SHAPES if a.shape is None else [SHAPES[a.shape]]):
        var = variants(N, heads, L, hd)
        fns = {(name, part): fn for name, (f, b) in var.items() for part, fn in (("fwd", f), ("bwd", b))}
        iters = {}
        for key, fn in fns.items():   # warm-up of every variant, and the iteration count of its window
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[key] = max(10, int(WINDOW / max(window(fn, 10), 1e-7)))
        times = {key: [] for key in fns}
        for _ in range(a.rounds):
            for key, fn in fns.items():
                times[key].append(window(fn, iters[key]))
        for (name, part), ts in times.items():
            row = dict(N=N, heads=heads, L=L, hd=hd, variant=name, part=part, median_us=statistics.median(ts) * 1e6,
                       min_us=min(ts) * 1e6, max_us=max(ts) * 1e6, rounds=a.rounds, iters=iters[(name, part)])
            rows.append(row)
            print(f"N{N} h{heads} L{L} hd{hd} {name:10s} {part}: {row['median_us']:9.1f} us "
                  f"({row['min_us']:.1f} .. {row['max_us']:.1f}, {a.rounds} x {row['iters']} calls)", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
