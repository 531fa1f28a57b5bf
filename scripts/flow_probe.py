"""The rectified-flow kernels' time per launch beside the same update written as torch ops, and ms per image of
RectifiedFlow.sample (Euler-20, Heun-10) beside DDIM-20 and DPMSolver-20 on the CIFAR UNet and DiT-S/2 (bf16, B = 16).

Kernel legs, at (N, C, H, W) = (128, 3, 32, 32) and (64, 3, 64, 64): dmc_flow_step for each row kind (Euler, Heun
predictor, Heun corrector), with and without the in-kernel guidance (cfg_scale 3, the two halves of one 2N-row buffer read
in place), and dmc_flow_guide (guidance_rescale 0.7, p_threshold 0.995; a shape above its 16384 elements per sample would
be skipped). Each leg is 100 back-to-back repetitions captured in one HIP graph (the host's enqueue stays
out of the figure), timed by device events around a replay; the legs' replays are interleaved and the figure is the median
of --reps (>= 20) replays after warm-up:
  kernel        one launch
  torch graph   the same update as torch ops, captured the same way: the yardstick, device time against device time
  torch eager   the same torch ops NOT in a graph, 100 eager repetitions between two device events, host enqueue
                included, as a user without the kernel runs them outside a captured step
Sampler legs: whole sample() calls (the replayed step graph at B = 16), host clock around a synchronised call,
interleaved, median of --reps.

    python scripts/flow_probe.py [--reps 20] [--out profiles/flow_probe.txt] [--no-models]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from bench import CIFAR, DIT_S2  # noqa: E402

INNER = 100
KINDS = ("euler", "predictor", "corrector")


def torch_step(kind, x, pc, pu, scale, xb, d, h, hh):
    """(out, xb_out, d_out) of one row as torch ops; h, hh: [N, 1, 1, 1] tensors, as a per-sample table gather gives."""
    g = pc if pu is None else pu + scale * (pc - pu)
    if kind == "corrector":
        return xb + hh * (d + g), None, None
    out = x + h * g
    if kind == "predictor":
        return out, x.clone(), g.clone() if pu is None else g
    return out, None, None


def torch_guide(x, pc, pu, scale, phi, sigma, p):
    g = pu + scale * (pc - pu)
    f = phi * (pc.flatten(1).std(1) / g.flatten(1).std(1)) + (1 - phi)
    g = g * f.view(-1, 1, 1, 1)
    x0 = x - sigma * g
    s = torch.quantile(x0.flatten(1).abs(), p, dim=1).clamp(min=1.0).view(-1, 1, 1, 1)
    return (x - torch.clamp(x0, -s, s) / s) / sigma


def graphed(fn):
    """fn repeated INNER times in one graph -> a callable returning one replay's device time in us per repetition."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(INNER):
            fn()
    g.replay()
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / INNER
    return once


def eager(fn):
    """fn repeated INNER times eagerly -> a callable returning the device time in us per repetition."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / INNER
    return once


def medians(legs, reps):
    els = {k: [] for k in legs}
    for _ in range(reps):
        for k, once in legs.items():
            els[k].append(once())
    return {k: statistics.median(v) for k, v in els.items()}, {k: min(v) for k, v in els.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "flow_probe.txt"))
    ap.add_argument("--no-models", action="store_true", help="kernel legs only")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    from diffusion_models_collection_amd import kernels as K
    from diffusion_models_collection_amd.diffusion import DDIM, DPMSolver, RectifiedFlow
    from diffusion_models_collection_amd.models import DiT, UNet
    if not torch.cuda.is_available():
        raise SystemExit("flow_probe: no GPU (a timing needs the device)")
    torch.manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    heun = RectifiedFlow(1000, 10, solver="heun", device="cuda")
    coef = heun.step_coefficients
    row = {"predictor": 4, "corrector": 5, "euler": 18}
    say(f"rectified-flow probe: {torch.cuda.get_device_name(0)}, {INNER} launches per graph replay, median of {a.reps} "
        "replays, us per launch")
    for shape in ((128, 3, 32, 32), (64, 3, 64, 64)):
        N = shape[0]
        x, xb, d = (torch.randn(shape, device="cuda") for _ in range(3))
        both = torch.randn((2 * N,) + shape[1:], device="cuda")
        out, xbo, do = (torch.empty_like(x) for _ in range(3))
        for kind in KINDS:
            k = torch.full((N,), row[kind], dtype=torch.long, device="cuda")
            h, hh = coef[k][:, 1].view(-1, 1, 1, 1), coef[k][:, 2].view(-1, 1, 1, 1)
            for guided in (False, True):
                pc, pu = (both[:N], both[N:]) if guided else (both[:N], None)
                legs = {"kernel": graphed(lambda: K.flow_step(x, pc, k, coef, pu=pu, scale=3.0, xb=xb, dprev=d, out=out,
                                                              xb_out=xbo, d_out=do)),
                        "torch graph": graphed(lambda: torch_step(kind, x, pc, pu, 3.0, xb, d, h, hh)),
                        "torch eager": eager(lambda: torch_step(kind, x, pc, pu, 3.0, xb, d, h, hh))}
                med, low = medians(legs, a.reps)
                say(f"flow_step {tuple(shape)} {kind:9s} guidance {'in kernel' if guided else 'none     '}: kernel "
                    f"{med['kernel']:7.2f}  torch graph {med['torch graph']:7.2f}  torch eager {med['torch eager']:7.2f}"
                    f"   kernel/torch graph {med['kernel'] / med['torch graph']:.3f}   (min {low['kernel']:.2f}, "
                    f"{low['torch graph']:.2f}, {low['torch eager']:.2f})")
        if shape[1] * shape[2] * shape[3] <= 16384:
            k = torch.full((N,), row["predictor"], dtype=torch.long, device="cuda")
            sigma = coef[k][:, 0].view(-1, 1, 1, 1)
            legs = {"kernel": graphed(lambda: K.flow_guide(x, both[:N], both[N:], 3.0, 0.7, k, coef, threshold=True,
                                                           p_threshold=0.995, out=out)),
                    "torch graph": graphed(lambda: torch_guide(x, both[:N], both[N:], 3.0, 0.7, sigma, 0.995)),
                    "torch eager": eager(lambda: torch_guide(x, both[:N], both[N:], 3.0, 0.7, sigma, 0.995))}
            med, low = medians(legs, a.reps)
            say(f"flow_guide {tuple(shape)} rescale 0.7, p 0.995: kernel {med['kernel']:7.2f}  torch graph "
                f"{med['torch graph']:7.2f}  torch eager {med['torch eager']:7.2f}   kernel/torch graph "
                f"{med['kernel'] / med['torch graph']:.3f}   (min {low['kernel']:.2f}, {low['torch graph']:.2f}, "
                f"{low['torch eager']:.2f})")

    if not a.no_models:
        B = 16
        shape = (B, 3, 32, 32)
        samplers = {"Euler-20": RectifiedFlow(1000, 20, solver="euler", device="cuda"), "Heun-10": heun,
                    "DDIM-20": DDIM(1000, 20, device="cuda"), "DPMSolver-20": DPMSolver(1000, 20, device="cuda")}
        evals = {"Euler-20": 20, "Heun-10": 19, "DDIM-20": 20, "DPMSolver-20": len(samplers["DPMSolver-20"].inference_timesteps)}
        models = {"CIFAR UNet": UNet(**CIFAR, compute_dtype="bf16").cuda().eval(),
                  "DiT-S/2": DiT(**DIT_S2, num_classes=None, dropout=0.0, compute_dtype="bf16").cuda().eval()}
        for mname, m in models.items():
            with torch.no_grad():
                for smp in samplers.values():       # warm-up: code objects, weight packs, the kept step graphs
                    smp.sample(m, shape)
                    smp.sample(m, shape)
                els = {k: [] for k in samplers}
                for _ in range(a.reps):
                    for k, smp in samplers.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        smp.sample(m, shape)
                        torch.cuda.synchronize()
                        els[k].append((time.perf_counter() - t0) * 1e3)
            say(f"sample, {mname} bf16, B={B}, replayed step graph, median of {a.reps}: " + "  ".join(
                f"{k} ({evals[k]} evaluations) {statistics.median(v) / B:6.3f} ms/image (call {statistics.median(v):7.2f} "
                f"ms, min {min(v):.2f})" for k, v in els.items()))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
