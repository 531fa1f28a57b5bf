"""dmc_cfg_guide's time per launch beside the launches it replaces and beside eager torch ops, and DDIM-50
sample_with_cfg on the CIFAR UNet (bf16, B = 16) with guidance_rescale 0.7 against 0.

Kernel legs, at (N, per) = (16, 3072) and (128, 3072), 'v' prediction, cfg_scale 3, p_threshold 0.995, guidance_rescale
0 and 0.7. Each leg is 100 back-to-back repetitions captured in one HIP graph (the host's enqueue stays out of the figure),
timed by device events around a replay; the legs' replays are interleaved, and the figure is the median of --reps (>= 20)
replays after warm-up:
  guide    one dmc_cfg_guide launch
  pair     dmc_pred_convert (both halves, eps only) + dmc_cfg_x0 mode 0: what dmc_cfg_guide replaces at rescale 0 (the
           pair has no rescale; it stands beside the 0.7 row for scale only)
  torch    the same arithmetic as eager torch ops (guidance, std ratio, conversion, quantile, clamp), NOT in a graph:
           100 eager repetitions between two device events, host enqueue included, as a user without the kernel runs it
Sampler legs: whole DDIM-50 calls (the replayed step graph at B = 16), host clock around a synchronised call, interleaved.

    python scripts/cfg_guide_probe.py [--reps 20] [--out profiles/cfg_guide_probe.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from bench import CIFAR  # noqa: E402

INNER = 100


def torch_guide(x, pc, pu, scale, phi, sa, s1, p):
    g = pu + scale * (pc - pu)
    if phi > 0:
        f = phi * (pc.flatten(1).std(1) / g.flatten(1).std(1)) + (1 - phi)
        g = g * f.view(-1, 1, 1, 1)
    eps = s1 * x + sa * g
    x0 = sa * x - s1 * g
    s = torch.quantile(x0.flatten(1).abs(), p, dim=1).clamp(min=1.0).view(-1, 1, 1, 1)
    return eps, torch.clamp(x0, -s, s) / s


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cfg_guide_probe.txt"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    from diffusion_models_collection_amd import kernels as K
    from diffusion_models_collection_amd.diffusion import DDIM
    from diffusion_models_collection_amd.models import UNet
    if not torch.cuda.is_available():
        raise SystemExit("cfg_guide_probe: no GPU (a timing needs the device)")
    torch.manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ddim = DDIM(1000, 50, device="cuda", prediction_type="v")
    sa, s1, ac = ddim.sqrt_alphas_cumprod, ddim.sqrt_one_minus_alphas_cumprod, ddim.alphas_cumprod
    say(f"dmc_cfg_guide probe: {torch.cuda.get_device_name(0)}, {INNER} launches per graph replay, median of {a.reps} "
        "replays, us per launch")
    for N in (16, 128):
        shape = (N, 3, 32, 32)
        x = torch.randn(shape, device="cuda")
        both = torch.randn((2 * N,) + shape[1:], device="cuda")
        t = torch.randint(0, 1000, (N,), device="cuda")
        sat, s1t = sa[t].view(-1, 1, 1, 1), s1[t].view(-1, 1, 1, 1)
        eo, xo = torch.empty_like(x), torch.empty_like(x)
        conv = torch.empty_like(both)

        def pair():
            K.pred_convert("v", x, t, sa, s1, both, want_x0=False, out=(conv, None))
            K.cfg_x0(x, conv[:N], conv[N:], 3.0, t, ac, None, 0, 0.995, out=(eo, xo))

        for phi in (0.0, 0.7):
            legs = {"guide": graphed(lambda: K.cfg_guide("v", x, both[:N], both[N:], 3.0, phi, t, sa, s1, 0.995,
                                                        out=(eo, xo))),
                    "pair": graphed(pair),
                    "torch": eager(lambda: torch_guide(x, both[:N], both[N:], 3.0, phi, sat, s1t, 0.995))}
            els = {k: [] for k in legs}
            for _ in range(a.reps):
                for k, once in legs.items():
                    els[k].append(once())
            med = {k: statistics.median(v) for k, v in els.items()}
            say(f"N={N:4d} per=3072 rescale={phi}: guide {med['guide']:8.2f}  pred_convert+cfg_x0 {med['pair']:8.2f}  "
                f"torch ops (eager) {med['torch']:8.2f}   guide/pair {med['guide'] / med['pair']:.3f}  "
                f"guide/torch {med['guide'] / med['torch']:.3f}   (min guide {min(els['guide']):.2f}, "
                f"pair {min(els['pair']):.2f}, torch {min(els['torch']):.2f})")

    m = UNet(**CIFAR, compute_dtype="bf16").cuda().eval()
    B = 16
    shape = (B, 3, 32, 32)
    y = torch.randint(1, 10, (B,), device="cuda")
    legs = {"rescale 0": lambda: ddim.sample_with_cfg(m, shape, y, guidance_rescale=0.0),
            "rescale 0.7": lambda: ddim.sample_with_cfg(m, shape, y, guidance_rescale=0.7)}
    with torch.no_grad():
        for fn in legs.values():          # warm-up: code objects, weight packs, the kept step graphs
            fn()
            fn()
        els = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                els[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in els.items()}
    say(f"DDIM-50 sample_with_cfg, CIFAR UNet bf16, B={B}, 'v', replayed step graph, ms per call, median of {a.reps}: "
        + "  ".join(f"{k} {v:7.2f} (min {min(els[k]):.2f}, max {max(els[k]):.2f})" for k, v in med.items())
        + f"   0.7 / 0 = {med['rescale 0.7'] / med['rescale 0']:.4f}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
