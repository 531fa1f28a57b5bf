"""DPM-Solver++ (20 log-SNR steps) against DDIM-50 on the CIFAR UNet (bf16): ms per call, img/s and ms per model
evaluation, three timed calls each per batch size, in one process.

    python scripts/dpm_probe.py [--batches 16,128] [--warmup 1] [--fixed-cost]

Per-step claim: the DPM-Solver++ step costs what the DDIM step costs (its kernel moves 5 tensors where DDIM's moves 3,
against a forward of a few ms); the margin is the spread of DDIM's own three calls. User-facing claim: img/s.
--fixed-cost instead times both samplers at 20 and 50 requested steps and splits the best call time into a marginal
cost per evaluation and a fixed cost per call (ms per step above is call time / evaluations, so it carries the fixed
cost divided by 20 for one sampler and by 50 for the other).
"""
import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from bench import CIFAR  # noqa: E402


def timed(sampler, model, shape, calls, warmup):
    with torch.no_grad():
        for _ in range(warmup):
            sampler.sample(model, shape)
        els = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sampler.sample(model, shape)
            torch.cuda.synchronize()
            els.append(time.perf_counter() - t0)
    return els


def fixed_cost(model, batches, warmup):
    from diffusion_models_collection_amd.diffusion import DDIM, DPMSolver
    for B in batches:
        for name, cls in (("DDIM", DDIM), ("DPMSolver", DPMSolver)):
            pts = []
            for steps in (20, 50):
                smp = cls(1000, steps, device="cuda")
                evals = len(smp.inference_timesteps)
                els = timed(smp, model, (B, 3, 32, 32), 3, warmup)
                pts.append((evals, min(els) * 1e3))
                print(f"B={B:4d} {name:9s} evals {evals:3d}  ms/call " + " ".join(f"{e * 1e3:7.2f}" for e in els),
                      flush=True)
            (n0, t0), (n1, t1) = pts
            slope = (t1 - t0) / (n1 - n0)
            print(f"B={B:4d} {name:9s} marginal {slope:.4f} ms per evaluation, fixed {t0 - slope * n0:.3f} ms per call",
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,128")
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls before the three timed ones (graph capture)")
    ap.add_argument("--fixed-cost", action="store_true", help="marginal ms per evaluation and fixed ms per call")
    a = ap.parse_args()
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.diffusion import DDIM, DPMSolver
    torch.manual_seed(0)
    m = UNet(**CIFAR, compute_dtype="bf16").cuda().eval()
    if a.fixed_cost:
        fixed_cost(m, [int(b) for b in a.batches.split(",")], a.warmup)
        return
    samplers = [("DDIM-50", DDIM(1000, 50, device="cuda")), ("DPMSolver-20", DPMSolver(1000, 20, device="cuda"))]
    for B in [int(b) for b in a.batches.split(",")]:
        rows = {}
        for name, smp in samplers:
            evals = len(smp.inference_timesteps)
            els = timed(smp, m, (B, 3, 32, 32), 3, a.warmup)
            per_step = [e * 1e3 / evals for e in els]
            rows[name] = (els, per_step)
            print(f"B={B:4d} {name:13s} evals {evals:3d}  ms/call " + " ".join(f"{e * 1e3:7.1f}" for e in els)
                  + "  ms/step " + " ".join(f"{p:6.3f}" for p in per_step)
                  + f"  img/s (best) {B / min(els):8.1f}", flush=True)
        d, p = rows["DDIM-50"], rows["DPMSolver-20"]
        spread = max(d[1]) - min(d[1])
        print(f"B={B:4d} per step: DDIM {min(d[1]):.3f} ms (spread of its three calls {spread:.3f} ms), DPMSolver "
              f"{min(p[1]):.3f} ms, difference {min(p[1]) - min(d[1]):+.3f} ms;  img/s ratio DPMSolver-20 / DDIM-50 "
              f"{min(d[0]) / min(p[0]):.2f}x", flush=True)


if __name__ == "__main__":
    main()
