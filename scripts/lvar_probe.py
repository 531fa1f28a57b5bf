"""The learned-variance kernels' cost beside the kernels they stand next to, at the CIFAR training shape. Two figures per
arm, the arms taking turns for `--legs` legs so that drift of the machine hits every arm alike (after a warm-up of all):
  graph  `--iters` calls captured in one graph, device events around a replay: the host's enqueue is out of the figure,
         and the achieved bytes per second are the bytes the call must move (computed here from the shapes) over it
  eager  device events around `--iters` back-to-back calls through the Python wrappers: the larger of the device time and
         the host's enqueue, which is what an uncaptured loop pays

    python scripts/lvar_probe.py [--batch 128] [--iters 200] [--legs 5]

Arms and the bytes they must move (fp32, n = B*3*32*32 elements):
  hybrid            dmc_hybrid_objective on [B, 6, 32, 32]: reads out (2n) and noise (n), writes dout (2n)      5n * 4
                    (x0 is read for the t = 0 samples only with an eps target; the timesteps here are uniform)
  objective         dmc_objective on [B, 3, 32, 32]: reads pred and noise, writes dpred                         3n * 4
  torch             the unfused torch composition of the hybrid loss and its gradient (autograd), same inputs
  step_learned      dmc_ddpm_step_learned: reads x, eps, v (in place), z, writes out                            5n * 4
  step              dmc_ddpm_step: reads x, eps, z, writes out                                                  4n * 4
  vlb_learned       dmc_vlb_step_learned with x_next: reads x0, x_t, pred, v, z_next, writes x_next             6n * 4
  vlb               dmc_vlb_step with x_next: reads x0, x_t, pred, z_next, writes x_next                        5n * 4
At this size (1.5 MB per [B, 3, 32, 32] tensor) every operand stays in the last-level cache between launches, so the
rates say how far a launch is from its latency floor, not from HBM.
"""
import argparse
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from diffusion_models_collection_amd import kernels as K  # noqa: E402
from diffusion_models_collection_amd.diffusion import DDPM  # noqa: E402

LN2 = math.log(2.0)


def torch_hybrid(out, x0, noise, t, coef, vlb_weight):
    """The same loss from torch ops (eps target, l2), gradient by autograd: what the fused kernel replaces."""
    C = x0.shape[1]
    o = out.detach().requires_grad_(True)
    pred, v = o[:, :C], o[:, C:]
    simple = ((noise - pred) ** 2).flatten(1).mean(1).mean()
    row = coef[t].view(-1, coef.shape[1], 1, 1, 1)
    cp, lvmin, R, kmin = row[:, 1], row[:, 3], row[:, 4], row[:, 5]
    delta = cp * (pred.detach() - noise)
    d = (v + 1) * 0.5 * R
    kl = 0.5 * (d + torch.expm1(-d)) + kmin * torch.exp(-d) * delta * delta
    isig = torch.exp(-0.5 * (lvmin + d))
    zp, zm = (delta + 1 / 255) * isig, (delta - 1 / 255) * isig
    cdf = lambda z: 0.5 * torch.special.erfc(-z / math.sqrt(2.0))   # noqa: E731
    left = zm <= 0
    pr = torch.where(x0 < -0.999, cdf(zp), torch.where(x0 > 0.999, cdf(-zm),
                     cdf(torch.where(left, zp, -zm)) - cdf(torch.where(left, zm, -zp))))
    term = torch.where((t == 0).view(-1, 1, 1, 1), -pr.clamp_min(1e-12).log(), kl)
    total = simple + vlb_weight * (term.flatten(1).mean(1) / LN2).mean()
    total.backward()
    return total.detach(), o.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200, help="launches per timed leg")
    ap.add_argument("--legs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lvar_probe: no GPU; a time measured elsewhere says nothing")
    dev = torch.device("cuda")
    B, C = a.batch, 3
    g = torch.Generator().manual_seed(7)
    x0 = ((torch.randint(0, 256, (B, C, 32, 32), generator=g).float() / 127.5) - 1).to(dev)
    noise, z = (torch.randn(B, C, 32, 32, generator=g).to(dev) for _ in range(2))
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    out = torch.cat([noise + 0.1 * torch.randn_like(noise), torch.rand_like(noise) * 2 - 1], 1).contiguous()
    pred = out[:, :C].contiguous()
    smp = DDPM(device="cuda", variance_type="learned_range")
    sa, s1 = smp.sqrt_alphas_cumprod, smp.sqrt_one_minus_alphas_cumprod
    coef = smp._lvar_table(dev)
    fixed = smp._vlb_table("fixed_small", dev)
    tabs = [smp._tab(k, dev) for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                       "posterior_mean_coef2")]
    lv = smp.posterior_log_variance_clipped
    x_t = smp.q_sample(x0, t, noise)
    tn = (t - 1).contiguous()
    one = torch.ones((), device=dev)
    dout, dpred, res, xn = torch.empty_like(out), torch.empty_like(pred), torch.empty_like(x0), torch.empty_like(x0)
    rows = tuple(torch.empty(B, device=dev) for _ in range(4))
    n = x0.numel()
    arms = {
        "hybrid": (5 * n * 4, lambda: K.hybrid_objective("eps", "l2", out, x0, noise, t, sa, s1, coef, vlb_weight=0.001,
                                                          dloss=one, dout=dout)),
        "objective": (3 * n * 4, lambda: K.objective("eps", "l2", pred, x0, noise, t, sa, s1, dloss=one, out=dpred)),
        "torch": (None, lambda: torch_hybrid(out, x0, noise, t, coef, 0.001)),
        "step_learned": (5 * n * 4, lambda: K.ddpm_step_learned(x_t, out, t, *tabs, coef, z=z, res=res)),
        "step": (4 * n * 4, lambda: K.ddpm_step(x_t, pred, t, *tabs, lv, z=z, out=res)),
        "vlb_learned": (6 * n * 4, lambda: K.vlb_step_learned(x0, x_t, out, t, coef, z_next=z, t_next=tn, sa=sa, s1=s1,
                                                              x_next=xn, rows=rows)),
        "vlb": (5 * n * 4, lambda: K.vlb_step(x0, x_t, pred, t, fixed, z_next=z, t_next=tn, sa=sa, s1=s1, x_next=xn,
                                              out=rows)),
    }
    l_k, _ = K.hybrid_objective("eps", "l2", out, x0, noise, t, sa, s1, coef, vlb_weight=0.001, dloss=one, dout=dout)
    l_t, g_t = torch_hybrid(out, x0, noise, t, coef, 0.001)
    print(f"loss kernel {float(l_k[0]):.7f} torch {float(l_t):.7f}; gradient max abs diff "
          f"{float((dout - g_t).abs().max()):.3e} of {float(g_t.abs().max()):.3e}", flush=True)
    for fn in (f for _, f in arms.values()):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    graphs = {}
    for k, (nbytes, fn) in arms.items():
        if nbytes is None:
            continue        # the autograd composition allocates its graph anew per call: eager only
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(a.iters):
                fn()
        graphs[k].replay()
    torch.cuda.synchronize()

    def timed(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    def eager(fn):
        for _ in range(a.iters):
            fn()

    us, ug = {k: [] for k in arms}, {k: [] for k in graphs}
    for _ in range(a.legs):
        for k, (_, fn) in arms.items():
            us[k].append(timed(lambda: eager(fn)))
            if k in graphs:
                ug[k].append(timed(graphs[k].replay))
    for k, (nbytes, _) in arms.items():
        for tag, v in (("graph", ug.get(k)), ("eager", us[k])):
            if not v:
                continue
            rate = (f"  {nbytes / (min(v) * 1e-6) / 1e12:6.3f} TB/s over {nbytes / 1e6:.2f} MB" if tag == "graph" else "")
            print(f"{k:13s} {tag} us/call " + " ".join(f"{x:7.2f}" for x in v) + f"   best {min(v):7.2f}  spread "
                  f"{max(v) - min(v):.2f}{rate}", flush=True)


if __name__ == "__main__":
    main()
