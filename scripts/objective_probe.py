"""The training objective's cost in the graphed train step: CIFAR UNet, bf16, B = 128, ms per step with the default
objective (eps target, unweighted: dmc_loss_fwd + dmc_loss_bwd), with prediction_type='v', and with 'v' plus
snr_gamma=5 (both: one dmc_objective call). One process; every arm runs one untimed leg (warm-up steps, capture, first
replays), then the arms take turns for three timed legs each, so drift of the machine hits every arm alike.

    python scripts/objective_probe.py [--batch 128] [--steps 100] [--legs 3] [--arms default,v,v_gamma]

Byte count: the objective reads pred, x0 and noise and writes dpred once, four passes of B*3*32*32*4 = 1.5 MB, a few
microseconds of a step of about 11 ms; a non-default arm that sits above the default one by more than three times the
default arm's own spread needs an explanation. `--arms default` touches nothing this objective added, so the same file
also times an older tree (run it from that tree's scripts/).
"""
import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from bench import CIFAR, make_trainer  # noqa: E402

ARMS = {"default": {}, "v": {"prediction_type": "v"}, "v_gamma": {"prediction_type": "v", "snr_gamma": 5.0}}


def make_arm(name, batch):
    model, tr = make_trainer(CIFAR, "bf16", "cuda", 0, 1)
    extra = ARMS[name]
    if extra:      # what DiffusionTrainer does with these config keys (make_trainer builds its own config)
        tr.diffusion.set_prediction_type(extra["prediction_type"])
        tr.snr_gamma = extra.get("snr_gamma")
    model.train()
    gen = torch.Generator().manual_seed(7)
    pool = [(torch.rand(batch, 3, 32, 32, generator=gen) * 2 - 1).cuda() for _ in range(4)]
    return tr, pool


def leg(tr, pool, steps):
    torch.cuda.synchronize()
    r0 = tr._graph.replays if tr._graph is not None else 0
    t0 = time.perf_counter()
    for i in range(steps):
        loss = tr.train_step(pool[i % len(pool)], 0)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    graphed = tr._graph is not None and tr._graph.replays - r0 == steps
    return el * 1e3 / steps, graphed, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100, help="train steps per leg")
    ap.add_argument("--legs", type=int, default=3, help="timed legs per arm")
    ap.add_argument("--arms", default="default,v,v_gamma")
    a = ap.parse_args()
    names = a.arms.split(",")
    arms = {n: make_arm(n, a.batch) for n in names}
    for n, (tr, pool) in arms.items():
        ms, graphed, loss = leg(tr, pool, a.steps)       # untimed: eager warm-up, capture, first replays
        print(f"{n:8s} untimed leg {ms:7.3f} ms/step  loss {loss:.4f}", flush=True)
    res = {n: [] for n in names}
    for k in range(a.legs):
        for n, (tr, pool) in arms.items():
            ms, graphed, loss = leg(tr, pool, a.steps)
            assert graphed, f"{n}: a timed step was not a graph replay"
            res[n].append(ms)
    for n in names:
        v = res[n]
        print(f"{n:8s} ms/step " + " ".join(f"{x:7.3f}" for x in v)
              + f"   best {min(v):7.3f}  spread {max(v) - min(v):.3f}", flush=True)
    if "default" in res:
        d = res["default"]
        spread = max(d) - min(d)
        for n in names:
            if n != "default":
                diff = min(res[n]) - min(d)
                ratio = f"{diff / spread:+.1f} x" if spread > 0 else "no multiple of"     # one leg has no spread
                print(f"{n:8s} - default: {diff:+.3f} ms/step ({ratio} the default arm's spread of {spread:.3f} ms)",
                      flush=True)


if __name__ == "__main__":
    main()
