"""DiM throughput (bf16), separate from bench.py: train img/s and DDIM-50 img/s for both token mixers, and the
selective scan's time per launch with its algorithmic bytes against the 8 TB/s HBM rate of scripts/kernel_roofline.py.

    python scripts/bench_dim.py [--reps 5] [--quick] [--scan NAME] [--mixers mamba] [--no-big] [--orders]
                                [--out profiles/dim_bench.json]

--scan NAME: the Mamba cases are built with DiM(scan=NAME) (a pattern of models/dim.py: row, bidir, cross, zigzag).
--orders: also the per-launch times of the scan and the causal conv under the orders row (the plain entry points),
row_rev, col and snake_col (the _ord entry points), and the four index_select passes per block that a gather
formulation of an order would add (x and z rows forward, their gradients backward: [T, 2E] each way).

Shapes: 32x32 / H 384 / depth 12 / B 128 (the DiT-S/2 line's shape of bench.py); the reference's configs/cifar10_dim.py
(96x96, patch 2, H 384, depth 12, L = 2304) at its B = 8 and at the largest B of --big that fits.
Method: every (shape, mixer) is built once and warmed up, then the timed windows of all of them are interleaved,
--reps rounds; the median and the min / max over the rounds are reported. Windows are bracketed by HIP events.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from diffusion_models_collection_amd import kernels as K  # noqa: E402
from diffusion_models_collection_amd.diffusion import DDIM, DDPM  # noqa: E402
from diffusion_models_collection_amd.models import DiM  # noqa: E402
from diffusion_models_collection_amd.utils.trainer import DiffusionTrainer  # noqa: E402

DEV = "cuda"
HBM = 8e12


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e-3


class Case:
    def __init__(self, name, img, B, mixer, steps, scan="row"):
        self.name, self.B, self.mixer, self.steps = name, B, mixer, steps
        self.scan = scan if mixer == "mamba" else "row"
        mp = dict(img_size=(img, img), patch_size=2, in_channels=3, hidden_size=384, depth=12, state_size=16,
                  mlp_ratio=4.0, dropout=0.1, mixer=mixer)
        if self.scan != "row":
            mp["scan"] = self.scan
        torch.manual_seed(0)
        self.model = DiM(**mp, num_classes=10, compute_dtype="bf16").to(DEV)
        with torch.no_grad():       # off the zero adaLN init, so that no branch is multiplied by an exact zero
            for p in self.model.parameters():
                p.add_(0.02 * torch.randn_like(p))
        opt = torch.optim.AdamW(self.model.parameters(), lr=1e-4, weight_decay=1e-4)
        cfg = {"epochs": 1, "save_dir": "/tmp/dmc_dim_bench", "sample_dir": "/tmp/dmc_dim_bench", "loss_type": "l2",
               "use_ema": True, "ema_decay": 0.999, "conditional": True, "num_classes": 10, "cfg_dropout_prob": 0.2,
               "model_type": "dim", "model_params": mp}
        self.tr = DiffusionTrainer(self.model, DDPM(device=DEV), None, opt, None, device=DEV, config=cfg)
        self.x = (torch.rand(B, 3, img, img, device=DEV) * 2 - 1)
        self.y = torch.randint(0, 10, (B,), device=DEV)
        self.ddim = DDIM(1000, 50, device=DEV)
        self.shape = (B, 3, img, img)
        self.i = 0
        self.train_s, self.ddim_s = [], []

    def train_step(self):
        self.model.train()
        self.tr.train_step((self.x, self.y), self.i)
        self.i += 1

    def sample(self):
        self.model.eval()
        with torch.no_grad():
            self.ddim.sample(self.model, self.shape, y=self.y)

    def warm(self):
        for _ in range(3):
            self.train_step()
        self.sample()
        torch.cuda.synchronize()

    def measure(self):
        self.train_s.append(timed(self.train_step, self.steps))
        self.ddim_s.append(timed(self.sample, 1))

    def result(self):
        def line(ts, per):
            r = sorted(per / t for t in ts)
            return {"img_per_s": round(statistics.median(r), 1), "min": round(r[0], 1), "max": round(r[-1], 1)}
        return {"shape": self.name, "B": self.B, "mixer": self.mixer, "scan": self.scan,
                "train": line(self.train_s, self.B),
                "ddim50": line(self.ddim_s, self.B), "graphed_train": self.tr._graph is not None}


def scan_probe(B, L, E=768, N=16, reps=20):
    """µs per launch of dmc_selective_scan_fwd / bwd (bf16 rows, fp32 delta / Bm / Cm) and their algorithmic bytes.
    Forward: u, z, delta, Bm, Cm in, y out. Backward: those and dy in; du, dz, ddelta, dBm, dCm out."""
    dt = torch.bfloat16
    T = B * L
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    u, xz, dy = rn(T, E).to(dt), rn(T, 2 * E).to(dt), rn(T, E).to(dt)
    dpre, bc = rn(T, E), rn(T, 2 * N)
    A_log = torch.log(torch.arange(1, N + 1, device=DEV, dtype=torch.float32)).repeat(E, 1).contiguous()
    D, bias = torch.ones(E, device=DEV), torch.zeros(E, device=DEV)
    y = torch.empty(T, E, dtype=dt, device=DEV)
    states = K.scan_states(B, L, E, N, DEV)
    du, ddp, dxz, dbc = (torch.empty(T, c, dtype=dt, device=DEV) for c in (E, E, 2 * E, 2 * N))
    dA, dD = torch.empty(E, N, device=DEV), torch.empty(E, device=DEV)

    def fwd():
        K.selective_scan_fwd(dt, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, A_log, D, bias, B, L, E, N, states, y, E)

    def bwd():
        K.selective_scan_bwd(dt, dy, E, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, A_log, D, bias, B, L, E, N,
                             states, du, E, dxz, 2 * E, E, ddp, E, dbc, 2 * N, 0, dA, dD)

    fwd(); bwd()
    torch.cuda.synchronize()
    tf = sorted(timed(fwd, reps) for _ in range(3))[1]
    tb = sorted(timed(bwd, reps) for _ in range(3))[1]
    bytes_f = T * (E * (2 + 2 + 4 + 2) + 2 * N * 4)
    bytes_b = T * (E * (2 + 2 + 4 + 2) + 2 * N * 4 + E * (2 + 2 + 2) + 2 * N * 2)
    return {"B": B, "L": L, "E": E, "fwd_us": round(tf * 1e6, 1), "bwd_us": round(tb * 1e6, 1),
            "fwd_alg_bytes": bytes_f, "bwd_alg_bytes": bytes_b,
            "fwd_frac_of_hbm": round(bytes_f / tf / HBM, 3), "bwd_frac_of_hbm": round(bytes_b / tb / HBM, 3)}


ORDERS = ("row", "row_rev", "col", "snake_col")


def order_probe(B, h, w, E=768, N=16, reps=20):
    """µs per launch (bf16 rows) of the scan forward / backward and the causal conv forward / backward over B images
    of h x w tokens, per order: "row" through the plain entry points, the others through the _ord ones; and of the four
    index_select passes over [T, 2E] rows that gathering a block's tokens into walking order and back would add. The
    rounds of all orders are interleaved; median and min / max over 5 rounds."""
    from diffusion_models_collection_amd.models.dim import SCAN_ORDERS, scan_permutation
    dt = torch.bfloat16
    L = h * w
    T = B * L
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    u, xz, dy = rn(T, E).to(dt), rn(T, 2 * E).to(dt), rn(T, E).to(dt)
    dpre, bc = rn(T, E), rn(T, 2 * N)
    A_log = torch.log(torch.arange(1, N + 1, device=DEV, dtype=torch.float32)).repeat(E, 1).contiguous()
    D, bias = torch.ones(E, device=DEV), torch.zeros(E, device=DEV)
    cw, cb = 0.5 * rn(E, 1, 4), 0.1 * rn(E)
    y = torch.empty(T, E, dtype=dt, device=DEV)
    states = K.scan_states(B, L, E, N, DEV)
    du, ddp, dxz, dbc = (torch.empty(T, c, dtype=dt, device=DEV) for c in (E, E, 2 * E, 2 * N))
    dA, dD = torch.empty(E, N, device=DEV), torch.empty(E, device=DEV)
    dcw, dcb = torch.empty(E, 1, 4, device=DEV), torch.empty(E, device=DEV)

    def fns(name):
        code = SCAN_ORDERS.index(name)
        if code == 0:
            return {
                "scan_fwd": lambda: K.selective_scan_fwd(dt, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, A_log, D, bias,
                                                         B, L, E, N, states, y, E),
                "scan_bwd": lambda: K.selective_scan_bwd(dt, dy, E, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, A_log, D,
                                                         bias, B, L, E, N, states, du, E, dxz, 2 * E, E, ddp, E, dbc,
                                                         2 * N, 0, dA, dD),
                "conv_fwd": lambda: K.causal_conv_silu_fwd(dt, xz, 2 * E, cw, cb, B, L, E, y, E),
                "conv_bwd": lambda: K.causal_conv_silu_bwd(dt, dy, E, xz, 2 * E, cw, cb, B, L, E, dxz, 2 * E, dcw, dcb),
            }
        return {
            "scan_fwd": lambda: K.selective_scan_fwd_ord(dt, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, A_log, D, bias,
                                                         B, h, w, code, E, N, states, y, E),
            "scan_bwd": lambda: K.selective_scan_bwd_ord(dt, dy, E, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, A_log,
                                                         D, bias, B, h, w, code, E, N, states, du, E, dxz, 2 * E, E, ddp,
                                                         E, dbc, 2 * N, 0, dA, dD),
            "conv_fwd": lambda: K.causal_conv_silu_fwd_ord(dt, xz, 2 * E, cw, cb, B, h, w, code, E, y, E),
            "conv_bwd": lambda: K.causal_conv_silu_bwd_ord(dt, dy, E, xz, 2 * E, cw, cb, B, h, w, code, E, dxz, 2 * E,
                                                           dcw, dcb),
        }

    table = {name: fns(name) for name in ORDERS}
    perm = scan_permutation("snake_col", h, w).to(DEV)
    idx = (torch.arange(B, device=DEV)[:, None] * L + perm[None, :]).reshape(T)
    gathered = torch.empty_like(xz)

    def gather4():
        for _ in range(4):
            torch.index_select(xz, 0, idx, out=gathered)

    table["gather"] = {"index_select_x4": gather4}
    times = {name: {k: [] for k in f} for name, f in table.items()}
    for f in table.values():
        for fn in f.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(5):
        for name, f in table.items():
            for k, fn in f.items():
                times[name][k].append(timed(fn, reps) * 1e6)
    out = {"B": B, "h": h, "w": w, "L": L, "E": E}
    for name, f in times.items():
        out[name] = {k: {"us": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                     for k, v in f.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="2 rounds, no large-batch search")
    ap.add_argument("--big", type=int, nargs="*", default=[64, 32, 16], help="batch sizes tried at 96x96, largest first")
    ap.add_argument("--scan", default="row", help="scan pattern of the Mamba cases (models/dim.py)")
    ap.add_argument("--mixers", nargs="+", default=["mamba", "attention"], choices=["mamba", "attention"])
    ap.add_argument("--no-big", action="store_true", help="no large-batch search at 96x96")
    ap.add_argument("--orders", action="store_true", help="per-launch times of the scan and conv per order, and of the "
                                                          "gathers an order would cost without the in-kernel walk")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = 2 if args.quick else args.reps
    specs = [("32x32_B128", 32, 128, 10), ("96x96_B8", 96, 8, 5)]
    cases, big = [], None
    for name, img, B, steps in specs:
        for mixer in args.mixers:
            c = Case(name, img, B, mixer, steps, args.scan)
            c.warm()
            cases.append(c)
    if not args.quick and not args.no_big:
        for B in args.big:          # the largest batch at which both mixers train and sample
            try:
                cs = [Case(f"96x96_B{B}", 96, B, mixer, 3, args.scan) for mixer in args.mixers]
                for c in cs:
                    c.warm()
                cases += cs
                big = B
                break
            except torch.cuda.OutOfMemoryError:
                cs = None
                torch.cuda.empty_cache()
    for _ in range(reps):
        for c in cases:
            c.measure()
    scans = [scan_probe(128, 256), scan_probe(8, 2304)] + ([scan_probe(big, 2304)] if big else [])
    out = {"bench": "dim", "dtype": "bf16", "reps": reps, "device": torch.cuda.get_device_name(0),
           "lines": [c.result() for c in cases], "scan": scans, "largest_B_96x96": big}
    if args.orders:
        out["orders"] = [order_probe(128, 16, 16), order_probe(8, 48, 48)]
    print(json.dumps(out))
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
