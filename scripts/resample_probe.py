"""Time per call of the loss-aware timestep sampling kernels, and of dmc_objective_is / dmc_hybrid_objective_is against
dmc_objective / dmc_hybrid_objective of this build and (--prev) of another build of libdmc.so, e.g. the previous commit's
(scripts/build_prev.sh), on the same inputs in the same process.

Every arm is 200 calls (loss and gradient in one pass: the main kernel plus its final kernel) captured in one graph
between two device events, so the host's enqueue is out of the figure. The arms are replayed in interleaved rounds
(A, B, C, ..., A, B, C, ...) so drift hits all alike; per arm the rounds' figures, their minimum and their spread
(max - min) are printed. The libraries are loaded with ctypes directly: a build without the new symbols still serves
its dmc_objective.

    python scripts/resample_probe.py [--prev diffusion_models_collection_amd/libdmc_prev.so] [--rounds 7]
"""
import argparse
import ctypes
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
CALLS = 200
P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def load(path):
    lib = ctypes.CDLL(str(path))
    protos = {"dmc_objective": [I, I] + [P] * 7 + [I, I, I] + [P] * 5,
              "dmc_objective_is": [I, I] + [P] * 8 + [I, I, I] + [P] * 6,
              "dmc_hybrid_objective": [I, I] + [P] * 8 + [I, I, I, F] + [P] * 5,
              "dmc_hybrid_objective_is": [I, I] + [P] * 9 + [I, I, I, F] + [P] * 6,
              "dmc_ts_history_update": [P, P, I, I, I, P, P, P],
              "dmc_ts_sample": [P, P, I, I, F, P, I, P, P, P, P, P]}
    for name, args in protos.items():
        if hasattr(lib, name):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = I
    return lib


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def graph_of(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from diffusion_models_collection_amd.diffusion import DDPM, _vlb
    new = load(ROOT / "diffusion_models_collection_amd" / "libdmc.so")
    prev = load(a.prev) if a.prev else None
    dev = torch.device("cuda", 0)
    smp = DDPM(device="cuda")
    T, N, C, HW = 1000, 128, 3, 32 * 32
    per = C * HW
    g = torch.Generator().manual_seed(0)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev)      # noqa: E731
    pred, x0, noise, out6 = mk(N, per), mk(N, per).clamp(-1, 1), mk(N, per), mk(N, 2 * per) * 0.5
    t = torch.randint(0, T, (N,), generator=g).to(dev)
    sa, s1 = smp.sqrt_alphas_cumprod.to(dev), smp.sqrt_one_minus_alphas_cumprod.to(dev)
    w = smp._snr_weights(5.0, dev)
    iw = torch.from_numpy(10.0 ** np.random.default_rng(1).uniform(-1, 1, T)).float().to(dev)
    coef = torch.from_numpy(_vlb.learned_coefficients(smp.alphas_cumprod.cpu().numpy(), "eps")).to(dev)
    one = torch.ones((), device=dev)
    loss, row = torch.empty(3, device=dev), torch.empty(N, device=dev)
    dpred, dout = torch.empty_like(pred), torch.empty_like(out6)
    ws = torch.empty(2 * 64 * N, device=dev)
    Kh = 10
    hist = torch.rand(T, Kh, device=dev)
    count = torch.full((T,), Kh, dtype=torch.int32, device=dev)
    u = torch.rand(N, device=dev)
    t_out = torch.empty(N, dtype=torch.long, device=dev)
    p_, iw_, cdf_ = (torch.empty(T, device=dev) for _ in range(3))
    rl = torch.rand(N, device=dev)

    def st():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def check(rc):
        assert rc == 0, rc

    def objective(lib):
        return lambda: check(lib.dmc_objective(0, 1, ptr(pred), ptr(x0), ptr(noise), ptr(t), ptr(sa), ptr(s1), ptr(w), T,
                                               N, per, ptr(one), ptr(loss), ptr(dpred), ptr(ws), st()))

    def hybrid(lib):
        return lambda: check(lib.dmc_hybrid_objective(0, 1, ptr(out6), ptr(x0), ptr(noise), ptr(t), ptr(sa), ptr(s1),
                                                      ptr(w), ptr(coef), T, N, per, 0.001, ptr(one), ptr(loss),
                                                      ptr(dout), ptr(ws), st()))

    arms = {}
    if prev is not None:
        arms["dmc_objective            --prev"] = objective(prev)
    arms["dmc_objective            this build"] = objective(new)
    arms["dmc_objective_is         iw + row_loss"] = lambda: check(new.dmc_objective_is(
        0, 1, ptr(pred), ptr(x0), ptr(noise), ptr(t), ptr(sa), ptr(s1), ptr(w), ptr(iw), T, N, per, ptr(one), ptr(loss),
        ptr(row), ptr(dpred), ptr(ws), st()))
    if prev is not None:
        arms["dmc_hybrid_objective     --prev"] = hybrid(prev)
    arms["dmc_hybrid_objective     this build"] = hybrid(new)
    arms["dmc_hybrid_objective_is  iw + row_loss"] = lambda: check(new.dmc_hybrid_objective_is(
        0, 1, ptr(out6), ptr(x0), ptr(noise), ptr(t), ptr(sa), ptr(s1), ptr(w), ptr(iw), ptr(coef), T, N, per, 0.001,
        ptr(one), ptr(loss), ptr(row), ptr(dout), ptr(ws), st()))
    arms["dmc_ts_history_update    T=1000 K=10 N=128"] = lambda: check(new.dmc_ts_history_update(
        ptr(t), ptr(rl), N, T, Kh, ptr(hist), ptr(count), st()))
    arms["dmc_ts_sample            T=1000 K=10 N=128"] = lambda: check(new.dmc_ts_sample(
        ptr(hist), ptr(count), T, Kh, 0.001, ptr(u), N, ptr(t_out), ptr(p_), ptr(iw_), ptr(cdf_), st()))
    graphs = {k: graph_of(fn) for k, fn in arms.items()}
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, gr in graphs.items():
            times[k].append(replay_us(gr))
    print(f"[{N}, {C}, 32, 32] fp32 (hybrid: [{N}, {2 * C}, 32, 32]), eps, l2, min-SNR weights, loss and gradient; "
          f"us per call, {CALLS} calls per graph replay, {a.rounds} interleaved rounds")
    for k, v in times.items():
        print(f"{k:44s} min {min(v):7.2f}  spread {max(v) - min(v):5.2f}  rounds " + " ".join(f"{x:6.2f}" for x in v),
              flush=True)


if __name__ == "__main__":
    main()
